"""pairing_plan.h (the scratch sums of the pairing entry points, which are all
that keeps an Arena take inside its reservation) on the host:
tests/cpp/test_pairing_scratch.cpp replays the takes of multi_pairing_prepared,
mipp_lookahead (E = 1, 2, 4, 8), multi_pairing and gt_product_final for groups
in {1, 2, 8} and 17 pair counts from 0 to 4097, and checks
replayed <= scratch <= replayed + the fixed slack for each."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairing_scratch_host(tmp_path):
    exe = str(tmp_path / "test_pairing_scratch")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_pairing_scratch.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    cases, bad = r.stdout.split()[1], r.stdout.split()[3]
    # 3 groups x 17 counts x 3 entry points + 4 E x 16 counts + the level and size checks
    assert int(cases) == 3 * 17 * 3 + 4 * 16 + 6 + 1 and bad == "0", r.stdout
