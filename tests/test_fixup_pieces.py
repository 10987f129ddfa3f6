"""msm_pieces.h (the piece count the MSM's fixup kernels, the order kernel and
the long-list fixup share) on the host: tests/cpp/test_fixup_pieces.cpp --
a bucket inside one chunk, ending exactly on a chunk boundary, spanning
LONG_PARTS and LONG_PARTS + 1 chunks, empty, and a sweep against a direct
count of the chunks a bucket touches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixup_pieces_host(tmp_path):
    exe = str(tmp_path / "test_fixup_pieces")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_fixup_pieces.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    cases, bad = r.stdout.split()[1], r.stdout.split()[3]
    assert int(cases) > 30000 and bad == "0", r.stdout
