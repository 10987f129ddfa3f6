"""msm_pieces.h entry_flags / run_ends / run_slot on the host:
tests/cpp/test_entry_flags.cpp -- the flags k_sort_bin sets in the sorted
values mark exactly the first and last entry of every bucket, and the
flag-driven walk of the short-chunk accumulation sends every run where the
bounds predicate (bstart[key] >= c0, bend[key] <= c1) sent it, over random
sorted key arrays with empty buckets, several windows, a sentinel tail,
chunks of 2^3 .. 2^5 entries and window-group bounds that cut a chunk."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_flags_host(tmp_path):
    exe = str(tmp_path / "test_entry_flags")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_entry_flags.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    cases, bad = r.stdout.split()[1], r.stdout.split()[3]
    assert int(cases) > 30000 and bad == "0", r.stdout
