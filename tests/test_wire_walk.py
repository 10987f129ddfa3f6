"""csrc/wire_spark.h (the byte-level structure walk of the SPARK wire format)
alone on the host under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/cpp/test_wire_walk.cpp -- the golden proof and commitment and a
synthetic CommitterKey are accepted; every truncation, one appended byte and
every Vec length prefix replaced by itself +- 1, by 0 and by 2^63 + 1 are
rejected; the sanitizers report nothing."""
import os
import subprocess

import spark_wire_ref as W
import sparse_eval_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wire_walk_host(tmp_path):
    from testudo_amd import r1cs_eval
    exe = str(tmp_path / "test_wire_walk")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_wire_walk.cpp"), "-o", exe], check=True)
    blobs, _raw = W.load_fixture()
    paths = []
    for name in ("proof", "commitment"):
        paths.append(str(tmp_path / (name + ".bin")))
        with open(paths[-1], "wb") as f:
            f.write(blobs[name])
    fx = S.load_fixture()
    sz = r1cs_eval.sizes(fx["num_cons"], fx["num_vars"], max(len(M) for M in fx["mats"]))
    args = [sz.derefs_rows, sz.ell_ops, sz.ell_mem, sz.ell_derefs, sz.log_ops, sz.log_cells]
    r = subprocess.run([exe] + paths + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) > len(blobs["proof"]) + len(blobs["commitment"])
    assert words[2:] == ["bad", "0"], r.stdout
