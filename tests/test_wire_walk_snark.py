"""csrc/wire_snark.h (the byte-level structure walk of R1CSProof and of the
SNARK proof) alone on the host under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/test_wire_walk_snark.cpp -- the golden
byte strings of tests/golden/snark_wire.json are accepted; every truncation,
one appended byte and every length prefix replaced by itself +- 1, by 0 and by
2^63 + 1 are rejected; the sanitizers report nothing."""
import os
import subprocess

import snark_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wire_walk_snark_host(tmp_path):
    from testudo_amd import r1cs_eval
    exe = str(tmp_path / "test_wire_walk_snark")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_wire_walk_snark.cpp"), "-o", exe], check=True)
    blobs, _raw = N.load_wire_fixture()
    paths = []
    for name in ("snark_proof", "r1cs_proof"):
        paths.append(str(tmp_path / (name + ".bin")))
        with open(paths[-1], "wb") as f:
            f.write(blobs[name])
    num_cons, num_vars, _ni = N.FIXTURE_DIMS
    sz = r1cs_eval.sizes(num_cons, num_vars, num_cons)
    args = [num_cons, num_vars, sz.derefs_rows, sz.ell_ops, sz.ell_mem, sz.ell_derefs, sz.log_ops, sz.log_cells]
    r = subprocess.run([exe] + paths + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.stdout, r.stderr[-4000:])
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) > len(blobs["snark_proof"]) + len(blobs["r1cs_proof"])
    assert words[2:] == ["bad", "0"], r.stdout
