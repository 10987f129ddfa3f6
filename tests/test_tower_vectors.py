"""Host proof of the tower self-test's vectors (tests/tower_vectors.py, run on
the device by tests/test_tower_arith.py): every constructed class has its
defining property; the three references agree on every vector -- the Python
oracle (oracle/py/bls377.py), the linear forms both engines' tables encode
(tools/gen_wave_ops.py evaluate) and the exact model of rns_engine.h
(tools/gen_rns_ops.py: load, stage, store), whose internal asserts (64-bit
accumulators, beta < 15, CRT agreement of B' and the 2^32 channel, outputs
below 16 p) all hold on the RES edge operands; and field.h / pairing.h's own
host functions, compiled with g++ (tests/cpp/test_tower_ops.cpp), give the
same words, once more under AddressSanitizer and UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tower_vectors as V
from testudo_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = V.G
P = V.P
OPS = V.RNS_STAGES + ("inv",)


def test_constructed_classes_hold_their_properties():
    V.coeff_edges()
    V.mont_word_edges()
    V.structured()
    V.binary_pairs()
    V.res_slot_edges()
    V.res_vectors()
    V.g2_points()
    V.gt_pow_vectors()
    for op in V.WAVE_STAGES:
        V.wave_form_maximisers(op)
    c = V.COUNTS
    assert c["a coefficient edges"] == 6 * 12 + 7 + 2
    assert c["b Montgomery-word edges"] == 5 * 4 + 5
    assert c["c exact-multiple products"] >= 200 and c["a/b/f cross pairs"] >= 400
    assert c["d RES slot integers"] == 9 + 45 + 4 * 31 + 48
    assert c["e form maximisers f12_mul"] == 108 and c["e form maximisers cyc_sqr"] == 27
    assert c["e form maximisers conj"] == 12 and c["e form maximisers frob1"] >= 12
    assert c["g G2 points"] == 13 and c["f structured"] >= 16
    print("\n".join("%-40s %d" % kv for kv in sorted(c.items())))


def test_every_res_slot_integer_is_in_a_register():
    ints = {x for _, x in V.res_slot_edges()}
    assert {x for _, v in V.res_vectors() for x in v} == ints
    assert {0, 1, P - 1, P, P + 1, 8 * P, 15 * P, 16 * P - 2, 16 * P - 1} <= ints
    assert all(k * P + d in ints for k in range(1, 16) for d in (-1, 0, 1))
    for ch in range(31):
        m = G.lane_mod(ch) or 1 << 32
        assert {m - 1, m} <= ints
        assert max(x for x in ints if x % m == 0) == (16 * P - 1) // m * m
        assert max(x for x in ints if x % m == m - 1) == (16 * P - m) // m * m + m - 1


@pytest.mark.parametrize("op", OPS)
def test_references_agree_on_every_fq_vector(op):
    """oracle == linear forms == model of load -> stage -> store, per vector"""
    names, A, B = V.fq_operands("wave" if op in V.WAVE_STAGES + ("inv",) else "rns", op)
    if op == "f12_mul":  # the model on the classes' cross (thinned) and on all of class c and e
        keep = [i for i, n in enumerate(names) if not (" x " in n and i % 8)]
    else:
        keep = range(len(A))
    for i in range(len(A)):
        a, b = A[i], B[i] if B else None
        want = V.ref(op, a, b)
        assert V.wave_eval(op, a, b) == want, (op, names[i])
    for i in keep:
        a, b = A[i], B[i] if B else None
        want = V.ref(op, a, b)
        ra = [V.model_load(v * V.RQ % P) for v in a]
        rb = [V.model_load(v * V.RQ % P) for v in b] if b else None
        out = V.model_op(op, ra, rb)
        assert [V.model_store(r) for r in out] == [w * V.RQ % P for w in want], (op, names[i])


@pytest.mark.parametrize("op", OPS)
def test_model_asserts_hold_on_res_edges(op):
    """the model's internal asserts and the 16 p bound on class d (res_case
    raises otherwise), and the expected words stand for the oracle's values"""
    c = V.res_case(op)
    assert len(c.names) == len(c.exp) >= 23
    for row, inp in zip(V.res_lists(c.exp), c.inputs):
        want = V.ref(op, V.res_field(inp[:12]), V.res_field(inp[12:]) if len(inp) > 12 else None)
        assert [G.crt(r) * V.MBI % P for r in row] == want


def test_codec_cases():
    load, store = V.pass_cases()
    assert load.exp.shape == (len(load.names), 384) and store.exp.shape == (len(store.names), 144)


def test_python_op_table_matches_the_header(exe):
    """engine.py restates selftest_ops.h's tower op numbers and word counts"""
    r = subprocess.run([exe, "table"], capture_output=True, check=True)
    tab = np.frombuffer(r.stdout, dtype=np.int32).reshape(-1, 4)
    assert len(tab) == 1024
    for op, (valid, wa, wb, wo) in enumerate(tab):
        assert bool(valid) == E.selftest_tower_valid(op), op
        if valid:
            assert E.selftest_tower_words(op) == (wa, wb, wo), op
    for eng, names in E.SELFTEST_TOWER_ENGINE_OPS.items():
        for nm in names:
            assert tab[E.selftest_tower_op(eng, nm)][0] == 1


# ------------------------------------------ pairing.h's host functions ------
def _build(tmp, name, extra):
    out = str(tmp / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + extra + ["-I", os.path.join(ROOT, "testudo_amd", "csrc"),
                                                                  os.path.join(ROOT, "tests", "cpp", "test_tower_ops.cpp"), "-o", out],
                   check=True)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tower"), "test_tower_ops", ["-O2"])


def _run(exe, idx, a, b, wo):
    inp = struct.pack("<ii", idx, len(a)) + a.tobytes() + (b.tobytes() if b is not None else b"")
    r = subprocess.run([exe], input=inp, capture_output=True, check=True)
    return np.frombuffer(r.stdout, dtype=np.uint32).reshape(len(a), wo)


@pytest.mark.parametrize("op", OPS + ("final_exp",))
def test_host_tower_functions(exe, op):
    c = V.fq_case("rns", op)
    got = _run(exe, E.SELFTEST_TOWER_OPS[op], c.a, c.b, 144)
    bad = np.nonzero((got != c.exp).any(axis=1))[0]
    assert not len(bad), (op, len(bad), c.names[bad[0]], [hex(v) for v in c.inputs[bad[0]]])


def test_host_g2_prepare(exe):
    pts = [p for _, p in V.g2_points()]
    got = _run(exe, E.SELFTEST_TOWER_OPS["g2_prepare"], V.g2_words(pts), None, 69 * 72).reshape(len(pts), 69, 72)
    assert np.array_equal(got, V.g2_expected(pts))


def test_host_tower_functions_under_sanitizers(tmp_path):
    """the stand-alone host program once under ASan + UBSan (a plain binary
    with its own main)"""
    san = _build(tmp_path, "test_tower_ops_san", ["-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for op in ("f12_mul", "frob1", "inv", "final_exp"):
        c = V.fq_case("rns", op)
        n = 2 if op == "final_exp" else 4
        sel = slice(0, len(c.a), max(1, len(c.a) // n))
        a = np.ascontiguousarray(c.a[sel])
        b = None if c.b is None else np.ascontiguousarray(c.b[sel])
        assert np.array_equal(_run(san, E.SELFTEST_TOWER_OPS[op], a, b, 144), c.exp[sel]), op
    pts = [p for _, p in V.g2_points()][:3]
    got = _run(san, E.SELFTEST_TOWER_OPS["g2_prepare"], V.g2_words(pts), None, 69 * 72)
    assert np.array_equal(got.reshape(3, 69, 72), V.g2_expected(pts))
