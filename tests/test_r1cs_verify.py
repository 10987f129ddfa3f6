"""R1CS proof verification and the device R1CSInstance::evaluate.

  evaluate   tpst_r1cs_evaluate (r1csinstance.rs:308-311) bit-exact against
             sum val eq(rx)[row] eq(ry)[col] in Python, and against the cell
             sums at boolean points
  is_sat     tpst_r1cs_is_sat (r1csinstance.rs:244-274)
  verify     tpst_r1cs_verify / tpst_r1cs_verify_evals: the ten checks of the
             verifier circuit (constraints.rs:263-397) and Polynomial::verify
             (r1csproof.rs:469-480); `_py_verify` below restates them over
             oracle/py and is the reference semantics of the tamper list: the
             CPU test shows it rejects every tamper, the GPU test that the
             library does.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import bls377 as O
import pst as P
import r1cs as Q
from testudo_amd.encoding import fr_array, limbs_to_int, ptr

R = O.R
SRS_SEED = 0x7E57D1


def _ints(a):
    return [limbs_to_int(x) for x in np.asarray(a).reshape(-1, 4)]


def _py_evaluate(mats, rx, ry):
    """R1CSInstance::evaluate: sum over every entry of val eq(rx)[row] eq(ry)[col]."""
    ex, ey = Q.eq_evals(rx), Q.eq_evals(ry)
    return [sum(val * ex[r] * ey[c] for r, c, val in M) % R for M in mats]


def _py_verify(p, evals, inputs, num_cons, num_vars, srs, tr):
    """The ten steps of tpst_r1cs_verify_evals over the oracle: p is the dict
    Q.r1cs_prove returns (rounds_x / rounds_y / num_vars_log default to the
    lengths of its vectors).  r_abc and claims2 are never read."""
    nlog = Q.log2(num_vars)
    rounds_x, rounds_y = Q.log2(num_cons), nlog + 1
    if (p.get("rounds_x", len(p["sc1"])), p.get("rounds_y", len(p["sc2"])), p.get("num_vars_log", p["n_vars"])) != \
            (rounds_x, rounds_y, nlog):
        return False
    if len(p["sc1"]) != rounds_x or len(p["sc2"]) != rounds_y or len(p["rx"]) != rounds_x or len(p["ry"]) != rounds_y:
        return False
    frs = [p["initial_state"], p["transcript_sat_state"], p["eval_vars_at_ry"], *p["claims_phase2"], *p["rx"],
           *p["ry"], *[c for cs in p["sc1"] for c in cs], *[c for cs in p["sc2"] for c in cs], *evals, *inputs]
    if any(not 0 <= x < R for x in frs):
        return False
    # 1. commitment, initial state, inputs
    tr.append_gt(p["T"])
    if tr.challenge_scalar() != p["initial_state"]:
        return False
    Q.new_from_state2(tr, p["initial_state"])
    for x in inputs:
        Q.append_scalar(tr, x)
    # 2. tau
    tau = [tr.challenge_scalar() for _ in range(rounds_x)]
    # 3. phase one
    try:
        e1, rx = Q.sumcheck_verify(p["sc1"], 0, 3, tr)
    except AssertionError:
        return False
    # 4.
    if rx != list(p["rx"]):
        return False
    # 5.
    az, bz, cz, azbz = p["claims_phase2"]
    tb = 1
    for t, r in zip(tau, rx):
        tb = tb * (t * r + (1 - t) * (1 - r)) % R
    if azbz != az * bz % R or e1 != (azbz - cz) * tb % R:
        return False
    # 6. phase two
    ra, rb, rc = (tr.challenge_scalar() for _ in range(3))
    try:
        e2, ry = Q.sumcheck_verify(p["sc2"], (ra * az + rb * bz + rc * cz) % R, 2, tr)
    except AssertionError:
        return False
    # 7.
    if ry != list(p["ry"]):
        return False
    # 8. z(ry) and the matrix evaluations
    chi = Q.eq_evals(ry[1:])
    io = sum(a * b for a, b in zip([1] + list(inputs), chi)) % R
    zry = ((1 - ry[0]) * p["eval_vars_at_ry"] + ry[0] * io) % R
    if e2 != zry * (ra * evals[0] + rb * evals[1] + rc * evals[2]) % R:
        return False
    # 9.
    if tr.challenge_scalar() != p["transcript_sat_state"]:
        return False
    Q.new_from_state2(tr, p["transcript_sat_state"])
    # 10. Polynomial::verify of the witness opening
    return bool(P.Polynomial.verify(tr, srs, p["U"], ry[1:], p["eval_vars_at_ry"], p["pst_proof"], p["mipp"], p["T"]))


# Every tamper changes one thing of a valid (proof, instance, inputs,
# transcript, evals) tuple.  The same names drive the oracle restatement (CPU)
# and the library (GPU).
TAMPERS = ["sc1_coeff", "sc2_coeff", "claims_phase2_0", "claims_phase2_3", "rx_1", "ry_0", "ry_2",
           "eval_vars_at_ry", "transcript_sat_state", "initial_state", "T", "input", "extra_append",
           "matrix_value", "evals_1", "final_a", "non_canonical", "rounds_x"]


# ------------------------------------------------------------------ CPU ----
CPU_SHAPE = (32, 16, 3)


@pytest.fixture(scope="module")
def oracle_case():
    num_cons, num_vars, num_inputs = CPU_SHAPE
    mats, v, x = Q.synthetic_r1cs(num_cons, num_vars, num_inputs, 7)
    srs = P.SRS(2, 9)
    out = Q.r1cs_prove(mats, num_cons, num_vars, v, x, srs, P.PoseidonTranscript())
    return {"mats": mats, "inputs": x, "srs": srs, "proof": out, "evals": _py_evaluate(mats, out["rx"], out["ry"])}


def _oracle_run(case, name=None):
    num_cons, num_vars, _ = CPU_SHAPE
    p = copy.deepcopy(case["proof"])
    mats, inputs, evals = case["mats"], list(case["inputs"]), list(case["evals"])
    tr = P.PoseidonTranscript()
    bump = lambda v: (v + 1) % R  # noqa: E731
    if name == "sc1_coeff":
        p["sc1"][1][2] = bump(p["sc1"][1][2])
    elif name == "sc2_coeff":
        p["sc2"][2][1] = bump(p["sc2"][2][1])
    elif name == "claims_phase2_0":
        c = list(p["claims_phase2"])
        c[0] = bump(c[0])
        p["claims_phase2"] = tuple(c)
    elif name == "claims_phase2_3":
        c = list(p["claims_phase2"])
        c[3] = bump(c[3])
        p["claims_phase2"] = tuple(c)
    elif name == "rx_1":
        p["rx"][1] = bump(p["rx"][1])
    elif name == "ry_0":
        p["ry"][0] = bump(p["ry"][0])
    elif name == "ry_2":
        p["ry"][2] = bump(p["ry"][2])
    elif name in ("eval_vars_at_ry", "transcript_sat_state", "initial_state"):
        p[name] = bump(p[name])
    elif name == "T":
        p["T"] = O.f12_mul(p["T"], p["T"])  # another element of GT
    elif name == "input":
        inputs[0] = bump(inputs[0])
    elif name == "extra_append":
        Q.append_scalar(tr, 1)
    elif name == "matrix_value":
        Cm = list(mats[2])
        r, c, val = Cm[5]
        Cm[5] = (r, c, bump(val))
        evals = _py_evaluate((mats[0], mats[1], Cm), p["rx"], p["ry"])
    elif name == "evals_1":
        evals[1] = bump(evals[1])
    elif name == "final_a":
        p["mipp"] = dict(p["mipp"], final_a=O.g1_mul(O.G1_GEN, 5))
    elif name == "non_canonical":
        c = list(p["claims_phase2"])
        c[1] = R
        p["claims_phase2"] = tuple(c)
    elif name == "rounds_x":
        p["rounds_x"] = len(p["sc1"]) + 1
    else:
        assert name is None
    return _py_verify(p, evals, inputs, num_cons, num_vars, case["srs"], tr)


def test_py_verify_accepts_oracle_proof(oracle_case):
    assert _oracle_run(oracle_case) is True


@pytest.mark.parametrize("name", TAMPERS)
def test_py_verify_rejects_tamper(oracle_case, name):
    """Every entry of the tamper list is a rejection under the reference semantics."""
    assert _oracle_run(oracle_case, name) is False


def test_binding_declares_verifier_symbols():
    from testudo_amd import _lib
    lib = _lib.load()
    for s in ("tpst_r1cs_evaluate", "tpst_r1cs_is_sat", "tpst_r1cs_verify_evals", "tpst_r1cs_verify"):
        assert s in _lib.exported_symbols() and hasattr(lib, s)


# ------------------------------------------------------------------ GPU ----
def _srs(ctx, num_vars):
    from testudo_amd import sqrt_pst as S
    S.srs_setup(ctx, (Q.log2(num_vars) + 1) // 2, SRS_SEED)


def _prove(ctx, num_cons, num_vars, num_inputs, seed):
    from testudo_amd import r1cs as D
    from testudo_amd import sqrt_pst as S
    _srs(ctx, num_vars)
    inst, vars_, inputs = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, seed)
    proof, _, _ = D.R1CSProof.prove(inst, vars_, inputs, S.PoseidonTranscript())
    return inst, vars_, inputs, proof


def _points(seed, rx_n, ry_n):
    vals, _ = P.fr_stream(seed, rx_n + ry_n)
    vals = list(vals)
    return vals[:rx_n], vals[rx_n:]


def _check_evaluate(inst, mats, rx, ry):
    got = _ints(inst.evaluate(fr_array(rx), fr_array(ry)))
    assert got == _py_evaluate(mats, rx, ry)


@pytest.mark.gpu
@pytest.mark.parametrize("num_cons,num_vars,num_inputs", [(16, 16, 3), (256, 64, 10)])
def test_evaluate_synthetic_vs_python(ctx, num_cons, num_vars, num_inputs):
    """(16, 16, 3) has fewer rows than one wave; (256, 64, 10) fills one block."""
    from testudo_amd import r1cs as D
    inst, _, _ = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, 500 + num_cons)
    mats, _, _ = Q.synthetic_r1cs(num_cons, num_vars, num_inputs, 500 + num_cons)
    rx, ry = _points(77, Q.log2(num_cons), Q.log2(num_vars) + 1)
    _check_evaluate(inst, mats, rx, ry)


def _loaded_mats():
    """64 x (2 * 16): shuffled order, repeated cells, C empty, row 7 with 300
    entries, rows used: 0, 7, 13, 63 only (A) -- every other row is empty --
    entries in the constant column 16, the input columns 17..20 and the last
    column 31, the values 1 and r - 1."""
    rng = np.random.default_rng(11)
    val = lambda: int(rng.integers(1, 2 ** 62)) * int(rng.integers(1, 2 ** 62)) % R  # noqa: E731
    A = [(7, int(rng.integers(32)), val()) for _ in range(300)]
    A += [(0, 0, 1), (0, 0, R - 1), (0, 0, 5), (63, 31, R - 1), (63, 31, 1), (63, 31, 9), (13, 16, 1), (13, 16, val()),
          (13, 17, val()), (13, 20, R - 1), (0, 31, val()), (63, 0, val()), (63, 16, 1)]
    B = [(int(rng.integers(64)), int(rng.integers(32)), val()) for _ in range(90)] + [(5, 18, 1), (5, 19, R - 1)]
    Cm = []
    A = [A[i] for i in rng.permutation(len(A))]
    B = [B[i] for i in rng.permutation(len(B))]
    return A, B, Cm


def _load(ctx, mats, num_cons=64, num_vars=16, num_inputs=4):
    from testudo_amd import r1cs as D
    enc = lambda M: [(r, c, fr_array([v])[0]) for (r, c, v) in M]  # noqa: E731
    return D.R1CSInstance.new(ctx, num_cons, num_vars, num_inputs, *[enc(M) for M in mats])


def _bits(i, n):
    return [(i >> (n - 1 - j)) & 1 for j in range(n)]


@pytest.mark.gpu
def test_evaluate_loaded_instance_vs_python(ctx):
    mats = _loaded_mats()
    inst = _load(ctx, mats)
    rx, ry = _points(78, 6, 5)
    _check_evaluate(inst, mats, rx, ry)
    # coordinates 0, 1 and r - 1 mixed with random ones
    _check_evaluate(inst, mats, [0, rx[1], 1, R - 1, rx[4], 1], [R - 1, 0, ry[2], 1, ry[4]])
    _check_evaluate(inst, mats, [1, 1, R - 1, rx[3], 0, 0], [ry[0], R - 1, 1, 0, 0])


@pytest.mark.gpu
def test_evaluate_boolean_points_are_cell_sums(ctx):
    """rx = bits(row), ry = bits(col), MSB-first: the sum of the entries at that cell."""
    mats = _loaded_mats()
    inst = _load(ctx, mats)

    def cell(row, col):
        return [sum(v for r, c, v in M if (r, c) == (row, col)) % R for M in mats]

    # all zeros (a repeated cell of A: 1 + (r - 1) + 5), all ones (repeated: (r - 1) + 1 + 9),
    # a repeated cell of row 7, an empty cell (row 1 is empty in A; whatever B holds there)
    seven = [c for r, c, _ in mats[0] if r == 7]
    rep = next(c for c in seven if seven.count(c) > 1)
    for row, col in [(0, 0), (63, 31), (7, rep), (1, 3), (13, 16)]:
        got = _ints(inst.evaluate(fr_array(_bits(row, 6)), fr_array(_bits(col, 5))))
        assert got == cell(row, col), (row, col)
    assert cell(0, 0)[0] == 5 and cell(63, 31)[0] == 9 and cell(1, 3)[0] == 0 and cell(0, 0)[2] == 0


@pytest.mark.gpu
def test_evaluate_more_rows_than_threads(ctx):
    """The kernel launches at most EV_MAX_BLOCKS = 128 blocks of EV_BS = 256
    threads per matrix (csrc/r1cs.hip): 32768 lanes.  2^16 rows make every lane
    take two rows of the grid-stride loop."""
    from testudo_amd import r1cs as D
    num_cons, num_vars, num_inputs = 1 << 16, 16, 3
    inst, _, _ = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, 91)
    mats, _, _ = Q.synthetic_r1cs(num_cons, num_vars, num_inputs, 91)
    rx, ry = _points(79, 16, 5)
    _check_evaluate(inst, mats, rx, ry)


@pytest.mark.gpu
def test_evaluate_argument_errors(ctx):
    from testudo_amd import Context
    from testudo_amd import r1cs as D
    from testudo_amd.engine import TpstError
    inst, _, _ = D.R1CSInstance.produce_synthetic_r1cs(ctx, 16, 16, 3, 31)
    rx, ry = _points(80, 4, 5)
    with pytest.raises(TpstError, match=r"\(-1\)"):
        inst.evaluate(fr_array([rx[0], R, rx[2], rx[3]]), fr_array(ry))
    with pytest.raises(TpstError, match=r"\(-1\)"):
        inst.evaluate(fr_array(rx), fr_array(ry[:4] + [2 ** 256 - 1]))
    other = Context(0)
    try:
        out = np.zeros((3, 4), dtype=np.uint64)
        assert other.lib.tpst_r1cs_evaluate(other.h, inst.h, ptr(fr_array(rx)), ptr(fr_array(ry)), ptr(out)) == -1
    finally:
        other.close()


@pytest.mark.gpu
def test_is_sat(ctx):
    from testudo_amd import r1cs as D
    num_cons, num_vars, num_inputs = 64, 16, 4
    inst, vars_, inputs = D.R1CSInstance.produce_synthetic_r1cs(ctx, num_cons, num_vars, num_inputs, 4242)
    assert inst.is_sat(vars_, inputs) is True
    bad = vars_.copy()
    bad[3, 0] ^= np.uint64(1)
    assert inst.is_sat(bad, inputs) is False
    bad = inputs.copy()
    bad[1, 0] ^= np.uint64(1)
    assert inst.is_sat(vars_, bad) is False
    # the "extra entries in A" instance of test_r1cs_load_general_matrices
    mats, v, x = Q.synthetic_r1cs(num_cons, num_vars, num_inputs, 4242)
    assert _ints(vars_) == v and _ints(inputs) == x
    rng = np.random.default_rng(5)
    extra = [(int(rng.integers(num_cons)), int(rng.integers(2 * num_vars)), int(rng.integers(1, 2 ** 60)))
             for _ in range(40)]
    assert _load(ctx, mats).is_sat(vars_, inputs) is True
    assert _load(ctx, (mats[0] + extra, mats[1], mats[2])).is_sat(vars_, inputs) is False


@pytest.mark.gpu
@pytest.mark.parametrize("num_cons,num_vars,num_inputs", [(16, 16, 3), (64, 16, 5), (32, 32, 0)])
def test_verify_accepts_device_proof(ctx, num_cons, num_vars, num_inputs):
    from testudo_amd import sqrt_pst as S
    inst, _, inputs, proof = _prove(ctx, num_cons, num_vars, num_inputs, 2000 + num_cons)
    assert proof.verify(inst, inputs, S.PoseidonTranscript()) is True
    evals = inst.evaluate(proof.rx, proof.ry)
    assert proof.verify(inst, inputs, S.PoseidonTranscript(), evals=evals) is True
    # r_abc and claims_z_abc are not read
    blind = copy.deepcopy(proof)
    blind.r_abc[:] = 0
    blind.claims_z_abc[:] = 0
    assert blind.verify(inst, inputs, S.PoseidonTranscript()) is True
    assert blind.verify(inst, inputs, S.PoseidonTranscript(), evals=evals) is True


REJECT_SHAPE = (64, 16, 5)
REJECT_SEED = 2064


@pytest.fixture(scope="module")
def device_case(ctx):
    inst, vars_, inputs, proof = _prove(ctx, *REJECT_SHAPE, REJECT_SEED)
    return {"inst": inst, "inputs": inputs, "proof": proof, "evals": inst.evaluate(proof.rx, proof.ry)}


def _bump(a):
    """canonical Fr limbs + 1 (mod r), in place"""
    a[...] = fr_array([(limbs_to_int(a) + 1) % R])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", TAMPERS)
def test_verify_rejects_tamper(ctx, device_case, name):
    """One change from a fresh copy of a valid (64, 16, 5) proof: False
    (TPST_E_VERIFY), never an exception."""
    from testudo_amd import r1cs as D
    from testudo_amd import sqrt_pst as S
    _srs(ctx, REJECT_SHAPE[1])
    inst, inputs, evals = device_case["inst"], device_case["inputs"].copy(), None
    p = copy.deepcopy(device_case["proof"])
    tr = S.PoseidonTranscript()
    if name == "sc1_coeff":
        _bump(p.sc_proof_phase1[1, 2])
    elif name == "sc2_coeff":
        _bump(p.sc_proof_phase2[2, 1])
    elif name == "claims_phase2_0":
        _bump(p.claims_phase2[0])
    elif name == "claims_phase2_3":
        _bump(p.claims_phase2[3])
    elif name == "rx_1":
        _bump(p.rx[1])
    elif name == "ry_0":
        _bump(p.ry[0])
    elif name == "ry_2":
        _bump(p.ry[2])
    elif name in ("eval_vars_at_ry", "transcript_sat_state", "initial_state"):
        _bump(getattr(p, name))
    elif name == "T":  # the GT of another commitment
        other, _ = S.fr_stream(5, 16)
        _, T2 = S.Polynomial.from_evaluations(ctx, other).commit()
        assert not np.array_equal(T2, p.T)
        p.T = np.asarray(T2, dtype=np.uint64).reshape(72)
    elif name == "input":
        _bump(inputs[0])
    elif name == "extra_append":
        D.transcript_append_scalar(tr, fr_array([1]))
    elif name == "matrix_value":
        mats, _, _ = Q.synthetic_r1cs(*REJECT_SHAPE, REJECT_SEED)
        assert _load(ctx, mats, *REJECT_SHAPE).evaluate(p.rx, p.ry).tolist() == device_case["evals"].tolist()
        Cm = list(mats[2])
        r, c, val = Cm[5]
        Cm[5] = (r, c, (val + 1) % R)
        inst = _load(ctx, (mats[0], mats[1], Cm), *REJECT_SHAPE)
    elif name == "evals_1":
        evals = device_case["evals"].copy()
        _bump(evals[1])
    elif name == "final_a":
        p.mipp_proof.final_a = ctx.g1_mul_generator(fr_array([5]))[0]
    elif name == "non_canonical":
        p.claims_phase2[1] = fr_array([R])[0]
    elif name == "rounds_x":
        pr = p.pack()
        assert ctx.lib.tpst_r1cs_verify(ctx.h, inst.h, ptr(inputs), C.byref(tr.t), C.byref(pr)) == 0
        pr.rounds_x += 1
        tr = S.PoseidonTranscript()
        assert ctx.lib.tpst_r1cs_verify(ctx.h, inst.h, ptr(inputs), C.byref(tr.t), C.byref(pr)) == -5
        return
    assert p.verify(inst, inputs, tr, evals=evals) is False


@pytest.mark.gpu
def test_verify_without_srs_is_a_state_error(ctx, device_case):
    """A fresh context has no SRS: TPST_E_STATE raised, not False."""
    from testudo_amd import Context
    from testudo_amd import r1cs as D
    from testudo_amd import sqrt_pst as S
    from testudo_amd.engine import TpstError
    other = Context(0)
    try:
        inst, _, inputs = D.R1CSInstance.produce_synthetic_r1cs(other, *REJECT_SHAPE, REJECT_SEED)
        with pytest.raises(TpstError, match=r"\(-4\)"):
            device_case["proof"].verify(inst, inputs, S.PoseidonTranscript())
        with pytest.raises(TpstError, match=r"\(-4\)"):
            device_case["proof"].verify(inst, inputs, S.PoseidonTranscript(), evals=device_case["evals"])
        del inst
    finally:
        other.close()
