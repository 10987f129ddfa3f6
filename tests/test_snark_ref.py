"""CPU tests of the TestudoSnark / TestudoNizk restatement (tests/snark_ref.py),
its fixtures, and the Instance / Assignment API (testudo_amd/instance.py):

  * prove -> verify in both modes, both sponges' end states;
  * every tamper of the list is rejected by the restated verifier, and leaves
    the caller's transcript untouched;
  * tests/golden/snark.json and snark_wire.json regenerate byte for byte;
  * Instance.new against the reference's vectors (lib.rs:302-344,
    testudo_snark.rs:298-335), the padded-constraints case, and the digest
    against a second, literal serialisation written here.
"""
import hashlib
import struct

import pytest

import snark_ref as N

R = N.R


@pytest.fixture(scope="module")
def case():
    return N.fixture_case()


@pytest.fixture(scope="module")
def other(case):
    """another instance of the same shape, proved on a transcript with another prefix"""
    return N.make_case(*N.FIXTURE_DIMS, N.FIXTURE_SEED + 1, N.FIXTURE_SRS_SEED, prefix=[7], gens=case["gens"],
                       nizk=False)


# ------------------------------------------------------------ both modes ----
def test_snark_prove_then_verify(case):
    ok, F = N.verify_case(case)
    assert ok and F.state() == case["f_end"]
    p = case["proof"]
    assert p["inst_evals"] == N.S.multi_evaluate(case["mats"], p["sat"]["rx"], p["sat"]["ry"])
    assert len(p["sat"]["rx"]) == 4 and len(p["sat"]["ry"]) == 5


def test_nizk_prove_then_verify(case):
    nz = case["nizk"]
    F = N.H.Transcript()
    assert N.nizk_verify(nz["proof"], case["mats"], case["dims"], case["digest"], case["inputs"], case["srs"], F)
    assert F.state() == nz["f_end"]
    bad = bytearray(case["digest"])
    bad[17] ^= 1
    G = N.H.Transcript()
    before = G.state()
    assert not N.nizk_verify(nz["proof"], case["mats"], case["dims"], bytes(bad), case["inputs"], case["srs"], G)
    assert G.state() == before
    # the two modes fork their sponges from different absorbs: different challenges, different proofs
    assert nz["c"] != case["c"] and nz["proof"]["rx"] != case["proof"]["sat"]["rx"]


def test_second_case_verifies_on_its_own_prefix(other):
    ok, _F = N.verify_case(other)
    assert ok
    ok, _F = N.verify_case(other, prefix=[])
    assert not ok


def test_short_witness_is_padded():
    """n_vars < num_vars: the restatement pads with zeros (lib.rs:99-113)"""
    assert N.pad_vars([5, 6], 4) == [5, 6, 0, 0] and N.pad_vars([], 4) == [0] * 4
    with pytest.raises(AssertionError):
        N.pad_vars([1] * 5, 4)


# --------------------------------------------------------------- tampers ----
def _tamper_ids():
    # the names depend on the fixture's sizes only: N = cells / 2 = 16
    return N.SAT_TAMPERS + N.EVALS_TAMPERS + [n for n, _ in N._eval_tamper_paths(4, 5)] + N.OTHER_TAMPERS


def test_tamper_list_is_complete(case):
    names = N.tamper_names(case)
    assert names == _tamper_ids() and len(set(names)) == len(names)
    assert len(N.SAT_TAMPERS) == 12  # every field of R1CSProof (r1csproof.rs:33-53)
    for part in ("comm_derefs[0]", "prod.proof_ops coefficient", "prod.proof_mem coefficient", "hash.eval_val[0]",
                 "hash.proof_derefs.z1", "hash.proof_ops.z1", "hash.proof_mem.z1"):
        assert part in names


@pytest.mark.parametrize("name", _tamper_ids())
def test_restated_verifier_rejects_tamper(case, other, name):
    t = N.apply_tamper(name, case, other)
    F = N.H.Transcript()
    F.append_scalars(t["prefix"])
    before = F.state()
    assert not N.snark_verify(t["proof"], case["dims"], t["inputs"], case["srs"], t["comm"], case["gens"], F)
    assert F.state() == before


# -------------------------------------------------------------- fixtures ----
def test_fixture_regenerates_byte_equal():
    with open(N.GOLDEN) as f:
        assert f.read() == N.dump_fixture(N.make_fixture())


def test_fixture_round_trips(case):
    fx = N.load_fixture()
    assert fx["dims"] == N.FIXTURE_DIMS and fx["mats"] == case["mats"] and fx["rnd"] == case["rnd"]
    assert fx["c"] == case["c"] and fx["f_end"] == case["f_end"] and fx["q_end"] == case["q_end"]
    assert N.ser_snark_proof(fx["proof"]) == N.ser_snark_proof(case["proof"])
    assert fx["nizk"]["digest"] == case["digest"] and fx["nizk"]["f_end"] == case["nizk"]["f_end"]
    ok, F = N.verify_case(case, proof=fx["proof"], comm=fx["comm"])
    assert ok and F.state() == fx["f_end"]


def test_wire_fixture_is_the_restatement():
    got, raw = N.load_wire_fixture()
    want = dict(zip(("snark_proof", "r1cs_proof"), N.fixture_bytes()))
    assert got == want
    for k, b in want.items():
        assert raw[k]["len"] == len(b) and raw[k]["sha256"] == hashlib.sha256(b).hexdigest()


def test_wire_layout_lengths(case):
    """the length of R1CSProof from its field list (r1csproof.rs:33-53) at 16 x 16: rounds_x = 4,
    rounds_y = 5, m_col = m_row = 2"""
    rx, ry, mc, mr = 4, 5, 2, 2
    want = (8 + 48) + (8 + rx * (8 + 4 * 32)) + 4 * 32 + (8 + ry * (8 + 3 * 32)) + 32 + (8 + mr * 96) + \
        (8 + rx * 32) + (8 + ry * 32) + 32 + 32 + 576 + (8 + mc * 2 * 576) + (8 + mc * 2 * 48) + 48 + 96 + (8 + mc * 48)
    b = N.ser_r1cs_proof(case["proof"]["sat"])
    assert len(b) == want
    assert struct.unpack_from("<Q", b, 0)[0] == mr
    whole = N.ser_snark_proof(case["proof"])
    assert whole[:len(b)] == b and whole[-96:] == b"".join(e.to_bytes(32, "little") for e in case["proof"]["inst_evals"])
    assert len(whole) == len(b) + len(N.W.ser_r1cs_eval_proof(case["proof"]["eval"])) + 96


# ---------------------------------------------------------- Instance.new ----
ZERO = bytes(32)
LARGER_THAN_MOD = bytes([3, 0, 0, 0, 255, 255, 255, 255, 254, 91, 254, 255, 2, 164, 189, 83, 5, 216, 161, 9, 8, 216, 57, 51,
                         72, 125, 157, 41, 83, 167, 237, 115])


def test_instance_invalid_index():
    """lib.rs:302-319"""
    from testudo_amd.instance import Instance, InvalidIndex
    A, B, C = [(0, 0, ZERO)], [(100, 1, ZERO)], [(1, 1, ZERO)]
    with pytest.raises(InvalidIndex):
        Instance.new(4, 8, 1, A, B, C)
    with pytest.raises(N.InvalidIndex):
        N.instance_new(4, 8, 1, A, B, C)
    with pytest.raises(InvalidIndex):  # a column past num_vars + 1 + num_inputs
        Instance.new(4, 8, 1, [(0, 10, ZERO)], [], [])
    Instance.new(4, 8, 1, [(0, 9, ZERO)], [], [])


def test_instance_invalid_scalar():
    """lib.rs:321-344: larger_than_mod is rejected whether or not the top bits are masked"""
    from testudo_amd.instance import Assignment, Instance, InvalidScalar, from_random_bytes
    A, B, C = [(0, 0, ZERO)], [(1, 1, LARGER_THAN_MOD)], [(1, 1, ZERO)]
    with pytest.raises(InvalidScalar):
        Instance.new(4, 8, 1, A, B, C)
    with pytest.raises(N.InvalidScalar):
        N.instance_new(4, 8, 1, A, B, C)
    raw = int.from_bytes(LARGER_THAN_MOD, "little")
    assert raw >= R and raw & ((1 << 253) - 1) >= R
    assert from_random_bytes(LARGER_THAN_MOD) is None and N.from_random_bytes(LARGER_THAN_MOD) is None
    with pytest.raises(InvalidScalar):
        Assignment.new([ZERO, LARGER_THAN_MOD])
    # the published rule: at most 32 bytes, zero-extended, little endian
    assert from_random_bytes(b"\x05") == 5 and from_random_bytes(bytes(33)) is None
    assert from_random_bytes((R - 1).to_bytes(32, "little")) == R - 1
    assert from_random_bytes(R.to_bytes(32, "little")) is None


def _padded():
    from testudo_amd.instance import Instance
    pc = N.padded_case()
    return pc, Instance.new(pc["num_cons"], pc["num_vars"], pc["num_inputs"], pc["A"], pc["B"], pc["C"])


def test_instance_padded_constraints():
    """testudo_snark.rs:298-335: 1 constraint, 0 variables, 3 inputs -> 2 x 4, the (1, inputs) block
    shifted to column 4, the zero entries of lib.rs:199-203 at (tups.len().., column num_vars)"""
    from testudo_amd.instance import Assignment, InvalidNumberOfInputs, padded_dims
    pc, inst = _padded()
    assert (inst.num_cons, inst.num_vars, inst.num_inputs) == (2, 4, 3)
    assert padded_dims(1, 0, 3) == (2, 4)
    assert inst.A == [(0, 6, 1), (1, 0, 0)] and inst.B == [(0, 6, 1), (1, 0, 0)]
    assert inst.C == [(0, 5, 1), (0, 4, R - 13), (0, 7, R - 1)]  # three entries: range(3, 2) is empty
    assert inst.num_nz_entries == 3
    want = N.instance_new(pc["num_cons"], pc["num_vars"], pc["num_inputs"], pc["A"], pc["B"], pc["C"])
    assert (inst.num_cons, inst.num_vars, inst.num_inputs, [inst.A, inst.B, inst.C]) == want
    vars_, inputs = Assignment.new(pc["vars"]), Assignment.new(pc["inputs"])
    assert inputs.assignment == [16, 1, 2] and len(vars_) == 0
    assert inst.is_sat_host(vars_, inputs)                          # 1 * 1 = 16 - 13 - 2
    assert not inst.is_sat_host(vars_, Assignment([16, 1, 3]))
    with pytest.raises(InvalidNumberOfInputs):
        inst.is_sat_host(vars_, Assignment([16, 1]))
    with pytest.raises(InvalidNumberOfInputs):
        inst.is_sat_host(Assignment([0] * 5), inputs)


@pytest.mark.parametrize("dims,want", [((0, 0, 0), (1, 1)), ((1, 0, 3), (2, 4)), ((3, 5, 1), (4, 8)), ((4, 8, 1), (4, 8)),
                                       ((5, 2, 2), (8, 4)), ((2, 4, 4), (2, 8))])
def test_padded_dims(dims, want):
    """lib.rs:137-167 literally; num_cons = 0 ends at 1 there (0usize.next_power_of_two() is 1)"""
    from testudo_amd.instance import padded_dims
    assert padded_dims(*dims) == want
    assert N.instance_new(*dims, [], [], [])[:2] == want


def test_digest_against_a_literal_serialisation():
    """r1csinstance.rs:155-164: SHAKE-256 (256 bytes) over the Compress::Yes bytes, written out by
    hand for the padded instance"""
    _pc, inst = _padded()
    u = lambda v: struct.pack("<Q", v)  # noqa: E731
    f = lambda v: (v % R).to_bytes(32, "little")  # noqa: E731
    lit = u(2) + u(4) + u(3)                                            # num_cons, num_vars, num_inputs
    lit += u(1) + u(3) + u(2) + u(0) + u(6) + f(1) + u(1) + u(0) + f(0)  # A: num_vars_x, num_vars_y, M
    lit += u(1) + u(3) + u(2) + u(0) + u(6) + f(1) + u(1) + u(0) + f(0)  # B
    lit += u(1) + u(3) + u(3) + u(0) + u(5) + f(1) + u(0) + u(4) + f(-13) + u(0) + u(7) + f(-1)  # C
    assert inst.serialize() == lit
    assert inst.digest == hashlib.shake_256(lit).digest(256) and len(inst.digest) == 256
    assert inst.digest == N.instance_digest(inst.num_cons, inst.num_vars, inst.num_inputs, [inst.A, inst.B, inst.C])


def test_digest_of_the_fixture_instance(case):
    from testudo_amd.instance import Instance
    inst = Instance.from_entries(*case["dims"], *case["mats"])
    assert inst.digest == case["digest"]
    changed = [list(M) for M in case["mats"]]
    r, c, v = changed[2][5]
    changed[2][5] = (r, c, (v + 1) % R)
    assert Instance.from_entries(*case["dims"], *changed).digest != case["digest"]
