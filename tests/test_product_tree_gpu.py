"""GPU tests of the grand-product argument (csrc/product_tree.hip):
ProductCircuitEvalProofBatched::prove on the device, bit-exact against the
first-principles restatement tests/product_tree_ref.py and the fixture
tests/golden/product_tree.json; the host verifier on the device's proofs."""
import ctypes as C
import functools

import numpy as np
import pytest

import product_tree_ref as T
from testudo_amd.encoding import fr_array, limbs_to_int, ptr

pytestmark = pytest.mark.gpu

R = T.R
ROUND_BS = 256  # csrc/product_tree.hip PT_BS: lanes per block of the round kernel
E_ARG = -1
# (ell, P, D): no rounds at all; the smallest with rounds and dot products; the
# fixture's; layer 0's tables are exactly one block long (2^(ell-1) = PT_BS); its
# first round's sums fill exactly one block (2^(ell-2) = PT_BS lanes); several
# blocks and a reduce over more than one partial, with and without dot products
SHAPES = [(1, 1, 0), (2, 2, 2), (3, 2, 2), (9, 3, 2), (10, 3, 2), (11, 3, 2), (13, 2, 0)]
assert 1 << (9 - 1) == ROUND_BS and 1 << (10 - 2) == ROUND_BS


def _inputs(ell, P, D):
    if (ell, P, D) == (3, 2, 2):  # the fixture's inputs
        import golden_io as G
        c = T.load_case(G.load("product_tree.json")["cases"][0])
        return c["polys"], c["dotp"]
    polys, dotps, _whole = T.random_inputs(ell, P, D, 9000 + 100 * ell + 10 * P + D, special=ell in (9, 10))
    return polys, dotps


@functools.lru_cache(maxsize=None)
def _reference(ell, P, D):
    """the restatement's run for _inputs(ell, P, D), computed once"""
    polys, dotps = _inputs(ell, P, D)
    return T.run(polys, dotps)


def _arrays(polys, dotps):
    pa = np.stack([fr_array(p) for p in polys])
    if not dotps:
        return pa, None
    return pa, tuple(np.stack([fr_array(d[k]) for d in dotps]) for k in range(3))


def _ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[o:o + 32], "little") for o in range(0, len(b), 32)]


def _state(tr):
    st, sq, idx = tr.state()
    return [limbs_to_int(x) for x in st], sq, idx


def _to_device(ctx, a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", ctx.device))
    ctx.torch_to_lib()
    return d


def _same_as_reference(v, ell, P, D, proof, cp, cd, rand, tr):
    assert _ints(cp) == v["claims_prod"]
    assert _ints(cd) == v["claims_dotp"]
    assert _ints(proof.pack()) == T.flatten(v["proof"], ell, P, D)  # every coefficient and claim
    assert _ints(rand) == v["rand"]
    assert _state(tr) == v["transcript_end"]


@pytest.mark.parametrize("ell,P,D", SHAPES)
def test_prove_bit_exact_vs_restatement(ctx, ell, P, D):
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript
    v = _reference(ell, P, D)
    pa, da = _arrays(*_inputs(ell, P, D))
    # the host-pointer entry
    tr = FrTranscript()
    proof, cp, cd, rand = PT.prove(ctx, pa, da, tr)
    _same_as_reference(v, ell, P, D, proof, cp, cd, rand, tr)
    # the _dev entry; its inputs stay byte-identical
    d_p = _to_device(ctx, pa)
    d_d = [_to_device(ctx, a) for a in da] if da else [None] * 3
    tr2 = FrTranscript()
    proof2, cp2, cd2, rand2 = PT.prove_dev(ctx, ell, P, d_p.data_ptr(), D,
                                           *[a.data_ptr() if a is not None else 0 for a in d_d], tr2)
    _same_as_reference(v, ell, P, D, proof2, cp2, cd2, rand2, tr2)
    ctx.synchronize()
    assert np.array_equal(d_p.cpu().numpy().view(np.uint64).reshape(pa.shape), pa)
    for a, b in zip(d_d, da or []):
        assert np.array_equal(a.cpu().numpy().view(np.uint64).reshape(b.shape), b)
    # the host verifier accepts the device's proof and returns the restatement's claims
    vt = FrTranscript()
    res = PT.verify(cp, cd, proof, vt)
    assert res is not False
    assert _ints(res[0]) == v["claims_out"] and _ints(res[1]) == v["claims_dotp_out"] and _ints(res[2]) == v["rand"]
    assert _state(vt) == v["transcript_end"]


def test_fixture(ctx):
    """the committed fixture itself (not a rerun of the restatement)"""
    import golden_io as G
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript
    c = T.load_case(G.load("product_tree.json")["cases"][0])
    pa, da = _arrays(c["polys"], c["dotp"])
    tr = FrTranscript()
    proof, cp, cd, rand = PT.prove(ctx, pa, da, tr)
    _same_as_reference(c, c["ell"], c["P"], c["D"], proof, cp, cd, rand, tr)


def test_two_proofs_chain_on_one_transcript(ctx):
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript
    shapes = [(4, 2, 2), (3, 1, 0)]
    rt, tr = T.Transcript(), FrTranscript()
    for ell, P, D in shapes:
        polys, dotps, _ = T.random_inputs(ell, P, D, 9500 + ell)
        ref_proof, ref_rand = T.prove([T.product_circuit(p) for p in polys], dotps, rt)
        proof, _cp, _cd, rand = PT.prove(ctx, *_arrays(polys, dotps), tr)
        assert _ints(proof.pack()) == T.flatten(ref_proof, ell, P, D)
        assert _ints(rand) == ref_rand
        assert _state(tr) == rt.state()


def test_zero_entry_gives_a_zero_product(ctx):
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript
    polys, dotps, _ = T.random_inputs(4, 2, 0, 9600)
    polys[1][9] = 0
    v = T.run(polys, dotps)
    assert v["claims_prod"][1] == 0
    tr = FrTranscript()
    proof, cp, cd, rand = PT.prove(ctx, *_arrays(polys, dotps), tr)
    _same_as_reference(v, 4, 2, 0, proof, cp, cd, rand, tr)
    assert PT.verify(cp, cd, proof, FrTranscript()) is not False


def test_self_consistency_ell18(ctx):
    """random inputs at a size the restatement is too slow for: verify accepts,
    and every returned claim is the evaluation the argument stands for"""
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript, dense_evaluate
    from testudo_amd.sqrt_pst import fr_stream
    ell, P, D = 18, 2, 2
    n = 1 << ell
    polys, k = fr_stream(0x5054_0018, P * n)
    whole, _ = fr_stream(0x5054_0018, 3 * n, k)  # one unsplit (left, right, weight) triple
    polys = polys.reshape(P, n, 4)
    whole = whole.reshape(3, n, 4)
    # DotProductCircuit::split: circuits 0 / 1 = the halves of the triple
    da = tuple(np.ascontiguousarray(whole[j].reshape(2, n // 2, 4)) for j in range(3))
    proof, cp, cd, rand = PT.prove(ctx, polys, da, FrTranscript())
    res = PT.verify(cp, cd, proof, FrTranscript())
    assert res is not False
    claims, claims_dotp, vrand = res
    assert np.array_equal(vrand, rand)
    for p in range(P):
        assert np.array_equal(claims[p], dense_evaluate(ctx, polys[p], rand))
        acc = 1
        for x in _ints(polys[p]):
            acc = acc * x % R
        assert limbs_to_int(cp[p]) == acc
    for j in range(3):
        assert np.array_equal(claims_dotp[j], dense_evaluate(ctx, whole[j], rand))
    w = [_ints(whole[j]) for j in range(3)]
    for d in range(2):
        sl = slice(d * (n // 2), (d + 1) * (n // 2))
        assert limbs_to_int(cd[d]) == sum(a * b * c for a, b, c in zip(w[0][sl], w[1][sl], w[2][sl])) % R


def test_grid_stride_rounds_ell19(ctx):
    """2^(ell-2) lanes of layer 0's first round exceed the round kernel's block
    cap (csrc/product_tree.hip PT_MAX_BLOCKS = 256 blocks of 256 lanes per
    instance), so its lanes loop: the one path no smaller shape takes"""
    from testudo_amd import product_tree as PT
    from testudo_amd.hyrax import FrTranscript, dense_evaluate
    from testudo_amd.sqrt_pst import fr_stream
    ell = 19
    assert 1 << (ell - 2) > 256 * ROUND_BS
    poly, _ = fr_stream(0x5054_0019, 1 << ell)
    proof, cp, cd, rand = PT.prove(ctx, poly.reshape(1, 1 << ell, 4), None, FrTranscript())
    res = PT.verify(cp, cd, proof, FrTranscript())
    assert res is not False and np.array_equal(res[2], rand)
    assert np.array_equal(res[0][0], dense_evaluate(ctx, poly, rand))
    acc = 1
    for x in _ints(poly):
        acc = acc * x % R
    assert limbs_to_int(cp[0]) == acc


def test_bad_arguments(ctx):
    """TPST_E_ARG, no aborts"""
    from testudo_amd import product_tree as PT
    from testudo_amd.engine import TpstError
    from testudo_amd.hyrax import FrTranscript
    ell, P, D = 3, 2, 2
    polys, dotps = _inputs(ell, P, D)
    pa, da = _arrays(polys, dotps)
    lib = ctx.lib
    z = lambda n: np.zeros((n, 4), dtype=np.uint64)  # noqa: E731
    proof, cp, cd, rand = z(PT.proof_len(ell, P, D) + 64), z(P), z(4), z(ell)

    def call(ell=ell, P=P, D=D, null=None, pa=pa, da=da, tr=None):
        tr = tr or FrTranscript()
        a = {"polys": pa, "l": da[0], "r": da[1], "w": da[2], "proof": proof, "cp": cp, "cd": cd, "rand": rand}
        p = {k: (None if k == null else ptr(v)) for k, v in a.items()}
        return lib.tpst_prodcircuit_prove(ctx.h, ell, P, p["polys"], D, p["l"], p["r"], p["w"],
                                          None if null == "tr" else C.byref(tr.t), p["proof"], p["cp"], p["cd"],
                                          p["rand"])

    assert call() == 0
    for null in ("polys", "l", "r", "w", "tr", "proof", "cp", "cd", "rand"):
        assert call(null=null) == E_ARG, null
    assert lib.tpst_prodcircuit_prove(None, ell, P, ptr(pa), 0, None, None, None, C.byref(FrTranscript().t),
                                      ptr(proof), ptr(cp), None, ptr(rand)) == E_ARG
    assert call(ell=0) == E_ARG
    assert call(ell=31) == E_ARG
    assert call(P=0) == E_ARG
    assert call(D=1) == E_ARG       # odd D
    assert call(P=4096, D=2) == E_ARG
    for where in ("polys", "l", "r", "w"):  # a value >= r in every input array
        bad_p, bad_d = pa.copy(), [a.copy() for a in da]
        tgt = bad_p if where == "polys" else bad_d["lrw".index(where)]
        tgt[-1, -1] = fr_array([R])[0]
        assert call(pa=bad_p, da=bad_d) == E_ARG, where
    tr = FrTranscript()
    tr.t.squeezing = 2
    assert call(tr=tr) == E_ARG
    # the _dev entry: the same dimension checks, null device pointers
    d_p = _to_device(ctx, pa)
    assert lib.tpst_prodcircuit_prove_dev(ctx.h, ell, P, None, 0, None, None, None, C.byref(FrTranscript().t),
                                          ptr(proof), ptr(cp), None, ptr(rand)) == E_ARG
    assert lib.tpst_prodcircuit_prove_dev(ctx.h, ell, P, C.c_void_p(d_p.data_ptr()), 2, None, None, None,
                                          C.byref(FrTranscript().t), ptr(proof), ptr(cp), ptr(cd), ptr(rand)) == E_ARG
    assert lib.tpst_prodcircuit_prove_dev(ctx.h, 0, P, C.c_void_p(d_p.data_ptr()), 0, None, None, None,
                                          C.byref(FrTranscript().t), ptr(proof), ptr(cp), None, ptr(rand)) == E_ARG
    # the Python surface raises
    with pytest.raises(TpstError):
        PT.prove(ctx, pa[:, :6], None, FrTranscript())  # not a power of two
    with pytest.raises(TpstError):
        PT.prove(ctx, pa, tuple(a[:1] for a in da), FrTranscript())  # odd D
    # the context still works
    proof2, *_ = PT.prove(ctx, pa, da, FrTranscript())
    assert _ints(proof2.pack()) == T.flatten(_reference(ell, P, D)["proof"], ell, P, D)
