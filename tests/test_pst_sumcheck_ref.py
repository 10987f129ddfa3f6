"""CPU tests of the product sum-check's definition (tests/pst_sumcheck_ref.py)
and of the host-only verifier half tpst_pst_sumcheck_reduce:

* the restatement against brute force: e_0 is the plain sum over the cube,
  every round's s(0) + s(1) is e_i, the coefficients interpolate the round's
  evaluations, u_j = f_j(rho) by the oracle's Polynomial.eval, the final
  identity holds;
* tpst_pst_sumcheck_reduce through ctypes against the restatement's proofs: the
  same rho and the same transcript bytes at n = 4..7 on the five term shapes;
  TPST_E_VERIFY with the transcript untouched for every tamper; TPST_E_ARG for
  misuse.

Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_sumcheck_ref as SR
from testudo_amd.encoding import fr_array, gt_array, limbs_to_int, ptr

R = O.R
OK, E_ARG, E_VERIFY = 0, -1, -5
SHAPES = ["a", "b", "c", "c_bad", "d", "e"]

_GTS = []


def gts(B):
    """B of the five GT values of the n = 4 fixture, standing in for commitments"""
    if not _GTS:
        d = G.load("sqrt_pst_n4.json")
        towers = [G.gt(d["T"])] + [G.gt(t) for pair in d["comms_t"] for t in pair]
        _GTS.extend(O.fq12_from_tower(t) for t in towers)
    return _GTS[:B]


def gt_limbs(f):
    return gt_array(O.fq12_to_tower(f)).reshape(72)


def ref_start():
    """a transcript mid-protocol: something absorbed, one challenge squeezed"""
    tr = P.PoseidonTranscript()
    tr.append_gt(gts(5)[4])
    tr.challenge_scalar()
    return tr


def lib_start():
    from testudo_amd.sqrt_pst import PoseidonTranscript
    tr = PoseidonTranscript()
    tr.append_gt(gt_limbs(gts(5)[4]))
    tr.challenge_scalar()
    return tr


def sc_terms(terms):
    """[(coeff, [indices])] -> a tpst_sc_term array, unchecked (the tests hand over bad ones on purpose)"""
    from testudo_amd import _lib
    arr = (_lib.ScTerm * max(len(terms), 1))()
    for t, (c, idx) in enumerate(terms):
        arr[t].deg = len(idx) if not isinstance(idx, tuple) else idx[0]     # (deg, [indices]): a forced degree
        for k, j in enumerate(idx if not isinstance(idx, tuple) else idx[1]):
            arr[t].idx[k] = j
        for k in range(4):
            arr[t].coeff[k] = (c >> (64 * k)) & (2**64 - 1)
    return arr


def raw_reduce(tr, n, terms, tau, Ts, e0, rounds, u, B=None, M=None, null=None, pad=0):
    """tpst_pst_sumcheck_reduce on integers -> (rc, rho ints).  B / M override the counts handed over; null names
    one pointer argument to pass as NULL; pad: zero Fr appended to the rounds (a call that reads them as wider)."""
    from testudo_amd import _lib
    from testudo_amd.sqrt_pst import _ptr_array
    lib = _lib.load()
    arr = sc_terms(terms)
    tl = [gt_limbs(T) if not isinstance(T, np.ndarray) else T for T in Ts]
    ta = fr_array(tau) if tau is not None else None
    rd = fr_array([c for cs in rounds for c in cs] + [0] * pad)
    ua, ea = fr_array(u), fr_array([e0])
    rho = np.zeros((max(n, 1), 4), dtype=np.uint64)
    args = {"tr": C.addressof(tr.t), "Ts": _ptr_array(tl), "terms": C.addressof(arr), "e0": ptr(ea), "rounds": ptr(rd),
            "u": ptr(ua), "rho": ptr(rho)}
    if null is not None:
        args[null] = None
    rc = lib.tpst_pst_sumcheck_reduce(args["tr"], n, args["Ts"], len(tl) if B is None else B, args["terms"],
                                      len(terms) if M is None else M, None if ta is None else ptr(ta), args["e0"],
                                      args["rounds"], args["u"], args["rho"])
    return rc, [limbs_to_int(x) for x in rho]


# ------------------------------------------------------------ brute force ----
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_brute_force_n4(shape):
    n = 4
    Zs, terms, tau = SR.shape_case(shape, n)
    B, D = len(Zs), SR.degree(terms, tau)
    trace = []
    tr = ref_start()
    e0, rounds, u, rho = SR.prove(tr, n, Zs, terms, tau, gts(B), trace)
    assert e0 == SR.plain_sum(Zs, terms, tau)                  # the claim is the plain sum over the cube
    assert (e0 == 0) == (shape == "c")                         # the Hadamard relation holds only there
    assert len(rounds) == n and all(len(cs) == D + 1 for cs in rounds)
    e = e0
    for (ei, ev), cs, r in zip(trace, rounds, rho):
        assert ei == e and (ev[0] + ev[1]) % R == e            # s_i(0) + s_i(1) = e_i
        assert [SR.uni_eval(cs, t) for t in range(D + 1)] == list(ev)   # the coefficients interpolate s_i(0..D)
        e = SR.uni_eval(cs, r)
    for Z, uj in zip(Zs, u):
        assert P.Polynomial(Z).eval(rho) == uj                 # the oracle's own evaluation
    assert (1 if tau is None else SR.eq_at(tau, rho)) * SR.g_at(terms, u) % R == e     # the final identity
    assert SR.stages(n, Zs, terms, tau, rho) == ([ev for _, ev in trace], u)
    # the restated verifier agrees, with the prover's transcript
    tv = ref_start()
    assert SR.reduce(tv, n, B, terms, tau, gts(B), e0, rounds, u) == rho
    assert SR.transcript_bytes(tv) == SR.transcript_bytes(tr)
    # another claimed sum is not provable with these rounds
    assert SR.reduce(ref_start(), n, B, terms, tau, gts(B), (e0 + 1) % R, rounds, u) is None


def test_degree_one_runs_as_degree_two():
    """shape a: s_i is linear, sent as three coefficients with the last one zero"""
    Zs, terms, tau = SR.shape_case("a", 4)
    _, rounds, _, _ = SR.prove(ref_start(), 4, Zs, terms, tau, gts(1))
    assert all(len(cs) == 3 and cs[2] == 0 for cs in rounds)


# --------------------------------------------- tpst_pst_sumcheck_reduce -------
@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_sumcheck_reduce_matches_restatement(n, shape):
    Zs, terms, tau = SR.shape_case(shape, n)
    B = len(Zs)
    ref = ref_start()
    e0, rounds, u, rho = SR.prove(ref, n, Zs, terms, tau, gts(B))
    lib = lib_start()
    assert bytes(lib.t) == SR.transcript_bytes(ref_start())
    rc, got = raw_reduce(lib, n, terms, tau, gts(B), e0, rounds, u)
    assert rc == OK
    assert got == rho
    assert bytes(lib.t) == SR.transcript_bytes(ref)
    assert limbs_to_int(lib.challenge_scalar()) == ref.challenge_scalar()


def test_sumcheck_reduce_python_wrapper():
    from testudo_amd.sqrt_pst import sumcheck_reduce
    n = 5
    Zs, terms, tau = SR.shape_case("e", n)
    B = len(Zs)
    ref = ref_start()
    e0, rounds, u, rho = SR.prove(ref, n, Zs, terms, tau, gts(B))
    lt = [(fr_array([c])[0], idx) for c, idx in terms]
    tl = [gt_limbs(T) for T in gts(B)]
    rd = fr_array([c for cs in rounds for c in cs]).reshape(n, 4, 4)
    lib = lib_start()
    got = sumcheck_reduce(lib, n, lt, fr_array(tau), tl, fr_array([e0])[0], rd, fr_array(u))
    assert [limbs_to_int(x) for x in got] == rho and bytes(lib.t) == SR.transcript_bytes(ref)
    ub = fr_array(u)
    ub[1, 0] ^= np.uint64(1)
    lib = lib_start()
    assert sumcheck_reduce(lib, n, lt, fr_array(tau), tl, fr_array([e0])[0], rd, ub) is None
    assert bytes(lib.t) == SR.transcript_bytes(ref_start())


def _tamper_case(shape="e"):
    n = 5
    Zs, terms, tau = SR.shape_case(shape, n)
    e0, rounds, u, _ = SR.prove(ref_start(), n, Zs, terms, tau, gts(len(Zs)))
    return n, len(Zs), terms, tau, e0, rounds, u


def test_sumcheck_reduce_rejects_every_tamper():
    n, B, terms, tau, e0, rounds, u = _tamper_case()
    Ts = gts(B)
    start = bytes(lib_start().t)

    def rejected(terms=terms, tau=tau, Ts=Ts, e0=e0, rounds=rounds, u=u, **kw):
        tr = lib_start()
        rc, _ = raw_reduce(tr, n, terms, tau, Ts, e0, rounds, u, **kw)
        return rc == E_VERIFY and bytes(tr.t) == start

    tr = lib_start()
    assert raw_reduce(tr, n, terms, tau, Ts, e0, rounds, u)[0] == OK and bytes(tr.t) != start
    for i in (0, n // 2, n - 1):                       # first, a middle, the last round
        for c in range(4):                             # every coefficient of the cubic
            rd = [list(cs) for cs in rounds]
            rd[i][c] = (rd[i][c] + 1) % R
            assert rejected(rounds=rd), (i, c)
    for j in range(B):
        ub = list(u)
        ub[j] = (ub[j] + 1) % R
        assert rejected(u=ub), j
    assert rejected(e0=(e0 + 1) % R)
    for t in range(len(terms)):                        # a term's coefficient
        tb = list(terms)
        tb[t] = ((tb[t][0] + 1) % R, tb[t][1])
        assert rejected(terms=tb), t
    assert rejected(terms=[(terms[0][0], [1, 0])] + terms[1:])      # the same g with two indices swapped
    assert rejected(terms=[terms[0], (terms[1][0], [2, 3]), terms[2]])   # a changed index (every polynomial still used)
    assert rejected(terms=[terms[1], terms[0], terms[2]])           # two terms swapped
    tb = list(tau)
    tb[3] = (tb[3] + 1) % R
    assert rejected(tau=tb)                            # one coordinate
    assert rejected(Ts=[Ts[0], gts(5)[4], Ts[2], Ts[3]])   # a changed T_j
    assert rejected(tau=None)                          # has_tau flipped: the rounds then read as quadratics
    # a value >= r in each scalar field, a T coefficient >= p
    assert rejected(terms=[terms[0], (R, terms[1][1]), terms[2]])
    assert rejected(tau=[R + 1] + list(tau[1:]))
    assert rejected(e0=R)
    rd = [list(cs) for cs in rounds]
    rd[1][3] = R
    assert rejected(rounds=rd)
    assert rejected(u=[u[0], 2**256 - 1, u[2], u[3]])
    big = gt_limbs(Ts[1]).copy()
    big[5] = np.uint64(2**64 - 1)
    assert rejected(Ts=[Ts[0], big, Ts[2], Ts[3]])


def test_sumcheck_reduce_rejects_a_tau_added():
    """has_tau flipped the other way: a proof of sum f_0 f_1 presented under a tau (the rounds read as cubics)"""
    n, B, terms, tau, e0, rounds, u = _tamper_case("b")
    assert tau is None
    start = bytes(lib_start().t)
    tr = lib_start()
    assert raw_reduce(tr, n, terms, None, gts(B), e0, rounds, u)[0] == OK
    tr = lib_start()
    rc, _ = raw_reduce(tr, n, terms, [7] * n, gts(B), e0, rounds, u, pad=n)
    assert rc == E_VERIFY and bytes(tr.t) == start


def test_sumcheck_reduce_rejects_the_wrong_hadamard_claim():
    """shape c with one entry of f_2 wrong: the honest sum is not 0, and its proof does not pass for e_0 = 0"""
    n, B, terms, tau, e0, rounds, u = _tamper_case("c_bad")
    assert e0 != 0
    start = bytes(lib_start().t)
    tr = lib_start()
    assert raw_reduce(tr, n, terms, tau, gts(B), e0, rounds, u)[0] == OK
    tr = lib_start()
    assert raw_reduce(tr, n, terms, tau, gts(B), 0, rounds, u)[0] == E_VERIFY and bytes(tr.t) == start


def test_sumcheck_reduce_misuse():
    n, B, terms, tau, e0, rounds, u = _tamper_case()
    Ts = gts(B)
    start = bytes(lib_start().t)

    def misuse(**kw):
        tr = lib_start()
        args = dict(terms=terms, tau=tau, Ts=Ts, rounds=rounds, u=u)
        extra = {k: kw.pop(k) for k in ("B", "M", "null", "n") if k in kw}
        args.update(kw)
        rc, _ = raw_reduce(tr, extra.pop("n", n), args["terms"], args["tau"], args["Ts"], e0, args["rounds"],
                           args["u"], **extra)
        return rc == E_ARG and bytes(tr.t) == start

    for name in ("tr", "Ts", "terms", "e0", "rounds", "u", "rho"):
        assert misuse(null=name), name
    assert misuse(B=0) and misuse(M=0)
    assert misuse(Ts=[Ts[0]] * 257, u=[0] * 257)                                   # B > 256
    assert misuse(terms=[terms[k % 3] for k in range(65)])                         # M > 64
    assert misuse(terms=[terms[0], terms[1], (1, (0, [3]))])                       # a degree of 0
    assert misuse(terms=[terms[0], terms[1], (1, (4, [3, 3, 3]))])                 # a degree of 4
    assert misuse(terms=[(1, [0, 1, 2]), terms[2]])                                # D = 4: a cubic term under tau
    assert not misuse(terms=[(1, [0, 1, 2]), terms[2]], tau=None)                  # (without tau the shape is fine)
    assert misuse(terms=[terms[0], terms[1], (1, [B])])                            # an index >= B
    assert misuse(terms=terms[:2])                                                 # polynomial 3 in no term
    assert misuse(n=1) and misuse(n=-3) and misuse(n=41)                           # bad n
