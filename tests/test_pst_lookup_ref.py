"""CPU tests of the lookup argument's definition (tests/pst_lookup_ref.py) and
of the host-only verifier half tpst_pst_lookup_reduce:

* the restatement against its definition at n = 4: the multiplicities sum to
  L 2^n and are 0 at repeats, every h times its denominator is 1 (or m), the
  values at the 1/2 point are the oracle's Polynomial.eval and satisfy
  sum_l s_l = s_t -- and fail it for a non-member with m left as it is; one run
  end to end through the oracle's pairing;
* tpst_pst_lookup_reduce through ctypes against the restatement's proofs: the
  same rho' and the same transcript bytes at n = 4..7 x L = 1, 2, 3;
  TPST_E_VERIFY with the transcript untouched for every tamper; TPST_E_ARG for
  misuse.

Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import bls377 as O
import golden_io as G
import pst as P
import pst_lookup_ref as LR
from testudo_amd.encoding import fr_array, gt_array, limbs_to_int, ptr

R = O.R
OK, E_ARG, E_VERIFY = 0, -1, -5

_GTS = []


def gts(k):
    """k distinct GT values standing in for commitments: the five of the n = 4 fixture, then their products"""
    if not _GTS:
        d = G.load("sqrt_pst_n4.json")
        towers = [G.gt(d["T"])] + [G.gt(t) for pair in d["comms_t"] for t in pair]
        _GTS.extend(O.fq12_from_tower(t) for t in towers)
    while len(_GTS) < k:
        _GTS.append(O.f12_mul(_GTS[-1], _GTS[len(_GTS) - 4]))
    return _GTS[:k]


def gt_limbs(f):
    return gt_array(O.fq12_to_tower(f)).reshape(72)


class StandIns:
    """commit_T of the restatement without a pairing: the next of a fixed run of GT values per helper table"""

    def __init__(self, skip):
        self.k = skip

    def __call__(self, table):
        self.k += 1
        return gts(self.k)[-1]


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


def make_case(n, L, kind="range", seed=0x10C0):
    """(As, t): `range`: t(y) = y and uniform witnesses; `repeats`: 2^n / 4 random values, each 4 times in a
    shuffled table, and witnesses drawn from them"""
    rng = random.Random(seed + 16 * n + L)
    N = 1 << n
    if kind == "range":
        t = list(range(N))
    else:
        vals = [rng.randrange(R) for _ in range(N // 4)]
        t = vals * 4
        rng.shuffle(t)
    return [[t[rng.randrange(N)] for _ in range(N)] for _ in range(L)], t


def proof_case(n, L, kind="range", **kw):
    """the restatement's proof on stand-in commitments: (Ts, proof, rho', the prover's end transcript)"""
    As, t = make_case(n, L, kind)
    Ts = gts(L + 1)
    ref = ref_start()
    proof, _, rho2 = LR.prove_reduction(ref, As, t, Ts, StandIns(L + 1), **kw)
    return Ts, proof, rho2, ref


def raw_reduce(tr, n, Ts, proof, L=None, null=None):
    """tpst_pst_lookup_reduce on the restatement's values -> (rc, rho' ints).  L overrides the count handed over;
    null names one pointer argument to pass as NULL."""
    from testudo_amd import _lib
    from testudo_amd.sqrt_pst import _ptr_array
    lib = _lib.load()
    tl = [gt_limbs(T) if not isinstance(T, np.ndarray) else T for T in Ts]
    th = np.stack([gt_limbs(T) if not isinstance(T, np.ndarray) else T for T in [proof["T_m"]] + list(proof["T_h"])])
    arrs = {"Ts": _ptr_array(tl), "T_helpers": ptr(np.ascontiguousarray(th)),
            "rounds": ptr(fr_array([c for cs in proof["rounds"] for c in cs])), "u": ptr(fr_array(proof["u"])),
            "s": ptr(fr_array(proof["s"])), "mp_rounds": ptr(fr_array([c for cs in proof["mp_rounds"] for c in cs])),
            "mp_u": ptr(fr_array(proof["mp_u"]))}
    rho = np.zeros((max(n, 1), 4), dtype=np.uint64)
    arrs["rho"] = ptr(rho)
    arrs["tr"] = C.addressof(tr.t)
    if null is not None:
        arrs[null] = None
    rc = lib.tpst_pst_lookup_reduce(arrs["tr"], n, len(tl) - 1 if L is None else L, arrs["Ts"], arrs["T_helpers"],
                                    arrs["rounds"], arrs["u"], arrs["s"], arrs["mp_rounds"], arrs["mp_u"], arrs["rho"])
    return rc, [limbs_to_int(x) for x in rho]


# ------------------------------------------------------------ the definition ---
@pytest.mark.parametrize("kind", ["range", "repeats"])
@pytest.mark.parametrize("L", [1, 2])
def test_helpers_against_their_definition_n4(L, kind):
    n = 4
    N = 1 << n
    As, t = make_case(n, L, kind)
    beta = random.Random(0x10C1).randrange(R)
    m, hs = LR.helpers(As, t, beta)
    assert sum(m) == L * N
    for y, v in enumerate(t):
        if t.index(v) != y:
            assert m[y] == 0                                  # a repeat carries nothing
        else:
            assert m[y] == sum(a.count(v) for a in As)        # the first occurrence carries every hit
    if kind == "repeats":
        assert sum(1 for y, v in enumerate(t) if t.index(v) != y) == 3 * N // 4
    for a, h in zip(As, hs):
        assert all(x * (beta + v) % R == 1 for x, v in zip(h, a))
    assert all(x * (beta + v) % R == c for x, v, c in zip(hs[L], t, m))
    s = [LR.half_value(h) for h in hs]
    for h, sv in zip(hs, s):
        assert P.Polynomial(h).eval([LR.HALF] * n) == sv      # the oracle's own evaluation at the 1/2 point
    assert sum(s[:L]) % R == s[L]                             # the LogUp identity, honest prover
    # one witness entry replaced by a non-member, m left as it is: the identity fails
    bad = [list(a) for a in As]
    bad[L - 1][5] = max(t) + 1 if kind == "range" else (t[0] + 1) % R
    assert bad[L - 1][5] not in t
    _, hb = LR.helpers(bad, t, beta, m)
    sb = [LR.half_value(h) for h in hb]
    assert sum(sb[:L]) % R != sb[L]
    with pytest.raises(LR.NotInTable) as e:
        LR.multiplicities(bad, t)
    assert e.value.args == (L - 1, 5)


def test_the_terms_sum_to_the_claim():
    """sum_x eq(tau, x) g(x) over the honest tables is sum_l lambda^l, for any tau"""
    import pst_sumcheck_ref as SR
    n, L = 4, 2
    rng = random.Random(0x10C2)
    As, t = make_case(n, L, "repeats")
    beta, lam = rng.randrange(R), rng.randrange(R)
    m, hs = LR.helpers(As, t, beta)
    terms, claim = LR.lookup_terms(L, beta, lam)
    assert len(terms) == 2 * L + 3 and claim == (1 + lam) % R
    tau = [rng.randrange(R) for _ in range(n)]
    assert SR.plain_sum(As + [t, m] + hs, terms, tau) == claim


def test_whole_protocol_on_the_oracle_n4_l1():
    """prover and verifier restated end to end over the oracle's commitments and pairing (one size: slow)"""
    n, L = 4, 1
    srs = P.SRS(2)
    As, t = make_case(n, L)
    commitments = [P.Polynomial(Z).commit(srs) for Z in As + [t]]
    Ts = [T for _, T in commitments]
    tp = P.PoseidonTranscript()
    proof, _, _ = LR.prove(srs, tp, As, t, commitments)
    tv = P.PoseidonTranscript()
    assert LR.verify(srs, tv, n, Ts, proof)
    assert LR.transcript_bytes(tv) == LR.transcript_bytes(tp)
    bad = dict(proof, s=[(proof["s"][0] + 1) % R, (proof["s"][1] + 1) % R])   # still sum_l s_l = s_t, but wrong
    assert not LR.verify(srs, P.PoseidonTranscript(), n, Ts, bad)


# ---------------------------------------------- tpst_pst_lookup_reduce --------
@pytest.mark.parametrize("n", [4, 5, 6, 7])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_lookup_reduce_matches_restatement(n, L):
    Ts, proof, rho2, ref = proof_case(n, L, "range" if (n + L) % 2 else "repeats")
    lib = lib_start()
    assert bytes(lib.t) == LR.transcript_bytes(ref_start())
    rc, got = raw_reduce(lib, n, Ts, proof)
    assert rc == OK
    assert got == rho2
    assert bytes(lib.t) == LR.transcript_bytes(ref)
    # the restated verifier agrees
    tv = ref_start()
    assert LR.reduce(tv, n, Ts, proof) == rho2 and LR.transcript_bytes(tv) == LR.transcript_bytes(ref)
    assert limbs_to_int(lib.challenge_scalar()) == ref.challenge_scalar()


def test_lookup_reduce_python_wrapper():
    from testudo_amd.sqrt_pst import LookupProof, lookup_reduce
    n, L = 5, 2
    Ts, proof, rho2, ref = proof_case(n, L)
    lp = LookupProof(gt_limbs(proof["T_m"]), np.stack([gt_limbs(T) for T in proof["T_h"]]),
                     fr_array([c for cs in proof["rounds"] for c in cs]).reshape(n, 4, 4), fr_array(proof["u"]),
                     fr_array(proof["s"]), fr_array([c for cs in proof["mp_rounds"] for c in cs]).reshape(n, 3, 4),
                     fr_array(proof["mp_u"]), None, None, None)
    tl = [gt_limbs(T) for T in Ts]
    lib = lib_start()
    got = lookup_reduce(lib, n, tl, lp)
    assert [limbs_to_int(x) for x in got] == rho2 and bytes(lib.t) == LR.transcript_bytes(ref)
    lp.s = lp.s.copy()
    lp.s[0, 0] ^= np.uint64(1)
    lib = lib_start()
    assert lookup_reduce(lib, n, tl, lp) is None and bytes(lib.t) == LR.transcript_bytes(ref_start())


def test_lookup_reduce_rejects_every_tamper():
    n, L = 5, 2
    B = 2 * L + 3
    Ts, proof, _, _ = proof_case(n, L)
    start = bytes(lib_start().t)

    def rejected(Ts=Ts, **kw):
        tr = lib_start()
        rc, _ = raw_reduce(tr, n, Ts, dict(proof, **kw))
        return rc == E_VERIFY and bytes(tr.t) == start

    def bumped(key, *index):
        """the proof's list `key` with the entry at index (one or two levels) incremented mod r"""
        out = [list(x) if isinstance(x, (list, tuple)) else x for x in proof[key]]
        if len(index) == 1:
            out[index[0]] = (out[index[0]] + 1) % R
        else:
            out[index[0]][index[1]] = (out[index[0]][index[1]] + 1) % R
        return {key: out}

    def put(key, value, *index):
        out = [list(x) if isinstance(x, (list, tuple)) else x for x in proof[key]]
        if len(index) == 1:
            out[index[0]] = value
        else:
            out[index[0]][index[1]] = value
        return {key: out}

    tr = lib_start()
    assert raw_reduce(tr, n, Ts, proof)[0] == OK and bytes(tr.t) != start
    other = gts(12)[11]
    assert rejected(T_m=other)                                          # T_m
    for k in range(L + 1):                                              # a T_h
        th = list(proof["T_h"])
        th[k] = other
        assert rejected(T_h=th), k
    assert rejected(T_h=[proof["T_h"][1], proof["T_h"][0], proof["T_h"][2]])        # swapped h_0 / h_1
    assert rejected(Ts=[Ts[1], Ts[0], Ts[2]])                           # the statement's commitments swapped
    for k in range(L + 1):                                              # each s, s_t the last
        assert rejected(**bumped("s", k)), k
    # s_0 and s_t both moved: sum_l s_l = s_t still holds, the multi-point reduction does not
    assert rejected(s=[(proof["s"][0] + 1) % R, proof["s"][1], (proof["s"][2] + 1) % R])
    for i in (0, n // 2, n - 1):                                        # three rounds of each reduction
        for c in range(4):
            assert rejected(**bumped("rounds", i, c)), (i, c)
        for c in range(3):
            assert rejected(**bumped("mp_rounds", i, c)), (i, c)
    for j in range(B):                                                  # each u, each multi-point final value
        assert rejected(**bumped("u", j)), j
        assert rejected(**bumped("mp_u", j)), j
    # a value >= r in every scalar field, a T coefficient >= p
    assert rejected(**put("rounds", R, 1, 3))
    assert rejected(**put("mp_rounds", R + 1, 2, 0))
    assert rejected(**put("u", R, 0))
    assert rejected(**put("mp_u", 2**256 - 1, B - 1))
    assert rejected(**put("s", R, L))
    assert rejected(**put("s", R + 7, 0))
    big = gt_limbs(proof["T_m"]).copy()
    big[5] = np.uint64(2**64 - 1)
    assert rejected(T_m=big)
    big = gt_limbs(Ts[0]).copy()
    big[71] = np.uint64(2**64 - 1)
    assert rejected(Ts=[big, Ts[1], Ts[2]])


def test_lookup_reduce_rejects_a_beta_drawn_before_t_m():
    """the unsound ordering: a prover that squeezes beta first and absorbs T_m afterwards produces a proof that is
    complete under its own ordering (the restated sum-check accepts its own e_0) and that the library rejects"""
    n, L = 5, 2
    Ts, proof, _, _ = proof_case(n, L, beta_early=True)
    start = bytes(lib_start().t)
    tr = lib_start()
    rc, _ = raw_reduce(tr, n, Ts, proof)
    assert rc == E_VERIFY and bytes(tr.t) == start
    assert LR.reduce(ref_start(), n, Ts, proof) is None


def test_lookup_reduce_misuse():
    n, L = 5, 2
    Ts, proof, _, _ = proof_case(n, L)
    start = bytes(lib_start().t)

    def misuse(n=n, Ts=Ts, **kw):
        tr = lib_start()
        rc, _ = raw_reduce(tr, n, Ts, proof, **kw)
        return rc == E_ARG and bytes(tr.t) == start

    for name in ("tr", "Ts", "T_helpers", "rounds", "u", "s", "mp_rounds", "mp_u", "rho"):
        assert misuse(null=name), name
    assert misuse(L=0) and misuse(L=9, Ts=list(Ts) * 4)
    assert misuse(n=1) and misuse(n=-3) and misuse(n=41)
    assert misuse(n=30)                                                 # n + 3 > 32
