"""The lookup argument (include/tpst.h: tpst_poly_lookup_open and its parts)
restated from first principles over oracle/py: multiplicities with a dict,
inverses with pow(x, -1, r), the transcript steps over the oracle's sponge, and
the two sub-protocols composed from their own restatements
(tests/pst_sumcheck_ref.py, tests/pst_multi_ref.py).  What
testudo_amd/csrc/lookup.hip computes.  This protocol is the project's own; the
reference has none.

Values are the oracle's: Fr as int, GT as the oracle's Fq12.  As is the list
of the L witness tables, t the table; the polynomial order everywhere is
a_0..a_{L-1}, t, m, h_0..h_{L-1}, h_t."""
import bls377 as O
import pst as P
import pst_multi_ref as MR
import pst_sumcheck_ref as SR
from pst_combine_ref import append_fr, combine_challenge, combine_T, combine_tables, combine_v
from pst_multi_ref import transcript_bytes  # noqa: F401  (re-exported to the tests)

R = O.R
HALF = (R + 1) // 2


class NotInTable(Exception):
    """a witness entry that no table entry holds: args = (l, x), the least such pair"""


def multiplicities(As, t):
    """m[y] = #{(l, x) : a_l[x] = t[y]} at the first y holding the value, 0 at its repeats"""
    first = {}
    for y, v in enumerate(t):
        first.setdefault(v, y)
    m = [0] * len(t)
    for l, a in enumerate(As):
        for x, v in enumerate(a):
            if v not in first:
                raise NotInTable(l, x)
            m[first[v]] += 1
    return m


def inverses(f, beta, num=None):
    """num[i] / (beta + f[i])"""
    return [(1 if num is None else num[i]) * pow((beta + v) % R, -1, R) % R for i, v in enumerate(f)]


def helpers(As, t, beta, m=None):
    """(m, [h_0..h_{L-1}, h_t]); a given m is taken as it is"""
    m = multiplicities(As, t) if m is None else m
    return m, [inverses(a, beta) for a in As] + [inverses(t, beta, m)]


def half_value(h):
    """h(1/2, .., 1/2) = 2^-n sum_x h(x) for the multilinear h with these evaluations"""
    return sum(h) * pow(HALF, len(h).bit_length() - 1, R) % R


def lookup_terms(L, beta, lam):
    """step 4's terms and the claim e_0 = sum_{l < L} lambda^l"""
    terms = []
    for l in range(L + 1):
        h, f = L + 2 + l, l                       # l == L: h_t and t
        terms += [(pow(lam, l, R), [h, f]), (pow(lam, l, R) * beta % R, [h])]
    terms.append(((-pow(lam, L, R)) % R, [L + 1]))
    return terms, sum(pow(lam, l, R) for l in range(L)) % R


def lookup_claims(L, n, rho, u, s):
    """step 6's claims: every polynomial at rho, then every h at the 1/2 point"""
    B = 2 * L + 3
    return [(j, list(rho), u[j]) for j in range(B)] + [(L + 2 + k, [HALF] * n, s[k]) for k in range(L + 1)]


def step1(tr, L, n, Ts):
    append_fr(tr, L)
    append_fr(tr, n)
    for T in Ts:
        tr.append_gt(T)


def step2(tr, T_m):
    tr.append_gt(T_m)
    return tr.challenge_scalar()


def step3(tr, n, T_h):
    for T in T_h:
        tr.append_gt(T)
    tau = [tr.challenge_scalar() for _ in range(n)]
    return tau, tr.challenge_scalar()


def prove_reduction(tr, As, t, Ts, commit_T, beta_early=False):
    """Steps 1-5 and the multi-point reduction of the prover.  commit_T(table) -> the GT commitment of a helper
    table (the tests hand over the oracle's commit, or stand-ins where no pairing is wanted).  Returns (proof,
    tables, rho') with proof = dict(T_m, T_h, rounds, u, s, mp_rounds, mp_u) and tables = all B tables in order.
    beta_early: the UNSOUND ordering, beta drawn before T_m is absorbed (the verifier must reject its proofs)."""
    L, n = len(As), len(t).bit_length() - 1
    step1(tr, L, n, Ts)
    m = multiplicities(As, t)
    T_m = commit_T(m)
    if beta_early:
        beta = tr.challenge_scalar()
        tr.append_gt(T_m)
    else:
        beta = step2(tr, T_m)
    _, hs = helpers(As, t, beta, m)
    T_h = [commit_T(h) for h in hs]
    tau, lam = step3(tr, n, T_h)
    tables = [list(a) for a in As] + [list(t), m] + hs
    Tall = list(Ts) + [T_m] + T_h
    terms, claim = lookup_terms(L, beta, lam)
    e0, rounds, u, rho = SR.prove(tr, n, tables, terms, tau, Tall)
    assert e0 == claim                                  # the honest sum is the claim the verifier computes
    s = [half_value(h) for h in hs]
    mp_rounds, mp_u, rho2 = MR.prove_reduction(tr, n, tables, lookup_claims(L, n, rho, u, s), Tall)
    proof = dict(T_m=T_m, T_h=T_h, rounds=rounds, u=u, s=s, mp_rounds=mp_rounds, mp_u=mp_u)
    return proof, tables, rho2


def reduce(tr, n, Ts, proof):
    """The verifier's steps 1-5 and the multi-point reduction: rho', or None when a check fails.  tr is advanced
    either way (work on a copy to keep the caller's)."""
    L = len(Ts) - 1
    B = 2 * L + 3
    step1(tr, L, n, Ts)
    beta = step2(tr, proof["T_m"])
    tau, lam = step3(tr, n, proof["T_h"])
    Tall = list(Ts) + [proof["T_m"]] + list(proof["T_h"])
    terms, claim = lookup_terms(L, beta, lam)
    rho = SR.reduce(tr, n, B, terms, tau, Tall, claim, proof["rounds"], proof["u"])
    if rho is None:
        return None
    s = proof["s"]
    if sum(s[:L]) % R != s[L]:
        return None
    return MR.verify_reduction(tr, n, B, lookup_claims(L, n, rho, proof["u"], s), Tall, proof["mp_rounds"],
                               proof["mp_u"])


def prove(srs, tr, As, t, commitments):
    """the whole prover on the oracle: (proof with "open" = (U, pst_proof, mipp), rho', (comm_list*, T*, v*))"""
    helper_comms = []

    def commit_T(table):
        comms, T = P.Polynomial(table).commit(srs)
        helper_comms.append((comms, T))
        return T

    Ts = [T for _, T in commitments]
    proof, tables, rho2 = prove_reduction(tr, As, t, Ts, commit_T)
    Tall = Ts + [proof["T_m"]] + proof["T_h"]
    w = combine_challenge(tr, rho2, Tall, proof["mp_u"])
    pl = P.Polynomial(combine_tables(tables, w))
    comms, T = pl.commit(srs)
    v = pl.eval(rho2)
    proof["open"] = pl.open(tr, comms, srs, rho2, T)
    return proof, rho2, (comms, T, v)


def verify(srs, tr, n, Ts, proof):
    """the whole verifier on the oracle"""
    rho2 = reduce(tr, n, Ts, proof)
    if rho2 is None:
        return False
    Tall = list(Ts) + [proof["T_m"]] + list(proof["T_h"])
    w = combine_challenge(tr, rho2, Tall, proof["mp_u"])
    U, pst_proof, mipp = proof["open"]
    return P.Polynomial.verify(tr, srs, U, rho2, combine_v(proof["mp_u"], w), pst_proof, mipp, combine_T(Tall, w))
