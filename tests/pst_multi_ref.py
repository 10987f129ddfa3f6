"""The multi-point opening (include/tpst.h: tpst_poly_open_multi and its
parts) restated from first principles over oracle/py: the statement absorb and
the challenges over the oracle's sponge, the sum-check with Python integers on
brute-force tables of 2^n entries (no half tables, no Montgomery form, nothing
of the device's layout), the final identity, and the hand-over to the combined
opening of tests/pst_combine_ref.py.  What testudo_amd/csrc/poly_multi.hip
computes.  This protocol is the project's own; the reference has none.

Values are the oracle's: Fr as int, GT as the oracle's Fq12.  A claim is
(poly_index, point, value) with the point MSB-first (pst.get_chi_i)."""
import bls377 as O
import pst as P
from pst_combine_ref import append_fr, combine_challenge, combine_T, combine_tables, combine_v

R = O.R
INV2 = pow(2, -1, R)


def transcript_bytes(tr):
    """the oracle transcript as the bytes of a tpst_transcript: 3 x 6 u64 limbs, squeezing, index"""
    mode, idx = tr.sponge.mode
    out = b"".join(int(s).to_bytes(48, "little") for s in tr.sponge.state)
    return out + (1 if mode == "squeeze" else 0).to_bytes(4, "little") + int(idx).to_bytes(4, "little")


def absorb_statement(tr, n, B, claims, Ts):
    """step 1: B, K, n; every T_j; every claim (index, coordinates, value); gamma -> a_k = gamma^k"""
    append_fr(tr, B)
    append_fr(tr, len(claims))
    append_fr(tr, n)
    for T in Ts:
        tr.append_gt(T)
    for j, point, v in claims:
        append_fr(tr, j)
        for x in point:
            append_fr(tr, x)
        append_fr(tr, v)
    gamma = tr.challenge_scalar()
    return [pow(gamma, k, R) for k in range(len(claims))]


def eq_tables(n, B, claims, a):
    """D_j[x] = sum_{k: j_k = j} a_k eq(r_k, x), the whole 2^n table by the definition"""
    D = [[0] * (1 << n) for _ in range(B)]
    for (j, point, _), ak in zip(claims, a):
        for x in range(1 << n):
            D[j][x] = (D[j][x] + ak * P.get_chi_i(point, x)) % R
    return D


def from_evals3(e0, e1, e2):
    """UniPoly::from_evals (unipoly.rs:15-45) for three evaluations at 0, 1, 2: (c0, c1, c2)"""
    c = e0 % R
    a = INV2 * (e2 - e1 - e1 + c) % R
    return c, (e1 - c - a) % R, a


def uni_eval(cs, x):
    return sum(c * pow(x, i, R) for i, c in enumerate(cs)) % R


def bind_top(tab, rho):
    """bound_poly_var_top: the most significant variable set to rho"""
    h = len(tab) // 2
    return [(tab[i] + rho * (tab[i + h] - tab[i])) % R for i in range(h)]


def round_sums(D, F):
    """s(0) and s(2) of the round over the top variable of sum_j D_j F_j"""
    h = len(F[0]) // 2
    s0 = sum(d[i] * f[i] for d, f in zip(D, F) for i in range(h)) % R
    s2 = sum((2 * d[i + h] - d[i]) * (2 * f[i + h] - f[i]) for d, f in zip(D, F) for i in range(h)) % R
    return s0, s2


def full_sum(D, F):
    return sum(x * y for d, f in zip(D, F) for x, y in zip(d, f)) % R


def stages(n, Zs, claims, a, rho):
    """the reduction under given weights and challenges: ([(s_i(0), s_i(2))], [u_j]) -- what
    tpst_poly_multi_sumcheck_stages returns"""
    D, F = eq_tables(n, len(Zs), claims, a), [list(Z) for Z in Zs]
    sums = []
    for i in range(n):
        sums.append(round_sums(D, F))
        D, F = [bind_top(t, rho[i]) for t in D], [bind_top(t, rho[i]) for t in F]
    return sums, [f[0] for f in F]


def eq_at(point, rho):
    out = 1
    for x, y in zip(point, rho):
        out = out * (x * y + (1 - x) * (1 - y)) % R
    return out


def prove_reduction(tr, n, Zs, claims, Ts, trace=None):
    """steps 1-3 of the prover: (rounds [(c0, c1, c2)], u, rho).  trace (a list): per round (e_i, the full
    sum of the tables before the round, s_i(0), s_i(1), s_i(2))."""
    a = absorb_statement(tr, n, len(Zs), claims, Ts)
    e = sum(ak * v for ak, (_, _, v) in zip(a, claims)) % R
    D, F = eq_tables(n, len(Zs), claims, a), [list(Z) for Z in Zs]
    rounds, rho = [], []
    for _ in range(n):
        s0, s2 = round_sums(D, F)
        s1 = (e - s0) % R
        if trace is not None:
            trace.append((e, full_sum(D, F), s0, s1, s2))
        cs = from_evals3(s0, s1, s2)
        for c in cs:
            append_fr(tr, c)
        r = tr.challenge_scalar()
        e = uni_eval(cs, r)
        D, F = [bind_top(t, r) for t in D], [bind_top(t, r) for t in F]
        rounds.append(cs)
        rho.append(r)
    return rounds, [f[0] for f in F], rho


def verify_reduction(tr, n, B, claims, Ts, rounds, u):
    """steps 1-3 of the verifier: rho, or None when a round check or the final identity fails.  tr is advanced
    either way (work on a copy to keep the caller's)."""
    a = absorb_statement(tr, n, B, claims, Ts)
    e = sum(ak * v for ak, (_, _, v) in zip(a, claims)) % R
    rho = []
    for cs in rounds:
        if (2 * cs[0] + cs[1] + cs[2]) % R != e:  # s_i(0) + s_i(1)
            return None
        for c in cs:
            append_fr(tr, c)
        r = tr.challenge_scalar()
        e = uni_eval(cs, r)
        rho.append(r)
    Drho = [0] * B
    for (j, point, _), ak in zip(claims, a):
        Drho[j] = (Drho[j] + ak * eq_at(point, rho)) % R
    if sum(x * y for x, y in zip(u, Drho)) % R != e:
        return None
    return rho


def prove(srs, tr, Zs, commitments, claims):
    """the whole prover on the oracle: (rounds, u, (U, pst_proof, mipp)), rho, (comm_list*, T*, v*)"""
    n = len(Zs[0]).bit_length() - 1
    Ts = [T for _, T in commitments]
    rounds, u, rho = prove_reduction(tr, n, Zs, claims, Ts)
    w = combine_challenge(tr, rho, Ts, u)
    pl = P.Polynomial(combine_tables(Zs, w))
    comms, T = pl.commit(srs)
    v = pl.eval(rho)
    return (rounds, u, pl.open(tr, comms, srs, rho, T)), rho, (comms, T, v)


def verify(srs, tr, n, claims, Ts, proof):
    """the whole verifier on the oracle"""
    rounds, u, (U, pst_proof, mipp) = proof
    rho = verify_reduction(tr, n, len(Ts), claims, Ts, rounds, u)
    if rho is None:
        return False
    w = combine_challenge(tr, rho, Ts, u)
    return P.Polynomial.verify(tr, srs, U, rho, combine_v(u, w), pst_proof, mipp, combine_T(Ts, w))
