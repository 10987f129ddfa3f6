"""The product sum-check (include/tpst.h: tpst_poly_sumcheck_open and its
parts) restated from first principles over oracle/py: the statement absorb and
the challenges over the oracle's sponge, the rounds with Python integers on
brute-force tables of 2^n entries (the whole eq table by its definition, no
half tables, no Montgomery form, nothing of the device's layout) and the final
identity; the hand-over to the combined opening is tests/pst_combine_ref.py's
combine_challenge.  What testudo_amd/csrc/poly_sumcheck.hip computes.
This protocol is the project's own; the reference has none.

Values are the oracle's: Fr as int, GT as the oracle's Fq12.  A term is
(coeff, [indices]); tau is a list of n Fr (MSB-first, pst.get_chi_i) or
None."""
import bls377 as O
import pst as P
from pst_combine_ref import append_fr
from pst_multi_ref import bind_top, eq_at, transcript_bytes, uni_eval  # noqa: F401  (re-exported to the tests)

R = O.R
INV2 = pow(2, -1, R)
INV6 = pow(6, -1, R)


def degree(terms, tau):
    """the round degree D: the largest term degree, one more under eq; D = 1 is run as D = 2"""
    return max(max(len(idx) for _, idx in terms) + (0 if tau is None else 1), 2)


def shape_case(shape, n, seed=0x5C00):
    """(Zs, terms, tau) of the issue's five term shapes on random tables:
    a      B = 1, g = f_0
    b      B = 2, g = f_0 f_1
    c      B = 3 with tau, g = f_0 f_1 - f_2 and f_2 = f_0 o f_1 (e_0 = 0); c_bad: one entry of f_2 changed
    d      B = 3, g = f_0 f_1 f_2
    e      B = 4 with tau, g = 3 f_0 f_1 + (r - 1) f_2 f_2 + f_3"""
    B = {"a": 1, "b": 2, "c": 3, "c_bad": 3, "d": 3, "e": 4}[shape]
    k, Zs = 0, []
    for _ in range(B):
        Z, k = P.fr_stream(seed + 64 * n + B, 1 << n, k)
        Zs.append(Z)
    tau, k = P.fr_stream(seed + 64 * n + B, n, k)
    if shape == "a":
        return Zs, [(1, [0])], None
    if shape == "b":
        return Zs, [(1, [0, 1])], None
    if shape in ("c", "c_bad"):
        Zs[2] = [x * y % R for x, y in zip(Zs[0], Zs[1])]
        if shape == "c_bad":
            Zs[2][(1 << n) - 3] = (Zs[2][(1 << n) - 3] + 1) % R
        return Zs, [(1, [0, 1]), (R - 1, [2])], tau
    if shape == "d":
        return Zs, [(1, [0, 1, 2])], None
    return Zs, [(3, [0, 1]), (R - 1, [2, 2]), (1, [3])], tau


def absorb_statement(tr, n, B, terms, tau, Ts, e0):
    """step 1: B, M, n, has_tau; every T_j; every term (degree, indices, coefficient); tau; e_0"""
    for x in (B, len(terms), n, 0 if tau is None else 1):
        append_fr(tr, x)
    for T in Ts:
        tr.append_gt(T)
    for c, idx in terms:
        append_fr(tr, len(idx))
        for j in idx:
            append_fr(tr, j)
        append_fr(tr, c)
    for x in tau or []:
        append_fr(tr, x)
    append_fr(tr, e0)


def eq_table(n, tau):
    """eq(tau, x) for every x by the definition, or all ones without tau"""
    return [1] * (1 << n) if tau is None else [P.get_chi_i(tau, x) for x in range(1 << n)]


def g_at(terms, vals):
    """sum_t c_t prod_i vals[idx_t[i]]"""
    total = 0
    for c, idx in terms:
        p = c
        for j in idx:
            p = p * vals[j] % R
        total += p
    return total % R


def plain_sum(Zs, terms, tau):
    """e_0 by the definition: sum_x eq(tau, x) g(x)"""
    n = len(Zs[0]).bit_length() - 1
    E = eq_table(n, tau)
    return sum(E[x] * g_at(terms, [Z[x] for Z in Zs]) for x in range(1 << n)) % R


def round_sums(E, F, terms, D):
    """s(0..D) of the round over the top variable: every table is lo + t (hi - lo) in it"""
    h = len(E) // 2
    out = []
    for t in range(D + 1):
        at = lambda tab, i: (tab[i] + t * (tab[i + h] - tab[i])) % R  # noqa: E731
        out.append(sum(at(E, i) * g_at(terms, [at(f, i) for f in F]) for i in range(h)) % R)
    return tuple(out)


def from_evals(ev):
    """UniPoly::from_evals (unipoly.rs:15-45): the coefficients, constant first, of the polynomial of degree
    len(ev) - 1 through (t, ev[t]), by finite differences"""
    if len(ev) == 3:
        a = 0
    else:
        a = INV6 * (ev[3] - 3 * ev[2] + 3 * ev[1] - ev[0]) % R           # third difference = 6 a
    b = INV2 * (ev[2] - 2 * ev[1] + ev[0] - 6 * a) % R                   # second difference at 0 = 2 b + 6 a
    lin = (ev[1] - ev[0] - a - b) % R
    return (ev[0] % R, lin, b) if len(ev) == 3 else (ev[0] % R, lin, b, a)


def stages(n, Zs, terms, tau, rho):
    """the rounds under given challenges: ([s_i(0..D)], [u_j]) -- what tpst_poly_sumcheck_stages returns"""
    D = degree(terms, tau)
    E, F = eq_table(n, tau), [list(Z) for Z in Zs]
    sums = []
    for i in range(n):
        sums.append(round_sums(E, F, terms, D))
        E, F = bind_top(E, rho[i]), [bind_top(t, rho[i]) for t in F]
    return sums, [f[0] for f in F]


def prove(tr, n, Zs, terms, tau, Ts, trace=None):
    """steps 1-3 of the prover: (e0, rounds [coefficients], u, rho).  trace (a list): per round (e_i, s_i(0..D))."""
    D = degree(terms, tau)
    E, F = eq_table(n, tau), [list(Z) for Z in Zs]
    rounds, rho = [], []
    e0 = e = None
    for i in range(n):
        ev = round_sums(E, F, terms, D)
        if i == 0:
            e0 = e = (ev[0] + ev[1]) % R
            absorb_statement(tr, n, len(Zs), terms, tau, Ts, e0)
        if trace is not None:
            trace.append((e, ev))
        cs = from_evals(ev)
        for c in cs:
            append_fr(tr, c)
        r = tr.challenge_scalar()
        e = uni_eval(cs, r)
        E, F = bind_top(E, r), [bind_top(t, r) for t in F]
        rounds.append(cs)
        rho.append(r)
    return e0, rounds, [f[0] for f in F], rho


def reduce(tr, n, B, terms, tau, Ts, e0, rounds, u):
    """steps 1-3 of the verifier: rho, or None when a round check or the final identity fails.  tr is advanced
    either way (work on a copy to keep the caller's)."""
    absorb_statement(tr, n, B, terms, tau, Ts, e0)
    e, rho = e0, []
    for cs in rounds:
        if (cs[0] + sum(cs)) % R != e:  # s_i(0) + s_i(1)
            return None
        for c in cs:
            append_fr(tr, c)
        r = tr.challenge_scalar()
        e = uni_eval(cs, r)
        rho.append(r)
    if (1 if tau is None else eq_at(tau, rho)) * g_at(terms, u) % R != e:
        return None
    return rho
