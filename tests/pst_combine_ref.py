"""The combined opening (include/tpst.h: tpst_poly_open_combined and its
parts) restated over oracle/py: the Fiat-Shamir derivation of the weights over
the oracle's sponge, and the linear combination of tables, row commitments, T
and v with Python integers.  What testudo_amd/csrc/poly_lincomb.hip computes.

Values are the oracle's: Fr as int, G1 as (x, y) or None, GT as the oracle's
Fq12."""
import bls377 as O
import pst as P

R = O.R


def append_fr(tr, x):
    """tpst_transcript_append_fr (poseidon_transcript.rs:83-85): an Fr absorbed as ONE Fq element of the
    same integer value.  oracle/py/pst.py's transcript has no such call: restated here over its sponge."""
    assert 0 <= x < R
    tr.sponge.absorb_elems([x])


def combine_challenge(tr, point, Ts, vs):
    """tpst_pst_combine_challenge: append_gt of every T_j, append_fr of the point and of every v_j, one
    challenge rho; w_j = rho^j."""
    for T in Ts:
        tr.append_gt(T)
    for x in point:
        append_fr(tr, x)
    for v in vs:
        append_fr(tr, v)
    rho = tr.challenge_scalar()
    return [pow(rho, j, R) for j in range(len(Ts))]


def combine_tables(Zs, w):
    """Z*[i] = sum_j w_j Z_j[i] mod r"""
    return [sum(wj * Z[i] for wj, Z in zip(w, Zs)) % R for i in range(len(Zs[0]))]


def combine_rows(lists, w):
    """out[i] = sum_j w_j lists[j][i] (G1, None = infinity)"""
    out = []
    for i in range(len(lists[0])):
        acc = None
        for wj, L in zip(w, lists):
            acc = O.g1_add(acc, O.g1_mul(L[i], wj))
        out.append(acc)
    return out


def combine_T(Ts, w):
    """T* = prod_j T_j^(w_j)"""
    acc = O.f12_one()
    for wj, T in zip(w, Ts):
        acc = O.f12_mul(acc, O.f12_pow(T, wj))
    return acc


def combine_v(vs, w):
    return sum(wj * v for wj, v in zip(w, vs)) % R


def parent_path(srs, Zs, w, point):
    """The definition of every combined value: commit / eval / open of Z* itself on a fresh transcript."""
    pl = P.Polynomial(combine_tables(Zs, w))
    comms, T = pl.commit(srs)
    v = pl.eval(point)
    tr = P.PoseidonTranscript()
    U, pst_proof, mipp = pl.open(tr, comms, srs, point, T)
    return comms, T, v, (U, pst_proof, mipp), tr
