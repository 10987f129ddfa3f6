"""The combined equation of tpst_pst_verify_batch restated over oracle/py
(integers, affine points, the oracle's pairing): what csrc/pst_verify_batch.hip
must decide, given the same multipliers.

An item is a dict with the oracle's values: U, point (n Fr), v, pst_proof
(m_row G2), mipp (oracle/py/pst.py mipp_prove's dict), T, and `tr`, a factory of
the item's starting transcript.  rho[j] = (rho_T, rho_2, rho_1, rho_U).

Per item (pst.py mipp_verify + pst_check, i.e. Polynomial.verify) the checks are
  (A) T prod t_l^{1/x} t_r^{x} == e(final_a, final_h)
  (B) e(g, final_h - v_h h) == prod e(pi^h_i, hmask_i - r_i h)
  (C) e(U - v g, h) == prod e(gmask_i - a_i g, pi_i)
  (D) U + sum (u_l / x + x u_r) == final_y final_a
and the batch accepts iff
  prod_j e(rho_T final_a, final_h) . (B_j)^{rho_2} . (C_j)^{rho_1}  ==  prod_j (T prod t_l^{1/x} t_r^{x})^{rho_T}
  sum_j rho_U (U + sum (u_l / x + x u_r) - final_y final_a)         ==  O
with (B_j), (C_j) written as products equal to one (right side moved over)."""
import bls377 as O
import pst as P

R = O.R


def replay(tr, mipp, b, U):
    """The transcript part of mipp_verify (pst.py:316-339): xs, xs_inv, rs, final_y, v_h."""
    tr.append_g1(U)
    xs, xs_inv = [], []
    final_y = 1
    for i, ((u_l, u_r), (t_l, t_r)) in enumerate(zip(mipp["comms_u"], mipp["comms_t"])):
        tr.append_g1(u_l)
        tr.append_g1(u_r)
        tr.append_gt(t_l)
        tr.append_gt(t_r)
        c_inv = tr.challenge_scalar()
        xs.append(pow(c_inv, -1, R))
        xs_inv.append(c_inv)
        final_y = final_y * (1 + c_inv * b[i] - b[i]) % R
    m = len(xs)
    rs = [tr.challenge_scalar() for _ in range(m)]
    vh = 1
    for i in range(m):
        vh = vh * (1 + rs[i] * xs_inv[m - i - 1] - rs[i]) % R
    return xs, xs_inv, rs, final_y, vh


def batch_accepts(srs, items, rho):
    """The combined check over all items (no per-item verdicts, no validation)."""
    g1s, g2s = [], []
    Rt = O.f12_one()
    usum = None
    for it, (rT, r2, r1, rU) in zip(items, rho):
        n = len(it["point"])
        m_col = n // 2
        m_row = n - m_col
        a, b = it["point"][:m_row], it["point"][m_row:]
        mp = it["mipp"]
        xs, xs_inv, rs, final_y, vh = replay(it["tr"](), mp, b, it["U"])
        # (A), weight rho_T
        g1s.append(O.g1_mul(mp["final_a"], rT))
        g2s.append(mp["final_h"])
        tc = it["T"]
        for (t_l, t_r), c, ci in zip(mp["comms_t"], xs, xs_inv):
            tc = O.f12_mul(tc, O.f12_mul(O.f12_pow(t_l, ci), O.f12_pow(t_r, c)))
        Rt = O.f12_mul(Rt, O.f12_pow(tc, rT))
        # (B) check_2 of final_h at rs, value v_h, weight rho_2 on the G1 side
        off = srs.nv - m_col
        g1s.append(O.g1_mul(srs.g, r2))
        g2s.append(O.g2_add(mp["final_h"], O.g2_neg(O.g2_mul(srs.h, vh))))
        for i in range(m_col):
            g1s.append(O.g1_mul(mp["pst_proof_h"][i], r2))
            g2s.append(O.g2_add(O.g2_mul(srs.h, rs[i]), O.g2_neg(srs.h_mask[off + i])))
        # (C) check of U at the reversed a, value v, weight rho_1
        arev = a[::-1]
        g1s.append(O.g1_mul(O.g1_add(it["U"], O.g1_neg(O.g1_mul(srs.g, it["v"]))), r1))
        g2s.append(srs.h)
        for i in range(m_row):
            g1s.append(O.g1_mul(O.g1_add(O.g1_mul(srs.g, arev[i]), O.g1_neg(srs.g_mask[i])), r1))
            g2s.append(it["pst_proof"][i])
        # (D), weight rho_U
        uc = it["U"]
        for (u_l, u_r), c, ci in zip(mp["comms_u"], xs, xs_inv):
            uc = O.g1_add(uc, O.g1_add(O.g1_mul(u_l, ci), O.g1_mul(u_r, c)))
        uc = O.g1_add(uc, O.g1_neg(O.g1_mul(mp["final_a"], final_y)))
        usum = O.g1_add(usum, O.g1_mul(uc, rU))
    return O.multi_pairing(g1s, g2s) == Rt and usum is None


def single_accepts(srs, it):
    """Polynomial.verify (mipp_verify + pst_check) of one item on its own transcript."""
    return P.Polynomial.verify(it["tr"](), srs, it["U"], it["point"], it["v"], it["pst_proof"], it["mipp"], it["T"])
