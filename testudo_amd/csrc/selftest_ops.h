// Per-element dispatch of the arithmetic self-tests (tpst_selftest_field /
// tpst_selftest_curve, selftest.hip): one field or curve operation on
// operands given as u32 words, exactly as the kernels hold them.  Everything
// here is TPST_HD, so tests/cpp/test_selftest_ops.cpp runs the same dispatch
// on the host (field.h's host product is a different algorithm from the
// device one: the host run proves the vectors and the expected values, the
// device run the device code).  The 4-lane (coop.h), pair (pair_fq2.h),
// Fq2x29 (acc_field.h) and glv_split forms are device-only and live in
// selftest.hip.
#pragma once
#include "curve.h"

namespace tpst {
namespace selftest {

// ---- field ops: op = family * 32 + index ---------------------------------
enum : int { FAM_FQ = 0, FAM_FR = 1, FAM_F29 = 2, FAM_FQ2 = 3, FAM_FQ2P = 4, N_FAM = 5 };
// Fq / Fr (field.h words: 12 / 8 per operand)
enum : int { F_MUL, F_SQR, F_ADD, F_SUB, F_NEG, F_TO_MONT, F_FROM_MONT, F_N };
// Fq29: operands and results are the radix-2^29 value itself (R = 2^377)
// packed as pack377 writes it, 12 words; from_std takes field.h words;
// the *4 forms take (a, c) and (b, d) as two packed values per operand
enum : int {
  F29_MUL, F29_SQR, F29_MUL_SUM, F29_MUL_SUB, F29_ADD, F29_SUB, F29_CNEG, F29_P_MINUS, F29_TO_STD,
  F29_TO_STD_MUL, F29_FROM_STD, F29_ROUNDTRIP, F29_MUL_SUM4, F29_MUL_SUB4, F29_N
};
enum : int { F2_MUL, F2_SQR, F2_N };                 // Fq2, 24 words per operand
enum : int { F2P_MUL, F2P_IS_ZERO, F2P_EQ, F2P_N };  // pair_fq2.h; flags: one word per lane of the pair

TPST_HD int field_family(int op) { return op >> 5; }
TPST_HD int field_index(int op) { return op & 31; }

TPST_HD bool field_op_valid(int op) {
  if (op < 0) return false;
  const int f = field_family(op), i = field_index(op);
  return f == FAM_FQ || f == FAM_FR ? i < F_N
         : f == FAM_F29             ? i < F29_N
         : f == FAM_FQ2             ? i < F2_N
         : f == FAM_FQ2P            ? i < F2P_N
                                    : false;
}

// u32 words per operand (a and b alike) and per result
TPST_HD int field_in_words(int op) {
  const int f = field_family(op), i = field_index(op);
  if (f == FAM_FR) return 8;
  if (f == FAM_FQ2 || f == FAM_FQ2P) return 24;
  if (f == FAM_F29 && (i == F29_MUL_SUM4 || i == F29_MUL_SUB4)) return 24;
  return 12;
}
TPST_HD int field_out_words(int op) {
  const int f = field_family(op), i = field_index(op);
  if (f == FAM_FR) return 8;
  if (f == FAM_FQ2) return 24;
  if (f == FAM_FQ2P) return i == F2P_MUL ? 24 : 2;
  return 12;
}

template <class C>
TPST_HD void fp_op(int idx, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const Fp<C> x = Fp<C>::from_limbs(a), y = Fp<C>::from_limbs(b);
  Fp<C> r;
  switch (idx) {
    case F_MUL: r = mul(x, y); break;
    case F_SQR: r = sqr(x); break;
    case F_ADD: r = add(x, y); break;
    case F_SUB: r = sub(x, y); break;
    case F_NEG: r = neg(x); break;
    case F_TO_MONT: r = to_mont(x); break;
    default: r = from_mont(x); break;
  }
#pragma unroll
  for (int i = 0; i < C::N; i++) out[i] = r.v[i];
}

TPST_HD void f29_op(int idx, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (idx == F29_FROM_STD) {
    pack377(from_std(Fq::from_limbs(a)), out);
    return;
  }
  const Fq29 x = unpack377(a), y = unpack377(b);
  if (idx == F29_TO_STD || idx == F29_TO_STD_MUL) {
    const Fq r = idx == F29_TO_STD ? to_std(x) : to_std_mul(x);
#pragma unroll
    for (int i = 0; i < 12; i++) out[i] = r.v[i];
    return;
  }
  Fq29 r;
  switch (idx) {
    case F29_MUL: r = mul(x, y); break;
    case F29_SQR: r = sqr(x); break;
    case F29_MUL_SUM: r = mul_sum(x, y, x, x); break;
    case F29_MUL_SUB: r = mul_sub(x, y, y, y); break;
    case F29_ADD: r = add(x, y); break;
    case F29_SUB: r = sub(x, y); break;
    case F29_CNEG: r = cneg(x, true); break;
    case F29_P_MINUS: r = p_minus(x); break;
    case F29_MUL_SUM4: r = mul_sum(x, y, unpack377(a + 12), unpack377(b + 12)); break;
    case F29_MUL_SUB4: r = mul_sub(x, y, unpack377(a + 12), unpack377(b + 12)); break;
    default: r = x; break;  // F29_ROUNDTRIP
  }
  pack377(r, out);
}

TPST_HD Fq2 load_fq2(const uint32_t* w) { return {Fq::from_limbs(w), Fq::from_limbs(w + 12)}; }
TPST_HD void store_fq2(uint32_t* w, const Fq2& a) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    w[i] = a.c0.v[i];
    w[12 + i] = a.c1.v[i];
  }
}

TPST_HD void fq2_op(int idx, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const Fq2 x = load_fq2(a), y = load_fq2(b);
  store_fq2(out, idx == F2_MUL ? mul(x, y) : sqr(x));
}

// one lane-form field op (every family but FAM_FQ2P); false: not a lane op
TPST_HD bool field_lane_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (!field_op_valid(op)) return false;
  const int i = field_index(op);
  switch (field_family(op)) {
    case FAM_FQ: fp_op<FqCfg>(i, a, b, out); return true;
    case FAM_FR: fp_op<FrCfg>(i, a, b, out); return true;
    case FAM_F29: f29_op(i, a, b, out); return true;
    case FAM_FQ2: fq2_op(i, a, b, out); return true;
    default: return false;
  }
}

// ---- curve ops: op = form * 16 + index -----------------------------------
// p is XYZZ; q is XYZZ too, and the mixed operations read its X, Y as the
// affine point (infinity: X = Y = 0); the result is XYZZ.  Words are field.h
// Montgomery words (R = 2^384), except FORM_FQ29_PK: the accumulation
// kernels' packed bucket format (R = 2^377, pack377) for p, q and the result.
// FORM_FQ2_ACC is the G2 tail kernels' Xyzz<Fq2x29> (acc_field.h) through
// load_acc / store_acc; the FORM_COOP_* forms are coop.h's add_affine_quad /
// add_quad / dbl_quad, 4 lanes per operation, on Xyzz<Fq29> (through
// load_acc, or load_pk for the packed buckets) and on Xyzz<Fq2x29>.
enum : int {
  FORM_FQ, FORM_FQ29_ACC, FORM_FQ29_PK, FORM_FQ2, FORM_COOP_FQ29_ACC, FORM_COOP_FQ2_ACC, FORM_PAIR, FORM_GLV,
  FORM_COOP_FQ29_PK, FORM_FQ2_ACC, N_FORM
};
enum : int { C_ADD_AFFINE, C_ADD, C_DBL, C_DBL_AFFINE, C_SUB_AFFINE, C_TO_AFFINE, C_N };
// chain-start forms: FORM_UNIT + a lane form (FORM_FQ .. FORM_FQ2), C_ADD_AFFINE
// only, runs add_affine_unit (curve.h) in that form's codec; p must be
// infinity or have ZZ = ZZZ = 1
constexpr int FORM_UNIT = 16;
constexpr int C_GLV_SPLIT = 0;  // FORM_GLV: 8-word canonical scalar in p (q unused) -> k1 | k2

TPST_HD int curve_form(int op) { return op >> 4; }
TPST_HD bool curve_form_unit(int f) { return f >= FORM_UNIT && f <= FORM_UNIT + FORM_FQ2; }
TPST_HD bool curve_form_coop(int f) {
  return f == FORM_COOP_FQ29_ACC || f == FORM_COOP_FQ29_PK || f == FORM_COOP_FQ2_ACC;
}
TPST_HD int curve_index(int op) { return op & 15; }

TPST_HD bool curve_op_valid(int op) {
  if (op < 0) return false;
  const int f = curve_form(op), i = curve_index(op);
  if (f <= FORM_FQ2) return i < C_N;
  if (curve_form_unit(f)) return i == C_ADD_AFFINE;
  if (curve_form_coop(f)) return i == C_ADD_AFFINE || i == C_ADD || i == C_DBL;
  if (f == FORM_PAIR || f == FORM_FQ2_ACC) return i <= C_SUB_AFFINE;  // no Fq2P / Fq2x29 inverse: no to_affine
  return f == FORM_GLV && i == C_GLV_SPLIT;
}

// u32 words per element of p, q and the result
TPST_HD int curve_words(int op) {
  const int f = curve_form_unit(curve_form(op)) ? curve_form(op) - FORM_UNIT : curve_form(op);
  const bool g2 = f == FORM_FQ2 || f == FORM_COOP_FQ2_ACC || f == FORM_PAIR || f == FORM_FQ2_ACC;
  return f == FORM_GLV ? 8 : g2 ? 96 : 48;
}

template <int COP, class F>
TPST_HD Xyzz<F> curve_op(const Xyzz<F>& p, const Xyzz<F>& q) {
  const Affine<F> qa = {q.X, q.Y};
  if constexpr (COP == C_ADD_AFFINE)
    return add_affine(p, qa);
  else if constexpr (COP == C_ADD)
    return add(p, q);
  else if constexpr (COP == C_DBL)
    return dbl(p);
  else if constexpr (COP == C_DBL_AFFINE)
    return dbl_affine(qa);
  else if constexpr (COP == C_SUB_AFFINE)
    return sub_affine(p, qa);
  else
    return to_xyzz(to_affine(p));
}

// the chain-start mixed add in place of C_ADD_AFFINE (FORM_UNIT forms)
template <class F>
TPST_HD Xyzz<F> curve_op_unit(const Xyzz<F>& p, const Xyzz<F>& q) {
  return add_affine_unit(p, Affine<F>{q.X, q.Y});
}

template <class F>
TPST_HD Xyzz<F> curve_op_rt(int cop, const Xyzz<F>& p, const Xyzz<F>& q, bool unit = false) {
  if (unit) return curve_op_unit(p, q);
  switch (cop) {
    case C_ADD_AFFINE: return curve_op<C_ADD_AFFINE>(p, q);
    case C_ADD: return curve_op<C_ADD>(p, q);
    case C_DBL: return curve_op<C_DBL>(p, q);
    case C_DBL_AFFINE: return curve_op<C_DBL_AFFINE>(p, q);
    case C_SUB_AFFINE: return curve_op<C_SUB_AFFINE>(p, q);
    default: return curve_op<C_TO_AFFINE>(p, q);
  }
}

// word codecs of the lane forms (what AccField<Fq>::in / out and load_pk /
// store_pk of acc_field.h do around the device kernels' loads and stores)
TPST_HD Xyzz<Fq> load_xyzz_words(const uint32_t* w) {
  return {Fq::from_limbs(w), Fq::from_limbs(w + 12), Fq::from_limbs(w + 24), Fq::from_limbs(w + 36)};
}
TPST_HD void store_xyzz_words(uint32_t* w, const Xyzz<Fq>& v) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    w[i] = v.X.v[i];
    w[12 + i] = v.Y.v[i];
    w[24 + i] = v.ZZ.v[i];
    w[36 + i] = v.ZZZ.v[i];
  }
}

// one lane-form curve op on the host's side of the codecs; false: not a lane form
TPST_HD bool curve_lane_op(int op, const uint32_t* p, const uint32_t* q, uint32_t* out) {
  if (!curve_op_valid(op)) return false;
  const int cop = curve_index(op);
  const bool unit = curve_form_unit(curve_form(op));
  switch (unit ? curve_form(op) - FORM_UNIT : curve_form(op)) {
    case FORM_FQ:
      store_xyzz_words(out, curve_op_rt(cop, load_xyzz_words(p), load_xyzz_words(q), unit));
      return true;
    case FORM_FQ29_ACC: {
      const Xyzz<Fq> a = load_xyzz_words(p), b = load_xyzz_words(q);
      const Xyzz<Fq29> r = curve_op_rt<Fq29>(cop, {from_std(a.X), from_std(a.Y), from_std(a.ZZ), from_std(a.ZZZ)},
                                             {from_std(b.X), from_std(b.Y), from_std(b.ZZ), from_std(b.ZZZ)}, unit);
      store_xyzz_words(out, {to_std(r.X), to_std(r.Y), to_std(r.ZZ), to_std(r.ZZZ)});
      return true;
    }
    case FORM_FQ29_PK: {
      const Xyzz<Fq29> r =
          curve_op_rt<Fq29>(cop, {unpack377(p), unpack377(p + 12), unpack377(p + 24), unpack377(p + 36)},
                            {unpack377(q), unpack377(q + 12), unpack377(q + 24), unpack377(q + 36)}, unit);
      pack377(r.X, out);
      pack377(r.Y, out + 12);
      pack377(r.ZZ, out + 24);
      pack377(r.ZZZ, out + 36);
      return true;
    }
    case FORM_FQ2: {
      const Xyzz<Fq2> r = curve_op_rt<Fq2>(cop, {load_fq2(p), load_fq2(p + 24), load_fq2(p + 48), load_fq2(p + 72)},
                                           {load_fq2(q), load_fq2(q + 24), load_fq2(q + 48), load_fq2(q + 72)}, unit);
      store_fq2(out, r.X);
      store_fq2(out + 24, r.Y);
      store_fq2(out + 48, r.ZZ);
      store_fq2(out + 72, r.ZZZ);
      return true;
    }
    default: return false;
  }
}

// ---- tower ops (tpst_selftest_tower): op = engine << 8 | in codec << 7 | out codec << 6 | index
// The pairing's two Fq12 engines on caller-chosen operands: the RNS chain
// engine (rns_engine.h: 12 waves and two elements per workgroup) and the
// radix wave engine (wave_tower.h: one wave per element).  Codecs (RNS engine
// only; the wave engine is TW_FQ in and out): TW_FQ = field.h Montgomery Fq12
// in tower order, 144 words, through rns::load (k = 1) / rns::store, or
// wave::load_f12 / store_f12; TW_RES = 12 x 32 raw residue words (channel
// lane & 31 of every coefficient's slot, any slot integer < 16 p) through
// rns::load_res / store_res.
enum : int { TE_RNS = 0, TE_WAVE = 1, N_TE = 2 };
enum : int { TW_FQ = 0, TW_RES = 1 };
// single stages (a, b -> out; b is read by T_F12_MUL and T_GT_POW only), then
// the composites: T_INV the engines' Fq12 inversion (rc_inv / fe_inv, the head
// of both final exponentiations), T_FINAL_EXP gt_prod_final with W = 1,
// T_G2_PREPARE g2_prepare_batch (a = n affine G2 points, 48 words each; out =
// 69 LineCoeff per point, coefficient-major: coefficient idx of point i at
// out + 72 (idx n + i)), T_GT_POW gt_pow_wave (a = base, b = 4 u64 base-x
// digits, 8 words; out = n x 144 result words, then n membership words ok[i],
// then one zero word when n is odd; the result of an element with ok == 0 is
// left zero), T_PASS no stage at all (RNS engine: the load straight into the
// store, so FQ -> RES is rns::load alone and RES -> FQ rns::store alone on the
// caller's slot integers)
enum : int {
  T_F12_MUL, T_F12_SQR, T_CYC_SQR, T_FROB1, T_FROB2, T_FROB3, T_CONJ, T_COPY, T_INV, T_FINAL_EXP, T_G2_PREPARE,
  T_GT_POW, T_PASS, T_N
};
constexpr int TOWER_FQ_WORDS = 144, TOWER_RES_WORDS = 12 * 32, TOWER_G2_WORDS = 48, TOWER_LINES_WORDS = 69 * 72;

TPST_HD int tower_engine(int op) { return op >> 8; }
TPST_HD int tower_codec_in(int op) { return (op >> 7) & 1; }
TPST_HD int tower_codec_out(int op) { return (op >> 6) & 1; }
TPST_HD int tower_index(int op) { return op & 63; }
TPST_HD int tower_op(int engine, int cin, int cout, int idx) { return engine << 8 | cin << 7 | cout << 6 | idx; }

TPST_HD bool tower_op_valid(int op) {
  if (op < 0) return false;
  const int e = tower_engine(op), i = tower_index(op);
  const bool fq = tower_codec_in(op) == TW_FQ && tower_codec_out(op) == TW_FQ;
  if (e == TE_RNS) return i <= T_INV || i == T_PASS || (fq && (i == T_FINAL_EXP || i == T_G2_PREPARE));
  if (e == TE_WAVE)
    return fq && (i == T_F12_MUL || i == T_CYC_SQR || i == T_FROB1 || i == T_FROB2 || i == T_CONJ || i == T_INV ||
                  i == T_GT_POW);
  return false;
}
TPST_HD bool tower_reads_b(int op) { return tower_index(op) == T_F12_MUL || tower_index(op) == T_GT_POW; }
// u32 words per element of a, of b (0: b is not read and may be null) and of
// the result (T_GT_POW: without the n + (n & 1) trailing membership words)
TPST_HD int tower_a_words(int op) {
  if (tower_index(op) == T_G2_PREPARE) return TOWER_G2_WORDS;
  return tower_codec_in(op) == TW_RES ? TOWER_RES_WORDS : TOWER_FQ_WORDS;
}
TPST_HD int tower_b_words(int op) {
  if (!tower_reads_b(op)) return 0;
  return tower_index(op) == T_GT_POW ? 8 : tower_a_words(op);
}
TPST_HD int tower_out_words(int op) {
  if (tower_index(op) == T_G2_PREPARE) return TOWER_LINES_WORDS;
  return tower_codec_out(op) == TW_RES ? TOWER_RES_WORDS : TOWER_FQ_WORDS;
}

}  // namespace selftest
}  // namespace tpst
