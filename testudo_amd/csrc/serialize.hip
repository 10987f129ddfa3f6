// arkworks wire format (ark-serialize 0.4, Compress::Yes) of the sqrt-PST
// objects: Commitment, Proof, MippProof (mipp.rs:21-28, derive
// CanonicalSerialize), CommitterKey -- the byte strings whose lengths are the
// proof_size / commiter_key_size columns of benches/pst.rs:43-46,64-74.
// Host-only code (no device work): the proof is a few KB.  The SPARK objects
// at the end of this file (R1CSCommitment, R1CSEvalProof) and the CommitterKey
// reader hold thousands of points: their readers validate on the device.  So do
// the readers of R1CSProof and of the SNARK proof after them (wire_snark.h).
//
// Restated encoding rules (ark-serialize / ark-ff / ark-ec 0.4):
//  * Fp: canonical value, little-endian, buffer_byte_size(MODULUS_BIT_SIZE +
//    flag bits) bytes (Fq: 48, Fr: 32); flags OR-ed into the top bits of the
//    last byte.  Fq2 = c0 || c1 with the flags on c1; Fq12 = its 12 Fq
//    coefficients in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...), no flags.
//  * short-Weierstrass affine, compressed: x with SWFlags -- bit 7 =
//    YIsNegative (y > -y in the field order; Fq2 orders by c1, then c0),
//    bit 6 = PointAtInfinity (x = 0), both set is invalid.  Deserialisation
//    takes y = the smaller square root of x^3 + b when the sign bit is clear,
//    then checks on-curve and the prime-order subgroup (Validate::Yes).
//  * usize as u64 LE; Vec<T> = u64 LE length || elements; tuples and structs
//    field by field in declaration order.
// Parity: restated from the published crates (not vendored here, no Rust
// toolchain), cross-checked against the independent Python restatement in
// oracle/py/serialize.py -- parity unpinned against arkworks itself.
#include <cstring>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "curve.h"
#include "point_codec.h"
#include "wire_snark.h"
#include "wire_spark.h"

using namespace tpst;

namespace {

typedef unsigned __int128 u128;

bool lt_p(const uint64_t* a) {  // a < p (canonical Fq)
  for (int i = 5; i >= 0; i--) {
    const uint64_t pi = (uint64_t)params::FQ_P[2 * i] | ((uint64_t)params::FQ_P[2 * i + 1] << 32);
    if (a[i] != pi) return a[i] < pi;
  }
  return false;
}

Fq fq_in(const uint64_t* c) {
  Fq a;
  memcpy(a.v, c, 48);
  return to_mont(a);
}
void fq_out(const Fq& a, uint64_t* c) {
  const Fq r = from_mont(a);
  memcpy(c, r.v, 48);
}

// canonical compare of two Fq (Montgomery in)
int fq_cmp(const Fq& a, const Fq& b) {
  uint64_t x[6], y[6];
  fq_out(a, x);
  fq_out(b, y);
  for (int i = 5; i >= 0; i--)
    if (x[i] != y[i]) return x[i] < y[i] ? -1 : 1;
  return 0;
}
bool neg_flag(const Fq& y) { return fq_cmp(y, neg(y)) > 0; }
bool neg_flag(const Fq2& y) {  // QuadExtField Ord: c1 first, then c0
  const Fq2 n = neg(y);
  const int c = fq_cmp(y.c1, n.c1);
  return c != 0 ? c > 0 : fq_cmp(y.c0, n.c0) > 0;
}

// ---- exponentiation and square roots over Fq (p - 1 = 2^46 q) ----
struct BigE {
  uint64_t w[6];
};
BigE p_minus(uint64_t k) {
  BigE e;
  for (int i = 0; i < 6; i++) e.w[i] = (uint64_t)params::FQ_P[2 * i] | ((uint64_t)params::FQ_P[2 * i + 1] << 32);
  e.w[0] -= k;  // p's low limb is 1: no borrow for k <= 1
  return e;
}
BigE shr(BigE e, int s) {
  for (int k = 0; k < s; k++)
    for (int i = 0; i < 6; i++) e.w[i] = (e.w[i] >> 1) | (i < 5 ? e.w[i + 1] << 63 : 0);
  return e;
}
Fq fq_pow(const Fq& a, const BigE& e) {
  Fq r = Fq::one();
  for (int i = 5; i >= 0; i--)
    for (int b = 63; b >= 0; b--) {
      r = sqr(r);
      if ((e.w[i] >> b) & 1) r = mul(r, a);
    }
  return r;
}
constexpr int TWO_ADICITY = 46;
struct SqrtConst {
  BigE q, q1h, legendre;  // q = (p-1)/2^46, (q+1)/2, (p-1)/2
  Fq z_q;                 // z^q for a non-residue z
  SqrtConst() {
    legendre = shr(p_minus(1), 1);
    q = shr(p_minus(1), TWO_ADICITY);
    q1h = q;
    q1h.w[0] += 1;  // q odd: q + 1 has no carry beyond limb 0 unless all ones (not the case)
    q1h = shr(q1h, 1);
    Fq z = Fq::one();
    for (;;) {
      z = add(z, Fq::one());
      if (eq(fq_pow(z, legendre), neg(Fq::one()))) break;
    }
    z_q = fq_pow(z, q);
  }
};
const SqrtConst& sqc() {
  static SqrtConst c;
  return c;
}
bool is_square(const Fq& a) { return is_zero(a) || eq(fq_pow(a, sqc().legendre), Fq::one()); }

// Tonelli-Shanks; false if a is a non-residue
bool fq_sqrt(const Fq& a, Fq& out) {
  if (is_zero(a)) {
    out = a;
    return true;
  }
  if (!is_square(a)) return false;
  const SqrtConst& C = sqc();
  int m = TWO_ADICITY;
  Fq c = C.z_q, t = fq_pow(a, C.q), r = fq_pow(a, C.q1h);
  while (!eq(t, Fq::one())) {
    int i = 0;
    Fq t2 = t;
    while (!eq(t2, Fq::one())) {
      t2 = sqr(t2);
      i++;
    }
    Fq b = c;
    for (int k = 0; k < m - i - 1; k++) b = sqr(b);
    m = i;
    c = sqr(b);
    t = mul(t, c);
    r = mul(r, b);
  }
  out = r;
  return true;
}

// Fq2 = Fq[u]/(u^2 + 5): complex method
bool fq2_sqrt(const Fq2& a, Fq2& out) {
  const Fq five = mul5(Fq::one());
  if (is_zero(a.c1)) {
    Fq s;
    if (fq_sqrt(a.c0, s)) {
      out = {s, Fq::zero()};
      return true;
    }
    // a0 = c^2 u^2 = -5 c^2  ->  c = sqrt(-a0 / 5)
    if (!fq_sqrt(neg(mul(a.c0, inv(five))), s)) return false;
    out = {Fq::zero(), s};
    return true;
  }
  Fq delta;
  if (!fq_sqrt(add(sqr(a.c0), mul5(sqr(a.c1))), delta)) return false;  // norm
  const Fq half = inv(dbl(Fq::one()));
  Fq x0 = mul(add(a.c0, delta), half), c0;
  if (!fq_sqrt(x0, c0)) {
    x0 = mul(sub(a.c0, delta), half);
    if (!fq_sqrt(x0, c0)) return false;
  }
  const Fq c1 = mul(a.c1, inv(dbl(c0)));
  out = {c0, c1};
  return eq(sqr(out), a);
}

template <class F>
struct Ser;
template <>
struct Ser<Fq> {
  static constexpr int BYTES = 48, LIMBS = 12;
  static void put_x(const Fq& x, uint8_t* b) { fq_out(x, (uint64_t*)(void*)b); }
  static bool get_x(const uint8_t* b, uint8_t flags_mask, Fq& x) {
    uint64_t l[6];
    memcpy(l, b, 48);
    reinterpret_cast<uint8_t*>(l)[47] &= (uint8_t)~flags_mask;
    if (!lt_p(l)) return false;
    x = fq_in(l);
    return true;
  }
  static bool sqrt(const Fq& a, Fq& r) { return fq_sqrt(a, r); }
};
template <>
struct Ser<Fq2> {
  static constexpr int BYTES = 96, LIMBS = 24;
  static void put_x(const Fq2& x, uint8_t* b) {
    fq_out(x.c0, (uint64_t*)(void*)b);
    fq_out(x.c1, (uint64_t*)(void*)(b + 48));
  }
  static bool get_x(const uint8_t* b, uint8_t flags_mask, Fq2& x) {
    uint64_t l0[6], l1[6];
    memcpy(l0, b, 48);
    memcpy(l1, b + 48, 48);
    reinterpret_cast<uint8_t*>(l1)[47] &= (uint8_t)~flags_mask;
    if (!lt_p(l0) || !lt_p(l1)) return false;
    x = {fq_in(l0), fq_in(l1)};
    return true;
  }
  static bool sqrt(const Fq2& a, Fq2& r) { return fq2_sqrt(a, r); }
};

// canonical limbs (x || y, all-zero = infinity) -> compressed bytes
template <class F>
bool put_point(const uint64_t* p, uint8_t* b) {
  constexpr int NQ = Ser<F>::LIMBS / 12;
  bool inf = true;
  for (int i = 0; i < Ser<F>::LIMBS; i++) inf &= p[i] == 0;
  if (inf) {
    memset(b, 0, Ser<F>::BYTES);
    b[Ser<F>::BYTES - 1] = 0x40;
    return true;
  }
  for (int k = 0; k < 2 * NQ; k++)
    if (!lt_p(p + 6 * k)) return false;
  Affine<F> a;
  Fq* c = reinterpret_cast<Fq*>(&a);
  for (int k = 0; k < 2 * NQ; k++) c[k] = fq_in(p + 6 * k);
  Ser<F>::put_x(a.x, b);
  if (neg_flag(a.y)) b[Ser<F>::BYTES - 1] |= 0x80;
  return true;
}

// compressed bytes -> canonical limbs; Validate::Yes
template <class F>
bool get_point(const uint8_t* b, uint64_t* p) {
  const uint8_t fl = b[Ser<F>::BYTES - 1] & 0xC0;
  if (fl == 0xC0) return false;
  memset(p, 0, Ser<F>::LIMBS * 8);
  Affine<F> a;
  if (!Ser<F>::get_x(b, 0xC0, a.x)) return false;
  if (fl == 0x40) return true;  // PointAtInfinity
  F y;
  if (!Ser<F>::sqrt(add(mul(sqr(a.x), a.x), CurveB<F>::b()), y)) return false;
  const bool y_neg = neg_flag(y);  // y is the larger root iff its flag would be negative
  a.y = (y_neg == (fl == 0x80)) ? y : neg(y);
  if (!on_curve(a) || !is_inf(scalar_mul(a, params::FR_P, 253))) return false;
  const Fq* c = reinterpret_cast<const Fq*>(&a);
  for (int k = 0; k < Ser<F>::LIMBS / 6; k++) fq_out(c[k], p + 6 * k);
  return true;
}

struct Writer {
  uint8_t* out;
  size_t cap, n = 0;
  bool ok = true;
  void bytes(const void* d, size_t k) {
    if (out && n + k <= cap) memcpy(out + n, d, k);
    n += k;
  }
  void u64(uint64_t v) { bytes(&v, 8); }
  template <class F>
  void point(const uint64_t* p) {
    uint8_t b[Ser<F>::BYTES];
    if (!put_point<F>(p, b)) ok = false;
    bytes(b, sizeof(b));
  }
  void gt(const uint64_t* f) {
    for (int k = 0; k < 12; k++)
      if (!lt_p(f + 6 * k)) ok = false;
    bytes(f, 576);
  }
};

int finish(const Writer& w, size_t* len) {
  if (len) *len = w.n;
  if (!w.ok) return TPST_E_ARG;
  if (w.out && w.n > w.cap) return TPST_E_ARG;
  return TPST_OK;
}

struct Reader {
  const uint8_t* in;
  size_t len, n = 0;
  bool ok = true;
  const uint8_t* take(size_t k) {
    if (n + k > len) {
      ok = false;
      return nullptr;
    }
    const uint8_t* p = in + n;
    n += k;
    return p;
  }
  uint64_t u64() {
    const uint8_t* p = take(8);
    uint64_t v = 0;
    if (p) memcpy(&v, p, 8);
    return v;
  }
  template <class F>
  void point(uint64_t* out) {
    const uint8_t* p = take(Ser<F>::BYTES);
    if (!p || !get_point<F>(p, out)) ok = false;
  }
  void gt(uint64_t* out) {
    const uint8_t* p = take(576);
    if (!p) return;
    memcpy(out, p, 576);
    for (int k = 0; k < 12; k++)
      if (!lt_p(out + 6 * k)) ok = false;
  }
};

bool proof_dims_ok(const tpst_open_proof* p) {
  return p && p->m_col >= 0 && p->m_row >= 0 && p->m_col <= TPST_MAX_VARS && p->m_row <= TPST_MAX_VARS;
}

}  // namespace

extern "C" int tpst_ser_g1(const uint64_t* p, uint8_t* out48) {
  if (!p || !out48) return TPST_E_ARG;
  return put_point<Fq>(p, out48) ? TPST_OK : TPST_E_ARG;
}
extern "C" int tpst_ser_g2(const uint64_t* p, uint8_t* out96) {
  if (!p || !out96) return TPST_E_ARG;
  return put_point<Fq2>(p, out96) ? TPST_OK : TPST_E_ARG;
}
extern "C" int tpst_de_g1(const uint8_t* in48, uint64_t* p) {
  if (!p || !in48) return TPST_E_ARG;
  return get_point<Fq>(in48, p) ? TPST_OK : TPST_E_ARG;
}
extern "C" int tpst_de_g2(const uint8_t* in96, uint64_t* p) {
  if (!p || !in96) return TPST_E_ARG;
  return get_point<Fq2>(in96, p) ? TPST_OK : TPST_E_ARG;
}

// Commitment { nv: usize, g_product: G1Affine }
extern "C" int tpst_ser_commitment(int nv, const uint64_t* g1, uint8_t* out, size_t cap, size_t* len) {
  if (!g1 || nv < 0) return TPST_E_ARG;
  Writer w{out, cap};
  w.u64((uint64_t)nv);
  w.point<Fq>(g1);
  return finish(w, len);
}

// Proof { proofs: Vec<G2Affine> } (m_row entries): sqrt_pst.rs:225
extern "C" int tpst_ser_pst_proof(const tpst_open_proof* p, uint8_t* out, size_t cap, size_t* len) {
  if (!proof_dims_ok(p)) return TPST_E_ARG;
  Writer w{out, cap};
  w.u64((uint64_t)p->m_row);
  for (int i = 0; i < p->m_row; i++) w.point<Fq2>(p->pst_proof[i]);
  return finish(w, len);
}

// MippProof { comms_t: Vec<(Fq12, Fq12)>, comms_u: Vec<(G1, G1)>, final_a: G1,
//             final_h: G2, pst_proof_h: ProofG1 { proofs: Vec<G1> } }  (mipp.rs:21-28)
extern "C" int tpst_ser_mipp_proof(const tpst_open_proof* p, uint8_t* out, size_t cap, size_t* len) {
  if (!proof_dims_ok(p)) return TPST_E_ARG;
  Writer w{out, cap};
  w.u64((uint64_t)p->m_col);
  for (int i = 0; i < p->m_col; i++) {
    w.gt(p->comms_t[i][0]);
    w.gt(p->comms_t[i][1]);
  }
  w.u64((uint64_t)p->m_col);
  for (int i = 0; i < p->m_col; i++) {
    w.point<Fq>(p->comms_u[i][0]);
    w.point<Fq>(p->comms_u[i][1]);
  }
  w.point<Fq>(p->final_a);
  w.point<Fq2>(p->final_h);
  w.u64((uint64_t)p->m_col);
  for (int i = 0; i < p->m_col; i++) w.point<Fq>(p->pst_proof_h[i]);
  return finish(w, len);
}

// inverse of the two above (U is serialised separately as a Commitment):
// fills m_row / m_col and every element, validating each point
extern "C" int tpst_de_open_proof(const uint8_t* pst, size_t pst_len, const uint8_t* mipp, size_t mipp_len,
                                  tpst_open_proof* out) {
  if (!pst || !mipp || !out) return TPST_E_ARG;
  memset(out, 0, sizeof(*out));
  Reader a{pst, pst_len};
  const uint64_t m_row = a.u64();
  if (!a.ok || m_row > TPST_MAX_VARS) return TPST_E_ARG;
  out->m_row = (int32_t)m_row;
  for (uint64_t i = 0; i < m_row; i++) a.point<Fq2>(out->pst_proof[i]);
  if (!a.ok || a.n != pst_len) return TPST_E_ARG;
  Reader b{mipp, mipp_len};
  const uint64_t m_col = b.u64();
  if (!b.ok || m_col > TPST_MAX_VARS) return TPST_E_ARG;
  out->m_col = (int32_t)m_col;
  for (uint64_t i = 0; i < m_col; i++) {
    b.gt(out->comms_t[i][0]);
    b.gt(out->comms_t[i][1]);
  }
  if (b.u64() != m_col) return TPST_E_ARG;
  for (uint64_t i = 0; i < m_col; i++) {
    b.point<Fq>(out->comms_u[i][0]);
    b.point<Fq>(out->comms_u[i][1]);
  }
  b.point<Fq>(out->final_a);
  b.point<Fq2>(out->final_h);
  if (b.u64() != m_col) return TPST_E_ARG;
  for (uint64_t i = 0; i < m_col; i++) b.point<Fq>(out->pst_proof_h[i]);
  if (!b.ok || b.n != mipp_len) return TPST_E_ARG;
  return TPST_OK;
}

// CommitterKey { nv: usize, powers_of_g: Vec<Vec<G1>>, powers_of_h: Vec<Vec<G2>>,
// g: G1, h: G2 } (ark-poly-commit multilinear_pc data_structures, after trim)
// from the flat SRS layout of tpst_srs_export
extern "C" int tpst_ser_committer_key(int nv, const uint64_t* flat, size_t flat_len, uint8_t* out, size_t cap,
                                      size_t* len) {
  if (!flat || nv < 1 || nv > TPST_MAX_VARS || flat_len != tpst_srs_flat_len(nv)) return TPST_E_ARG;
  const uint64_t* g = flat;
  const uint64_t* h = flat + 12;
  std::vector<const uint64_t*> pg(nv), ph(nv);
  size_t off = 36;
  for (int i = 0; i < nv; i++) {
    pg[i] = flat + off;
    off += ((size_t)1 << (nv - i)) * 12;
    ph[i] = flat + off;
    off += ((size_t)1 << (nv - i)) * 24;
  }
  Writer w{out, cap};
  w.u64((uint64_t)nv);
  w.u64((uint64_t)nv);
  for (int i = 0; i < nv; i++) {
    const size_t k = (size_t)1 << (nv - i);
    w.u64(k);
    for (size_t j = 0; j < k; j++) w.point<Fq>(pg[i] + 12 * j);
  }
  w.u64((uint64_t)nv);
  for (int i = 0; i < nv; i++) {
    const size_t k = (size_t)1 << (nv - i);
    w.u64(k);
    for (size_t j = 0; j < k; j++) w.point<Fq2>(ph[i] + 24 * j);
  }
  w.point<Fq>(g);
  w.point<Fq2>(h);
  return finish(w, len);
}

// ======================================================== SPARK objects ==
// R1CSCommitment, R1CSEvalProof and the reader of CommitterKey.  The layouts
// are the item lists of wire_spark.h (restated there from r1csinstance.rs:
// 55-61, 336-339, sparse_mlpoly.rs:52-55, 84-87, 325-332, 691-700, 1043-1050,
// 1337-1341, 1441-1445, product_tree.rs:138-170, sumcheck.rs:19-22,
// unipoly.rs:7-11, nizk/mod.rs:31-38, nizk/bullet.rs:19-23).  The writers are
// host only.  The readers walk the structure on the host, range-check every Fr,
// then hand all the object's points to the device in one batch per group
// (point_codec.hip): these objects hold thousands of points.
namespace {

bool lt_r(const uint64_t* a) {  // a < r (canonical Fr)
  for (int i = 3; i >= 0; i--) {
    const uint64_t ri = (uint64_t)params::FR_P[2 * i] | ((uint64_t)params::FR_P[2 * i + 1] << 32);
    if (a[i] != ri) return a[i] < ri;
  }
  return false;
}

// a G1 point of these objects: canonical and on the curve (one product chain; the subgroup is the
// reader's to check), or the writer reports TPST_E_ARG
void put_g1_checked(Writer& w, const uint64_t* p) {
  w.point<Fq>(p);
  if (w.ok && !on_curve(G1A{fq_in(p), fq_in(p + 6)})) w.ok = false;
}

// the rounds fields of the three openings, as the sizes fix them
void set_rounds(const tpst_r1cs_eval_sizes& z, tpst_r1cs_eval_proof* p) {
  p->proof_ops.rounds = wire::open_rounds(z.ell_ops);
  p->proof_mem.rounds = wire::open_rounds(z.ell_mem);
  p->proof_derefs.rounds = wire::open_rounds(z.ell_derefs);
}
bool rounds_ok(const tpst_r1cs_eval_sizes& z, const tpst_r1cs_eval_proof* p) {
  return p->proof_ops.rounds == wire::open_rounds(z.ell_ops) && p->proof_mem.rounds == wire::open_rounds(z.ell_mem) &&
         p->proof_derefs.rounds == wire::open_rounds(z.ell_derefs);
}

void write_items(Writer& w, const std::vector<wire::Item>& items, const uint64_t* const* bufs) {
  for (const wire::Item& it : items) {
    if (it.kind == wire::LEN) {
      w.u64((uint64_t)it.count);
      continue;
    }
    const uint64_t* src = bufs[it.buf] + it.word;
    for (size_t j = 0; j < it.count; j++) {
      if (it.kind == wire::FR) {
        if (!lt_r(src + 4 * j)) w.ok = false;
        w.bytes(src + 4 * j, 32);
      } else if (it.kind == wire::G1) {
        put_g1_checked(w, src + 12 * j);
      } else if (it.kind == wire::G2) {
        w.point<Fq2>(src + 24 * j);
      } else {
        w.gt(src + 72 * j);
      }
    }
  }
}

// the elements of a walked input into the caller's buffers: every Fr and Fq12 range-checked and copied, every
// point of `kind` decompressed and validated in one device batch.  TPST_E_ARG on any rejection.
int read_items(tpst_ctx* ctx, const uint8_t* in, const std::vector<wire::Item>& items, const std::vector<size_t>& offs,
               uint64_t* const* bufs) {
  for (size_t i = 0; i < items.size(); i++) {
    const wire::Item& it = items[i];
    if (it.kind == wire::GT) {  // 12 Fq each, no flags
      uint64_t* dst = bufs[it.buf] + it.word;
      memcpy(dst, in + offs[i], it.count * 576);
      for (size_t j = 0; j < 12 * it.count; j++)
        if (!lt_p(dst + 6 * j)) return fail(ctx, TPST_E_ARG, "wire format: Fq12 coefficient >= p");
      continue;
    }
    if (it.kind != wire::FR) continue;
    uint64_t* dst = bufs[it.buf] + it.word;
    memcpy(dst, in + offs[i], it.count * 32);
    for (size_t j = 0; j < it.count; j++)
      if (!lt_r(dst + 4 * j)) return fail(ctx, TPST_E_ARG, "wire format: scalar >= r");
  }
  for (wire::Kind kind : {wire::G1, wire::G2}) {
    const size_t B = wire::KIND_BYTES[kind], W = wire::KIND_WORDS[kind];
    size_t n = 0;
    for (const wire::Item& it : items)
      if (it.kind == kind) n += it.count;
    if (!n) continue;
    std::vector<uint8_t> packed(n * B);  // n is bounded by the input's length: the walk placed every run
    std::vector<uint64_t> limbs(n * W);
    size_t k = 0;
    for (size_t i = 0; i < items.size(); i++)
      if (items[i].kind == kind) {
        memcpy(&packed[k * B], in + offs[i], items[i].count * B);
        k += items[i].count;
      }
    size_t bad = n;
    const int rc = kind == wire::G1 ? point_decompress_batch<Fq>(ctx, packed.data(), n, limbs.data(), &bad)
                                    : point_decompress_batch<Fq2>(ctx, packed.data(), n, limbs.data(), &bad);
    if (rc) return rc;
    if (bad != n) return fail(ctx, TPST_E_ARG, "wire format: invalid point encoding");
    k = 0;
    for (const wire::Item& it : items)
      if (it.kind == kind) {
        memcpy(bufs[it.buf] + it.word, &limbs[k * W], it.count * W * 8);
        k += it.count;
      }
  }
  return TPST_OK;
}

}  // namespace

extern "C" int tpst_ser_r1cs_commitment(size_t num_cons, size_t num_vars, size_t num_inputs, size_t num_ops,
                                        size_t num_mem_cells, const uint64_t* comm_ops, size_t ops_rows,
                                        const uint64_t* comm_mem, size_t mem_rows, uint8_t* out, size_t cap,
                                        size_t* len) {
  size_t want_ops, want_mem;
  if (!comm_ops || !comm_mem || !wire::commitment_rows(num_ops, num_mem_cells, &want_ops, &want_mem) ||
      ops_rows != want_ops || mem_rows != want_mem)
    return TPST_E_ARG;
  Writer w{out, cap};
  for (size_t v : {num_cons, num_vars, num_inputs, wire::BATCH_SIZE, num_ops, num_mem_cells}) w.u64((uint64_t)v);
  w.u64((uint64_t)ops_rows);
  for (size_t i = 0; i < ops_rows; i++) put_g1_checked(w, comm_ops + 12 * i);
  w.u64((uint64_t)mem_rows);
  for (size_t i = 0; i < mem_rows; i++) put_g1_checked(w, comm_mem + 12 * i);
  return finish(w, len);
}

extern "C" int tpst_de_r1cs_commitment(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t dims[5],
                                       uint64_t* comm_ops, size_t ops_cap, size_t* ops_rows, uint64_t* comm_mem,
                                       size_t mem_cap, size_t* mem_rows) {
  if (!ctx || !in || !dims || !ops_rows || !mem_rows) return fail(ctx, TPST_E_ARG, "null argument");
  wire::CommitmentWalk w;
  if (!wire::walk_commitment(in, len, w)) return fail(ctx, TPST_E_ARG, "wire format: malformed R1CSCommitment");
  for (int k = 0; k < 5; k++) dims[k] = (size_t)w.dims[k];
  *ops_rows = w.ops_rows;
  *mem_rows = w.mem_rows;
  if (!comm_ops && !comm_mem && !ops_cap && !mem_cap) return TPST_OK;  // dimensions only
  if (!comm_ops || !comm_mem) return fail(ctx, TPST_E_ARG, "null argument");
  if (w.ops_rows > ops_cap || w.mem_rows > mem_cap) return fail(ctx, TPST_E_ARG, "wire format: capacity too small");
  const std::vector<wire::Item> items = {{wire::G1, 0, w.ops_rows, 0}, {wire::G1, 1, w.mem_rows, 0}};
  const std::vector<size_t> offs = {w.ops_off, w.mem_off};
  uint64_t* const bufs[2] = {comm_ops, comm_mem};
  return read_items(ctx, in, items, offs, bufs);
}

extern "C" int tpst_ser_r1cs_eval_proof(const tpst_r1cs_eval_sizes* sizes, const tpst_r1cs_eval_proof* proof,
                                        const uint64_t* comm_derefs, const uint64_t* prod_ops,
                                        const uint64_t* prod_mem, uint8_t* out, size_t cap, size_t* len) {
  std::vector<wire::Item> items;
  if (!sizes || !proof || !comm_derefs || !prod_ops || !prod_mem || !wire::proof_items(*sizes, items) ||
      !rounds_ok(*sizes, proof))
    return TPST_E_ARG;
  const uint64_t* const bufs[4] = {reinterpret_cast<const uint64_t*>(proof), comm_derefs, prod_ops, prod_mem};
  Writer w{out, cap};
  write_items(w, items, bufs);
  return finish(w, len);
}

extern "C" int tpst_de_r1cs_eval_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, const tpst_r1cs_eval_sizes* sizes,
                                       tpst_r1cs_eval_proof* proof, uint64_t* comm_derefs, uint64_t* prod_ops,
                                       uint64_t* prod_mem) {
  if (!ctx || !in || !sizes || !proof || !comm_derefs || !prod_ops || !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<wire::Item> items;
  std::vector<size_t> offs;
  if (!wire::proof_items(*sizes, items)) return fail(ctx, TPST_E_ARG, "wire format: sizes no proof has");
  if (!wire::walk_items(in, len, items, offs)) return fail(ctx, TPST_E_ARG, "wire format: malformed R1CSEvalProof");
  memset(proof, 0, sizeof(*proof));
  set_rounds(*sizes, proof);
  uint64_t* const bufs[4] = {reinterpret_cast<uint64_t*>(proof), comm_derefs, prod_ops, prod_mem};
  return read_items(ctx, in, items, offs, bufs);
}

extern "C" int tpst_de_committer_key(tpst_ctx* ctx, const uint8_t* in, size_t len, int* nv, uint64_t* flat,
                                     size_t flat_cap, size_t* flat_len) {
  if (!ctx || !in || !nv || !flat_len) return fail(ctx, TPST_E_ARG, "null argument");
  std::vector<wire::Item> items;
  std::vector<size_t> offs;
  if (!wire::walk_committer_key(in, len, nv, items, offs))
    return fail(ctx, TPST_E_ARG, "wire format: malformed CommitterKey");
  const int n = *nv;
  *flat_len = tpst_srs_flat_len(n);
  if (!flat && !flat_cap) return TPST_OK;  // dimensions only
  if (!flat) return fail(ctx, TPST_E_ARG, "null argument");
  if (*flat_len > flat_cap) return fail(ctx, TPST_E_ARG, "wire format: capacity too small");
  uint64_t* const bufs[1] = {flat};
  if (int rc = read_items(ctx, in, items, offs, bufs)) return rc;
  // the flat SRS ends with the verifier's masks g^{t_i}, h^{t_i}, which the key does not carry:
  // powers_of_g[i][x] = g^{eq(t[i..], x)} with t_i on x's lowest bit, so g^{t_i} is the sum of
  // level i's odd entries (eq sums to 1 over the other variables)
  size_t off = 36;
  uint64_t* gmask = flat + *flat_len - (size_t)n * 36;
  uint64_t* hmask = gmask + (size_t)n * 12;
  std::vector<uint64_t> odd, ones;
  for (int i = 0; i < n; i++) {
    const size_t h = (size_t)1 << (n - i - 1);
    ones.assign(4 * h, 0);
    for (size_t x = 0; x < h; x++) ones[4 * x] = 1;
    odd.resize(24 * h);
    for (size_t x = 0; x < h; x++) memcpy(&odd[12 * x], flat + off + 12 * (2 * x + 1), 96);
    if (int rc = tpst_g1_msm(ctx, odd.data(), h, ones.data(), h, gmask + 12 * i)) return rc;
    off += 2 * h * 12;
    for (size_t x = 0; x < h; x++) memcpy(&odd[24 * x], flat + off + 24 * (2 * x + 1), 192);
    if (int rc = tpst_g2_msm(ctx, odd.data(), h, ones.data(), h, hmask + 24 * i)) return rc;
    off += 2 * h * 24;
  }
  return TPST_OK;
}

// ================================================ R1CSProof, SNARK proof ==
// The layouts are the item lists of wire_snark.h (restated there from
// r1csproof.rs:32-53, sumcheck.rs:19-22, unipoly.rs:7-11, sqrt_pst.rs:201-204,
// mipp.rs:21-28).  Elements are written and read by the routines above: the
// same point, Fq12 and Fr codecs as Commitment, Proof and MippProof, the
// points of a whole object validated in one device batch per group.
namespace {

wire::SatDims dims_of_proof(const tpst_r1cs_proof* p) {
  return {p->rounds_x, p->rounds_y, p->open.m_col, p->open.m_row};
}

// the dimension fields of a proof just read
void set_sat_dims(const wire::SatDims& d, tpst_r1cs_proof* p) {
  p->rounds_x = d.rounds_x, p->rounds_y = d.rounds_y, p->num_vars_log = d.m_col + d.m_row;
  p->open.m_col = d.m_col, p->open.m_row = d.m_row;
}

}  // namespace

extern "C" int tpst_ser_r1cs_proof(const tpst_r1cs_proof* proof, uint8_t* out, size_t cap, size_t* len) {
  std::vector<wire::Item> items;
  if (!proof || proof->num_vars_log != proof->open.m_col + proof->open.m_row ||
      !wire::r1cs_proof_items(dims_of_proof(proof), items))
    return TPST_E_ARG;
  const uint64_t* const bufs[1] = {reinterpret_cast<const uint64_t*>(proof)};
  Writer w{out, cap};
  write_items(w, items, bufs);
  return finish(w, len);
}

extern "C" int tpst_de_r1cs_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t num_cons, size_t num_vars,
                                  tpst_r1cs_proof* proof) {
  if (!ctx || !in || !proof) return fail(ctx, TPST_E_ARG, "null argument");
  wire::SatDims d;
  std::vector<wire::Item> items;
  std::vector<size_t> offs;
  if (!wire::sat_dims(num_cons, num_vars, d) || !wire::r1cs_proof_items(d, items))
    return fail(ctx, TPST_E_ARG, "wire format: dimensions no R1CSProof has");
  if (!wire::walk_snark_items(in, len, items, offs)) return fail(ctx, TPST_E_ARG, "wire format: malformed R1CSProof");
  memset(proof, 0, sizeof(*proof));
  set_sat_dims(d, proof);
  uint64_t* const bufs[1] = {reinterpret_cast<uint64_t*>(proof)};
  return read_items(ctx, in, items, offs, bufs);
}

extern "C" int tpst_ser_snark_proof(const tpst_r1cs_eval_sizes* sizes, const tpst_snark_proof* proof,
                                    const uint64_t* comm_derefs, const uint64_t* prod_ops, const uint64_t* prod_mem,
                                    uint8_t* out, size_t cap, size_t* len) {
  std::vector<wire::Item> items;
  if (!sizes || !proof || !comm_derefs || !prod_ops || !prod_mem ||
      proof->sat.num_vars_log != proof->sat.open.m_col + proof->sat.open.m_row ||
      !wire::snark_items(dims_of_proof(&proof->sat), *sizes, items) || !rounds_ok(*sizes, &proof->eval))
    return TPST_E_ARG;
  const uint64_t* bufs[wire::S_NBUF];
  bufs[wire::S_SAT] = reinterpret_cast<const uint64_t*>(&proof->sat);
  bufs[wire::S_EVAL] = reinterpret_cast<const uint64_t*>(&proof->eval);
  bufs[wire::S_DEREFS] = comm_derefs, bufs[wire::S_PROD_OPS] = prod_ops, bufs[wire::S_PROD_MEM] = prod_mem;
  bufs[wire::S_EVALS] = &proof->inst_evals[0][0];
  Writer w{out, cap};
  write_items(w, items, bufs);
  return finish(w, len);
}

extern "C" int tpst_de_snark_proof(tpst_ctx* ctx, const uint8_t* in, size_t len, size_t num_cons, size_t num_vars,
                                   const tpst_r1cs_eval_sizes* sizes, tpst_snark_proof* proof, uint64_t* comm_derefs,
                                   uint64_t* prod_ops, uint64_t* prod_mem) {
  if (!ctx || !in || !sizes || !proof || !comm_derefs || !prod_ops || !prod_mem)
    return fail(ctx, TPST_E_ARG, "null argument");
  wire::SatDims d;
  std::vector<wire::Item> items;
  std::vector<size_t> offs;
  if (!wire::sat_dims(num_cons, num_vars, d) || !wire::snark_items(d, *sizes, items))
    return fail(ctx, TPST_E_ARG, "wire format: dimensions no proof has");
  if (!wire::walk_snark_items(in, len, items, offs)) return fail(ctx, TPST_E_ARG, "wire format: malformed SNARK proof");
  memset(proof, 0, sizeof(*proof));
  set_sat_dims(d, &proof->sat);
  set_rounds(*sizes, &proof->eval);
  uint64_t* bufs[wire::S_NBUF];
  bufs[wire::S_SAT] = reinterpret_cast<uint64_t*>(&proof->sat);
  bufs[wire::S_EVAL] = reinterpret_cast<uint64_t*>(&proof->eval);
  bufs[wire::S_DEREFS] = comm_derefs, bufs[wire::S_PROD_OPS] = prod_ops, bufs[wire::S_PROD_MEM] = prod_mem;
  bufs[wire::S_EVALS] = &proof->inst_evals[0][0];
  return read_items(ctx, in, items, offs, bufs);
}
