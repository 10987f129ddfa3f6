// Batched point decompression and validation on the device.
//
// The wire-format reader works point by point on one host thread (get_point<F>
// in serialize.hip): a Tonelli-Shanks root and a 253-bit [r]P per point.  A
// SPARK commitment or a committer key holds thousands of points, and the
// verifiers validate as many row commitments (host::point_in_subgroup).  Here
// every point is one device lane, blocks of 64 like k_gens_from_seeds:
//
//   k_point_decompress<F>  48 / 96 compressed bytes -> canonical x || y limbs
//                          (all-zero for infinity) and a status byte, by the
//                          steps of get_point<F>;
//   k_point_check<F>       canonical affine limbs -> the status byte
//                          host::point_in_subgroup<F> would give.
//
// The host routines are the definition of right: same verdict on every input
// (the infinity flag over any canonical x is infinity; x = p - 1 on G1 has
// y = 0 and order 2; x = 0 is a point of order 3), same limbs where they
// accept.  The subgroup test is the host's plain double-and-add by r.  The
// path is latency-bound: one serial chain per lane.
#define TPST_FQ2_ATTR TPST_NI  // out-of-line Fq2 products: not a throughput path
#include <chrono>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/tpst.h"
#include "ctx.h"
#include "device_util.h"
#include "fq_sqrt.h"
#include "point_codec.h"
#include "pst_state.h"  // point_valid: the verifiers' host loop below the threshold

using namespace tpst;

namespace {

struct CodecConsts {
  SqrtConsts s;
  uint32_t inv5[12];  // 1 / 5 (Montgomery): the Fq2 root of a = -5 c^2
};

__constant__ uint32_t FR_MODULUS[8] = {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu,
                                       0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};

// Fq2 = Fq[u]/(u^2 + 5), complex method: the port of fq2_sqrt (serialize.hip)
__device__ bool fq2_sqrt_dev(const Fq2& a, const CodecConsts& K, Fq2& out) {
  if (is_zero(a.c1)) {
    Fq s;
    if (fq_sqrt_dev(a.c0, K.s, s)) {
      out = {s, Fq::zero()};
      return true;
    }
    // a0 = c^2 u^2 = -5 c^2  ->  c = sqrt(-a0 / 5)
    if (!fq_sqrt_dev(neg(mul(a.c0, Fq::from_limbs(K.inv5))), K.s, s)) return false;
    out = {Fq::zero(), s};
    return true;
  }
  Fq delta;
  if (!fq_sqrt_dev(add(sqr(a.c0), mul5(sqr(a.c1))), K.s, delta)) return false;  // norm
  const Fq half = Fq::from_limbs(params::FQ_TWO_INV);
  Fq x0 = mul(add(a.c0, delta), half), c0;
  if (!fq_sqrt_dev(x0, K.s, c0)) {
    x0 = mul(sub(a.c0, delta), half);
    if (!fq_sqrt_dev(x0, K.s, c0)) return false;
  }
  const Fq c1 = mul(a.c1, inv(dbl(c0)));
  out = {c0, c1};
  return eq(sqr(out), a);
}

// per coordinate field: the root and the order of y against -y (neg_flag)
template <class F>
struct Codec;
template <>
struct Codec<Fq> {
  static constexpr int NQ = 1;
  static __device__ bool sqrt(const Fq& a, const CodecConsts& K, Fq& r) { return fq_sqrt_dev(a, K.s, r); }
  static __device__ bool y_larger(const Fq& y) { return cmp_canon(y, neg(y)) > 0; }
};
template <>
struct Codec<Fq2> {
  static constexpr int NQ = 2;
  static __device__ bool sqrt(const Fq2& a, const CodecConsts& K, Fq2& r) { return fq2_sqrt_dev(a, K, r); }
  static __device__ bool y_larger(const Fq2& y) {  // QuadExtField Ord: c1 first, then c0
    const Fq2 n = neg(y);
    const int c = cmp_canon(y.c1, n.c1);
    return c != 0 ? c > 0 : cmp_canon(y.c0, n.c0) > 0;
  }
};

// canonical words -> Montgomery element / back (NQ Fq coefficients)
template <class F>
__device__ F words_to_mont(const uint32_t* w) {
  F r;
  Fq* c = reinterpret_cast<Fq*>(&r);
  for (int q = 0; q < Codec<F>::NQ; q++) c[q] = to_mont(Fq::from_limbs(w + 12 * q));
  return r;
}
template <class F>
__device__ void store_canon(uint32_t* o, const F& v) {
  const Fq* c = reinterpret_cast<const Fq*>(&v);
  for (int q = 0; q < Codec<F>::NQ; q++) store_f<Fq>(o + 12 * q, from_mont(c[q]));
}

template <class F>
__device__ bool in_subgroup(const Affine<F>& a) {
  return on_curve(a) && is_inf(scalar_mul(a, FR_MODULUS, 253));
}

// one lane per point; status 0 = accepted, 1 = rejected
template <class F>
__global__ void __launch_bounds__(64) k_point_decompress(const uint32_t* __restrict__ in, size_t n, CodecConsts K,
                                                        uint32_t* __restrict__ out, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NQ = Codec<F>::NQ, W = 12 * NQ;
  uint32_t w[W];
#pragma unroll
  for (int k = 0; k < W; k++) w[k] = in[W * i + k];
  const uint32_t fl = w[W - 1] >> 30;  // SWFlags: 2 = YIsNegative, 1 = PointAtInfinity, 3 invalid
  w[W - 1] &= 0x3fffffffu;
  uint32_t* o = out + 2 * W * i;
#pragma unroll
  for (int k = 0; k < 2 * W; k++) o[k] = 0;
  bool ok = fl != 3;
  for (int q = 0; q < NQ; q++) ok = ok && lt_p_words(w + 12 * q);
  if (ok && fl != 1) {
    Affine<F> a;
    a.x = words_to_mont<F>(w);
    F y;
    ok = Codec<F>::sqrt(add(mul(sqr(a.x), a.x), CurveB<F>::b()), K, y);
    if (ok) {
      // y is the larger root iff its flag would be negative
      a.y = (Codec<F>::y_larger(y) == (fl == 2)) ? y : neg(y);
      ok = in_subgroup(a);
    }
    if (ok) {
      store_canon<F>(o, a.x);
      store_canon<F>(o + W, a.y);
    }
  }
  status[i] = ok ? 0 : 1;
}

template <class F>
__global__ void __launch_bounds__(64) k_point_check(const uint32_t* __restrict__ pts, size_t n,
                                                   uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NQ = Codec<F>::NQ, W = 12 * NQ;
  uint32_t w[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) w[k] = pts[2 * W * i + k];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 2 * W; k++) any |= w[k];
  bool ok = true;
  for (int q = 0; q < 2 * NQ; q++) ok = ok && lt_p_words(w + 12 * q);
  if (ok && any) {  // all-zero = infinity = valid
    Affine<F> a;
    a.x = words_to_mont<F>(w);
    a.y = words_to_mont<F>(w + W);
    ok = in_subgroup(a);
  }
  status[i] = ok ? 0 : 1;
}

const CodecConsts& codec_consts() {
  static const CodecConsts K = [] {
    CodecConsts k;
    k.s = sqrt_consts();
    const Fq i5 = inv(mul5(Fq::one()));
    memcpy(k.inv5, i5.v, 48);
    return k;
  }();
  return K;
}

size_t first_set(const std::vector<uint8_t>& st) {
  size_t i = 0;
  while (i < st.size() && !st[i]) i++;
  return i;
}

}  // namespace

namespace tpst {

template <class F>
int point_decompress_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad) {
  *first_bad = n;
  if (n == 0) return TPST_OK;
  constexpr size_t W = Words<F>::n;  // u32 per compressed point; 2 W per affine point
  const CodecConsts& K = codec_consts();
  std::vector<uint8_t> st(n);
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(n * W, 4) + Arena::need(n * 2 * W, 4) + Arena::need(n, 1)));
  uint32_t* d_in = ctx->io.take<uint32_t>(n * W);
  uint32_t* d_out = ctx->io.take<uint32_t>(n * 2 * W);
  uint8_t* d_st = ctx->io.take<uint8_t>(n);
  TPST_HIP(ctx, hipMemcpyAsync(d_in, in, n * W * 4, hipMemcpyHostToDevice, s));
  ctx->prof.begin(ST_POINT_CODEC, s);
  k_point_decompress<F><<<grid_for(n, 64), 64, 0, s>>>(d_in, n, K, d_out, d_st);
  ctx->prof.end(ST_POINT_CODEC, s);
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(out, d_out, n * 2 * W * 4, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipMemcpyAsync(st.data(), d_st, n, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  *first_bad = first_set(st);
  return TPST_OK;
}

template <class F>
int point_status_batch_locked(tpst_ctx* ctx, const uint64_t* pts, size_t n, uint8_t* status) {
  if (n == 0) return TPST_OK;
  constexpr size_t W = Words<F>::n;
  hipStream_t s = ctx->stream;
  ctx->io.reset();
  TPST_HIP(ctx, ctx->io.reserve(Arena::need(n * 2 * W, 4) + Arena::need(n, 1)));
  uint32_t* d_pts = ctx->io.take<uint32_t>(n * 2 * W);
  uint8_t* d_st = ctx->io.take<uint8_t>(n);
  TPST_HIP(ctx, hipMemcpyAsync(d_pts, pts, n * 2 * W * 4, hipMemcpyHostToDevice, s));
  ctx->prof.begin(ST_POINT_CODEC, s);
  k_point_check<F><<<grid_for(n, 64), 64, 0, s>>>(d_pts, n, d_st);
  ctx->prof.end(ST_POINT_CODEC, s);
  TPST_HIP(ctx, hipGetLastError());
  TPST_HIP(ctx, hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, s));
  TPST_HIP(ctx, hipStreamSynchronize(s));
  return TPST_OK;
}

template <class F>
int point_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad) {
  *first_bad = n;
  if (n == 0) return TPST_OK;
  std::vector<uint8_t> st(n);
  std::lock_guard<tpst::CtxMutex> lk(ctx->mu);
  TPST_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = point_status_batch_locked<F>(ctx, pts, n, st.data())) return rc;
  *first_bad = first_set(st);
  return TPST_OK;
}

// the verifiers' host loop: point_valid over every row on up to 16 host threads
static bool rows_valid_host(const uint64_t* pts, size_t n) {
  std::vector<char> bad(n, 0);
  host::parallel_for(n, [&](size_t i) { bad[i] = !point_valid<Fq>(pts + 12 * i); });
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok = ok && !bad[i];
  return ok;
}

int g1_rows_valid(tpst_ctx* ctx, const uint64_t* pts, size_t n, bool* ok) {
  if (n >= POINT_CHECK_DEVICE_MIN) {
    size_t bad = n;
    if (int rc = point_check_batch<Fq>(ctx, pts, n, &bad)) return rc;
    *ok = bad == n;
    return TPST_OK;
  }
  *ok = rows_valid_host(pts, n);
  return TPST_OK;
}

int g1_rows_host_bench(tpst_ctx* ctx, size_t n, int iters, double* ms) {
  if (n > ((size_t)1 << 20)) return fail(ctx, TPST_E_ARG, "more than 2^20 points");
  std::vector<uint64_t> k(4 * n, 0), pts(12 * n);
  for (size_t i = 0; i < n; i++) k[4 * i] = i + 1;
  if (int rc = tpst_g1_mul_generator(ctx, k.data(), n, pts.data())) return rc;
  bool ok = rows_valid_host(pts.data(), n);  // warm-up
  const auto t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < iters; it++) ok = rows_valid_host(pts.data(), n) && ok;
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / iters;
  return ok ? TPST_OK : fail(ctx, TPST_E_VERIFY, "a generator multiple failed the host check");
}

template int point_decompress_batch<Fq>(tpst_ctx*, const uint8_t*, size_t, uint64_t*, size_t*);
template int point_decompress_batch<Fq2>(tpst_ctx*, const uint8_t*, size_t, uint64_t*, size_t*);
template int point_check_batch<Fq>(tpst_ctx*, const uint64_t*, size_t, size_t*);
template int point_check_batch<Fq2>(tpst_ctx*, const uint64_t*, size_t, size_t*);
template int point_status_batch_locked<Fq>(tpst_ctx*, const uint64_t*, size_t, uint8_t*);
template int point_status_batch_locked<Fq2>(tpst_ctx*, const uint64_t*, size_t, uint8_t*);

}  // namespace tpst

namespace {

// the largest batch one call takes: 2^26 points, as tpst_gens_new
constexpr size_t MAX_BATCH = (size_t)1 << 26;

template <class F>
int de_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad) {
  if (!ctx || (n && (!in || !out))) return fail(ctx, TPST_E_ARG, "null argument");
  if (n > MAX_BATCH) return fail(ctx, TPST_E_ARG, "more than 2^26 points: split the batch");
  size_t bad = n;
  if (int rc = point_decompress_batch<F>(ctx, in, n, out, &bad)) return rc;
  if (first_bad) *first_bad = bad;
  return bad == n ? TPST_OK : fail(ctx, TPST_E_ARG, "invalid point encoding at index " + std::to_string(bad));
}

template <class F>
int check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad) {
  if (!ctx || (n && !pts)) return fail(ctx, TPST_E_ARG, "null argument");
  if (n > MAX_BATCH) return fail(ctx, TPST_E_ARG, "more than 2^26 points: split the batch");
  size_t bad = n;
  if (int rc = point_check_batch<F>(ctx, pts, n, &bad)) return rc;
  if (first_bad) *first_bad = bad;
  return bad == n ? TPST_OK : fail(ctx, TPST_E_VERIFY, "invalid point at index " + std::to_string(bad));
}

}  // namespace

extern "C" int tpst_de_g1_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad) {
  return de_batch<Fq>(ctx, in, n, out, first_bad);
}
extern "C" int tpst_de_g2_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad) {
  return de_batch<Fq2>(ctx, in, n, out, first_bad);
}
extern "C" int tpst_g1_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad) {
  return check_batch<Fq>(ctx, pts, n, first_bad);
}
extern "C" int tpst_g2_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad) {
  return check_batch<Fq2>(ctx, pts, n, first_bad);
}
