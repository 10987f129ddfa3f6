// What still runs on the radix "wave" engine (wave_tower.h: one wave per Fq12
// value, its op programs in LDS), and nothing else (pairing_kernels.h lists
// the pairing units):
//   gt_product_final  product of gathered Miller partials + final
//                     exponentiation (rank 0's finish of a row-sharded commit)
//   gt_pow_wave       the verifier's GT membership tests and exponentiations
#include "device_util.h"
#include "pairing_kernels.h"
#include "pairing_wave_fe.h"

namespace tpst {

// ---- product of a group's partials + final exponentiation ----------------
constexpr int FW = (int)plan::FW;          // waves per workgroup
constexpr int FW_SLOTS = 64 + 36;          // PROD, ACC, IN, TMP per wave
constexpr int FE_SLOTS = 10 * 12 + 24;     // wave 0: 10 registers + inversion temporaries
// (the op programs FE_SET of k_final_wave and k_gt_pow_wave: pairing_wave_fe.h)
constexpr size_t FW_LDS = (size_t)(FW_PROG + (wave::N_CONSTS + FW * FW_SLOTS + FE_SLOTS) * wave::SLOT) * 4;
static_assert(FW_LDS <= 65536, "final-exponentiation kernel LDS");

__device__ int fe_exp_by_x(const wave::Eng& e, const wave::lds_t* prog, int src, int r1, int r2) {
  int cur = src;
  for (int b = X_BITS - 2; b >= 0; b--) {
    int nxt = cur == r1 ? r2 : r1;
    wave::run(e, prog + FE_SET.off[FE_CYC], cur, 0, nxt);
    cur = nxt;
    if ((params::BLS_X >> b) & 1) {
      nxt = cur == r1 ? r2 : r1;
      wave::run(e, prog + FE_SET.off[FE_MUL], cur, src, nxt);
      cur = nxt;
    }
  }
  return cur;
}

// f (register F) -> f^(3(p^12-1)/r); returns the result register.  Same chain
// as final_exponentiation() in pairing.h (eprint 2020/875).  regs: ten Fq12
// registers, I: 24 slots of inversion temporaries (fe_inv).
__device__ int fe_final_exp(const wave::Eng& e, const wave::lds_t* prog, int F, int regs, int I) {
#define R(i) (regs + 12 * (i))
  fe_inv(e, prog, F, I, R(0));  // f^-1 through the tower norms and one Fq inversion
  // easy part
  wave::run(e, prog + FE_SET.off[FE_CONJ], F, 0, R(1));
  wave::run(e, prog + FE_SET.off[FE_MUL], R(1), R(0), R(2));  // r = conj(f) f^-1
  wave::run(e, prog + FE_SET.off[FE_FROB2], R(2), 0, R(1));
  wave::run(e, prog + FE_SET.off[FE_MUL], R(1), R(2), R(3));  // r = r^(p^2) r
  // hard part
  wave::run(e, prog + FE_SET.off[FE_CYC], R(3), 0, R(4));  // y0
  int t = fe_exp_by_x(e, prog, R(3), R(5), R(6));
  wave::run(e, prog + FE_SET.off[FE_CONJ], R(3), 0, R(7));  // y2 = conj(r)
  wave::run(e, prog + FE_SET.off[FE_MUL], t, R(7), R(8));   // y1 = y1 y2
  t = fe_exp_by_x(e, prog, R(8), R(5), R(6));  // y2
  wave::run(e, prog + FE_SET.off[FE_CONJ], R(8), 0, R(7));
  wave::run(e, prog + FE_SET.off[FE_MUL], R(7), t, R(9));   // y1 = conj(y1) y2
  t = fe_exp_by_x(e, prog, R(9), R(5), R(6));  // y2
  wave::run(e, prog + FE_SET.off[FE_FROB1], R(9), 0, R(7));
  wave::run(e, prog + FE_SET.off[FE_MUL], R(7), t, R(8));   // y1 = frob(y1) y2
  wave::run(e, prog + FE_SET.off[FE_MUL], R(3), R(4), R(0));  // r = r y0
  const int y0 = fe_exp_by_x(e, prog, R(8), R(5), R(6));
  const int y2 = fe_exp_by_x(e, prog, y0, y0 == R(5) ? R(6) : R(5), R(1));
  wave::run(e, prog + FE_SET.off[FE_FROB2], R(8), 0, R(2));  // y0 = frob2(y1)
  wave::run(e, prog + FE_SET.off[FE_CONJ], R(8), 0, R(3));
  wave::run(e, prog + FE_SET.off[FE_MUL], R(3), y2, R(4));   // y1 = conj(y1) y2
  wave::run(e, prog + FE_SET.off[FE_MUL], R(4), R(2), R(7));  // y1 = y1 y0
  wave::run(e, prog + FE_SET.off[FE_MUL], R(0), R(7), R(9));  // r = r y1
  return R(9);
#undef R
}

// out[g] = FE(prod of partial[g][0 .. T)): the FW waves multiply every FW-th
// partial each, wave 0 multiplies their products and runs the final
// exponentiation.  T = 0 gives 1.
__global__ void __launch_bounds__(64 * FW) k_final_wave(const Fq12* __restrict__ partial, size_t T,
                                                        Fq12* __restrict__ out) {
  extern __shared__ uint4 smem4[];
  __shared__ int acc_slot[FW];
  wave::lds_t* prog = (wave::lds_t*)(smem4);
  wave::lds_t* vals = prog + FW_PROG;
  wave::load_set(prog, FE_SET);
  wave::load_consts(vals, 0);
  __syncthreads();
  const int w = threadIdx.x >> 6;
  const size_t g = blockIdx.x;
  const int base = wave::N_CONSTS + w * FW_SLOTS;
  const wave::Eng e{vals, base, 0};
  int acc = base + 64, in = base + 76, tmp = base + 88;
  size_t cnt = 0;
  for (size_t k = w; k < T; k += FW, cnt++) {
    if (cnt == 0) {
      wave::load_f12(vals, acc, partial + g * T + k);
    } else {
      wave::load_f12(vals, in, partial + g * T + k);
      wave::run(e, prog + FE_SET.off[FE_MUL], acc, in, tmp);
      const int t = acc;
      acc = tmp;
      tmp = t;
    }
  }
  if (cnt == 0) wave::set_one(vals, acc);
  if ((threadIdx.x & 63) == 0) acc_slot[w] = acc;
  __syncthreads();
  if (w != 0) return;
  for (int v = 1; v < FW; v++) {
    wave::run(e, prog + FE_SET.off[FE_MUL], acc, acc_slot[v], tmp);
    const int t = acc;
    acc = tmp;
    tmp = t;
  }
  const int fe = wave::N_CONSTS + FW * FW_SLOTS;
  const int r = fe_final_exp(e, prog, acc, fe, fe + 120);
  wave::store_f12(vals, r, out + g);
}

// ---- tree product of the partials -------------------------------------------
// One wave per output: out[g][j] = prod of partials [g][j*CH .. j*CH+CH) (the
// tail chunk shorter).  Keeps k_final_wave's serial product short: without it
// k partials would be k / FW dependent Fq12 products per wave.
constexpr int RW = 4;
constexpr int RW_SLOTS = 64 + 36;
constexpr int RW_OPS[] = {wave::OP_F12_MUL};
constexpr wave::OpSet<1> RW_SET(RW_OPS);
constexpr int RW_PROG = RW_SET.words;
constexpr size_t RW_LDS = (size_t)(RW_PROG + (wave::N_CONSTS + RW * RW_SLOTS) * wave::SLOT) * 4;
static_assert(RW_LDS <= 65536, "tree-product kernel LDS");

__global__ void __launch_bounds__(64 * RW) k_f12_chunk_prod(const Fq12* __restrict__ in, size_t groups, size_t n,
                                                            size_t nout, Fq12* __restrict__ out, size_t chunk) {
  extern __shared__ uint4 smem4[];
  wave::lds_t* prog = (wave::lds_t*)(smem4);
  wave::lds_t* vals = prog + RW_PROG;
  wave::load_set(prog, RW_SET);
  wave::load_consts(vals, 0);
  __syncthreads();
  const int w = threadIdx.x >> 6;
  const size_t o = (size_t)blockIdx.x * RW + w;
  if (o >= groups * nout) return;
  const size_t g = o / nout, j = o % nout;
  const size_t k0 = j * chunk, k1 = (k0 + chunk < n) ? k0 + chunk : n;
  const int base = wave::N_CONSTS + w * RW_SLOTS;
  const wave::Eng e{vals, base, 0};
  int acc = base + 64, in_r = base + 76, tmp = base + 88;
  // the next factor's global load is issued before the current product runs
  // (12 lanes hold it in VGPRs), so its latency hides under the stage
  const int lane = threadIdx.x & 63;
  const Fq* src = reinterpret_cast<const Fq*>(in + g * n);
  wave::load_f12(vals, acc, in + g * n + k0);
  Fq nxt = lane < 12 && k0 + 1 < k1 ? src[12 * (k0 + 1) + lane] : Fq::zero();
  for (size_t k = k0 + 1; k < k1; k++) {
    if (lane < 12) wave::put_slot(vals, in_r + lane, nxt);
    wave::wave_sync();
    if (lane < 12 && k + 1 < k1) nxt = src[12 * (k + 1) + lane];
    wave::run(e, prog + RW_SET.off[0], acc, in_r, tmp);
    const int t = acc;
    acc = tmp;
    tmp = t;
  }
  wave::store_f12(vals, acc, out + o);
}

// groups x n partials -> groups x n' (n' <= 2 FW, what k_final_wave multiplies
// itself) by chunked tree products, one take per level (gt_product_scratch
// sums the same levels); sets partial to the buffer holding them and n to n'
static hipError_t tree_partials(Arena& ar, hipStream_t s, Fq12*& partial, size_t groups, size_t& n) {
  plan::Tree t = plan::partial_tree(n);
  for (; t.more(); t.step()) {
    const size_t nout = t.nout();
    Fq12* nxt = ar.take<Fq12>(groups * nout);
    k_f12_chunk_prod<<<grid_for(groups * nout, RW), 64 * RW, RW_LDS, s>>>(partial, groups, t.n, nout, nxt,
                                                                         plan::RW_CHUNK);
    TPST_TRY(hipGetLastError());
    partial = nxt;
  }
  n = t.n;
  return hipSuccess;
}

hipError_t gt_product_final(Arena& ar, hipStream_t s, const Fq12* d_partials, size_t groups, size_t n, Fq12* d_out) {
  if (!groups) return hipSuccess;
  Fq12* partial = const_cast<Fq12*>(d_partials);
  TPST_TRY(tree_partials(ar, s, partial, groups, n));
  k_final_wave<<<(unsigned)groups, 64 * FW, FW_LDS, s>>>(partial, n, d_out);
  return hipGetLastError();
}

// ---- GT exponentiation (MippProof::verify, mipp.rs:263-283) ---------------
// For f in GT (order r), f^p = f^x since p = x (mod r).  With e = sum_i e_i x^i
// (base-x digits; e < r < x^4, so the digits are exact, each < 2^64),
//     f^e = prod_i frob^i(f)^(e_i),
// a 4-way simultaneous exponentiation with 64-bit digits: 63 cyclotomic
// squarings and <= 64 products from the 16-entry subset table of
// (f, f^p, f^p^2, f^p^3), where the plain square-and-multiply needs 253
// squarings.  Membership first -- what arkworks' Validate::Yes
// deserialisation of a PairingOutput checks: f^(p^4) f == f^(p^2) puts f in
// the cyclotomic subgroup (order Phi12(p), so cyclotomic squaring applies),
// and then f^p == f^x puts it in GT, because gcd(p - x, Phi12(p)) = r for
// BLS12-377 (tests/test_kat_ref.py checks it).  ok[i] = 1 iff f_i is in GT
// (out[i] is only meaningful then); f = 0 is rejected first.
constexpr int GP_REGS = 20;  // R0 scratch, T1..T15 subset table, ACC, TMP, X1, X2
constexpr size_t GP_LDS = (size_t)(FW_PROG + (wave::N_CONSTS + 64 + 12 * GP_REGS) * wave::SLOT) * 4;
static_assert(GP_LDS <= 65536, "GT pow kernel LDS");

__device__ bool regs_equal(const wave::lds_t* lds, int a, int b) {
  const int lane = threadIdx.x & 63;
  const bool same = lane >= 12 || eq(wave::get_slot(lds, a + lane), wave::get_slot(lds, b + lane));
  return __all(same ? 1 : 0) != 0;
}

// one wave per exponentiation; ok == nullptr skips the membership test
__global__ void __launch_bounds__(64) k_gt_pow_wave(const Fq12* __restrict__ base, const uint64_t* __restrict__ digits,
                                                    size_t n, Fq12* __restrict__ out, uint32_t* __restrict__ ok) {
  extern __shared__ uint4 smem4[];
  wave::lds_t* prog = (wave::lds_t*)(smem4);
  wave::lds_t* vals = prog + FW_PROG;
  wave::load_set(prog, FE_SET);
  wave::load_consts(vals, 0);
  __syncthreads();
  if (blockIdx.x >= n) return;
  const size_t i = blockIdx.x;
  const uint64_t* d = digits + 4 * blockIdx.x;
  const wave::Eng e{vals, wave::N_CONSTS, 0};
#define R(k) (wave::N_CONSTS + 64 + 12 * (k))
  const int ACC = R(16), TMP = R(17), X1 = R(18), X2 = R(19);
  const wave::lds_t* P = prog;
  wave::load_f12(vals, R(1), base + i);
  const bool check = ok != nullptr;
  bool good = true;
  if (check) {
    // f = 0 passes both equations below but is not in GT (Validate::Yes rejects it)
    const int ln = threadIdx.x & 63;
    good = __any((ln < 12 && !is_zero(wave::get_slot(vals, R(1) + ln))) ? 1 : 0) != 0;
  }
  if (check && good) {  // cyclotomic subgroup: f^(p^4) f == f^(p^2)
    wave::run(e, P + FE_SET.off[FE_FROB2], R(1), 0, X1);
    wave::run(e, P + FE_SET.off[FE_FROB2], X1, 0, X2);
    wave::run(e, P + FE_SET.off[FE_MUL], X2, R(1), R(0));
    good = regs_equal(vals, R(0), X1);
  }
  // GT: f^p == f^x
  wave::run(e, P + FE_SET.off[FE_FROB1], R(1), 0, R(2));
  if (check && good) {
    const int fx = fe_exp_by_x(e, P, R(1), X1, X2);
    good = regs_equal(vals, fx, R(2));
  }
  const int lane = threadIdx.x & 63;
  if (check && lane == 0) ok[i] = good ? 1u : 0u;
  if (!good) return;
  // subset table T[m] = prod_{bit j of m} f^(p^j)
  wave::run(e, P + FE_SET.off[FE_FROB2], R(1), 0, R(4));
  wave::run(e, P + FE_SET.off[FE_FROB1], R(4), 0, R(8));
  for (int m = 3; m < 16; m++) {
    if ((m & (m - 1)) == 0) continue;  // powers of two are the bases themselves
    const int hi = 1 << (31 - __builtin_clz(m));
    wave::run(e, P + FE_SET.off[FE_MUL], R(m - hi), R(hi), R(m));
  }
  int acc = -1;
  for (int b = 63; b >= 0; b--) {
    if (acc >= 0) {
      const int nxt = acc == ACC ? TMP : ACC;
      wave::run(e, P + FE_SET.off[FE_CYC], acc, 0, nxt);
      acc = nxt;
    }
    const int mask = (int)((d[0] >> b) & 1) | (int)(((d[1] >> b) & 1) << 1) | (int)(((d[2] >> b) & 1) << 2) |
                     (int)(((d[3] >> b) & 1) << 3);
    if (!mask) continue;
    if (acc < 0) {
      acc = R(mask);
    } else {
      const int nxt = acc == ACC ? TMP : ACC;
      wave::run(e, P + FE_SET.off[FE_MUL], acc, R(mask), nxt);
      acc = nxt;
    }
  }
  if (acc < 0) {
    wave::set_one(vals, ACC);
    acc = ACC;
  }
  wave::store_f12(vals, acc, out + i);
#undef R
}

hipError_t gt_pow_wave(hipStream_t s, const Fq12* d_base, const uint64_t* d_digits, size_t n, Fq12* d_out,
                       uint32_t* d_ok) {
  if (!n) return hipSuccess;
  k_gt_pow_wave<<<(unsigned)n, 64, GP_LDS, s>>>(d_base, d_digits, n, d_out, d_ok);
  return hipGetLastError();
}

}  // namespace tpst
