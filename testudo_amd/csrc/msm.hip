// Host side of the MSM engine (see msm.h for the pipeline and the layout of
// its sources) and the G1 instantiations of the variable-base MSM.
#include "msm_var.h"

namespace tpst {

hipError_t Arena::reserve(size_t bytes) {
  if (bytes <= cap) return hipSuccess;
  if (base) {
    hipError_t e = hipFree(base);
    if (e != hipSuccess) return e;
    base = nullptr;
    cap = 0;
  }
  size_t want = bytes + (bytes >> 3);
  hipError_t e = hipMalloc(&base, want);
  if (e != hipSuccess) return e;
  cap = want;
  return hipSuccess;
}

void Profiler::begin(int st, hipStream_t s) {
  if (!on) return;
  if (used[st] + 2 > ev[st].size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    ev[st].push_back(a);
    ev[st].push_back(b);
  }
  (void)hipEventRecord(ev[st][used[st]], s);
}

void Profiler::end(int st, hipStream_t s) {
  if (!on || used[st] + 2 > ev[st].size()) return;
  (void)hipEventRecord(ev[st][used[st] + 1], s);
  used[st] += 2;
}

void Profiler::collect() {
  for (int st = 0; st < N_STAGES; st++) {
    for (size_t i = 0; i + 1 < used[st]; i += 2) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[st][i], ev[st][i + 1]) == hipSuccess) {
        total_ms[st] += ms;
        count[st] += 1;
      }
    }
    used[st] = 0;
  }
}

void Profiler::reset() {
  for (int st = 0; st < N_STAGES; st++) {
    used[st] = 0;
    total_ms[st] = 0;
    count[st] = 0;
  }
}

Profiler::~Profiler() {
  for (auto& v : ev)
    for (auto e : v) (void)hipEventDestroy(e);
}

void Arena::release() {
  if (base) (void)hipFree(base);
  base = nullptr;
  cap = off = 0;
  if (aux_ready) {
    for (auto& st : aux) {
      (void)hipStreamSynchronize(st);
      if (!aux_from) (void)hipStreamDestroy(st);
      st = nullptr;
    }
    for (auto& e : aux_ev) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
    aux_ready = false;
  }
}

hipError_t Arena::aux_init() {
  if (aux_ready) return hipSuccess;
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
  if (aux_from) {
    TPST_TRY(aux_from->aux_init());
    for (int i = 0; i < N_AUX; i++) aux[i] = aux_from->aux[i];
  } else {
    for (auto& st : aux) TPST_TRY(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest));
  }
  for (auto& e : aux_ev) TPST_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  aux_ready = true;
  return hipSuccess;
}

int msm_window_bits(size_t n) {
  // 16-bit signed windows are the sweet spot for ~2^18..2^22 points; smaller
  // inputs use smaller windows so buckets stay populated.
  int lg = bit_length(n ? n - 1 : 0);
  if (lg >= 20) return 16;
  if (lg >= 16) return 13;
  if (lg >= 12) return 10;
  if (lg >= 8) return 7;
  return 4;
}

int batch_window_bits(size_t N) {
  // rows of 1024 / 2048 scalars: 11-bit windows (2^20 commit 7.35 -> 7.05 ms
  // against 10; 12 -> 13 at 4096 was slower, 65.2 -> 65.8 ms:
  // profiles/r06/ab/ab_k1_window.txt)
  int lg = bit_length(N ? N - 1 : 0);
  if (lg >= 12) return 12;
  if (lg >= 10) return 11;
  if (lg >= 6) return 7;
  return 4;
}

// explicit instantiations (G1)
template hipError_t msm_var<Fq>(Arena&, hipStream_t, const uint32_t*, const uint32_t*, size_t, Xyzz<Fq>*, hipStream_t,
                                bool*, hipStream_t, bool);
template hipError_t points_to_mont<Fq>(hipStream_t, const uint32_t*, uint32_t*, size_t);
template hipError_t affine_from_mont<Fq>(hipStream_t, const uint32_t*, uint32_t*, size_t);
template hipError_t xyzz_to_affine_canonical<Fq>(hipStream_t, const Xyzz<Fq>*, uint32_t*, size_t);

}  // namespace tpst
