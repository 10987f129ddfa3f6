// Batched point decompression and validation on the device (point_codec.hip):
// the host-side entry the C-ABI, the wire-format readers and the verifiers share.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct tpst_ctx;

namespace tpst {

// From this many row commitments up the verifiers (sparse_eval.hip points_ok,
// hyrax.hip tpst_hyrax_eval_verify) validate them with k_point_check instead of
// the 16-thread host loop.  The smallest power of two from which the device
// check won in every median of tools/point_codec_time.py: the kernel is one
// serial 253-step chain per lane, 5.6 ms at any n measured, against 4.6 ms of
// the host loop at 512 points and 9.0 ms at 1024 (profiles/point_codec/README.md).
constexpr size_t POINT_CHECK_DEVICE_MIN = 1024;

// n compressed points (48 / 96 bytes each, host memory) -> n x 12 / 24 canonical
// limbs in `out`; *first_bad = the lowest rejected index, n if none.  Takes the
// context lock.  TPST_OK or TPST_E_HIP (the verdict is *first_bad alone).
template <class F>
int point_decompress_batch(tpst_ctx* ctx, const uint8_t* in, size_t n, uint64_t* out, size_t* first_bad);

// n canonical affine points (host memory) -> *first_bad as above
template <class F>
int point_check_batch(tpst_ctx* ctx, const uint64_t* pts, size_t n, size_t* first_bad);

// the same launch for a caller that already holds the context lock (the batch
// verifier): status[i] = 0 accepted, 1 rejected, for every point.  Stages in
// ctx->io (reset here) and synchronises the stream.
template <class F>
int point_status_batch_locked(tpst_ctx* ctx, const uint64_t* pts, size_t n, uint8_t* status);

// The verifiers' check of n row commitments (canonical affine G1, host memory):
// the host loop on up to 16 threads below POINT_CHECK_DEVICE_MIN, the device
// check from there.  *ok = every point is valid.  TPST_OK or TPST_E_HIP.
int g1_rows_valid(tpst_ctx* ctx, const uint64_t* pts, size_t n, bool* ok);

// tpst_microbench kind 20: the host loop of g1_rows_valid alone (whatever n) over the first n
// multiples of the G1 generator; *ms = host milliseconds of one pass, the mean of `iters` passes.
// The threshold above is this against tpst_g1_check_batch (tools/point_codec_time.py).
int g1_rows_host_bench(tpst_ctx* ctx, size_t n, int iters, double* ms);

}  // namespace tpst
