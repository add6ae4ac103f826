// Streaming entry points (include/dspcore_stream.h): the biquad cascade with
// an entry and an exit state, the host geometry of one SRC block, and the
// history roll of the SRC staging rows.
//
// k_iir_stream is the fused cascade of iir.hip shaped for streaming -- many
// channels, short rows -- with the carry scan seeded by the caller's state:
//   one wavefront per channel, lane c = chunk c of T = 32 ceil(n / 2048)
//   samples (C = ceil(n / T) <= 64);
//   pass 1: every chunk but the last runs the cascade from rest, E_c;
//   scan:   S_0 = zi, S_{c+1} = A^T S_c + E_c (step 0 included: S_1 = A^T zi
//           + E_0, where the one-shot scan starts from S_0 = 0 and skips it);
//   pass 2: chunk c reruns from S_c, clips, stores.
// Everything is wave-private: LDS instructions of one wave execute in program
// order, so the tile hand-offs and the scan need compiler fences only.
//
// Exit state.  Pass 2 runs whole 32-sample tiles (outputs past the row's end
// are not stored), so a lane's registers after the loop have advanced past the
// row's end whenever n % 32 != 0.  The state after exactly n samples is taken
// inside pass 2: after local sample n - 1 - (C - 1) T (a wave-uniform test of
// the sample index) lane C - 1 stores its delay lines to zf straight from the
// loop.  The state is never clipped.
//
// Non-finite input follows iir.hip: a chunk whose end state picked up an inf
// or NaN hands an all-NaN state on (nf_poison), so does a non-finite zi, and
// so does the exit state.
#include <vector>

#include "cascade.h"
#include "dspcore_stream.h"
#include "stream_pass.h"

namespace dsp {
namespace {

constexpr int kRollNT = 256;
constexpr int kRollPer = DSP_STREAM_MAX_HIST / kRollNT;

struct ScanMatrix {
  double P[16 * 16];  // A^T, row-major D x D, D = 2S <= 16
};

// The passes and the scan are stream_pass.h's (shared with iir_bank.hip).
// S: instantiated stage count (the caller's S padded with identity stages);
// Du = 2 * (the caller's S): the state components zi / zf carry.
template <int S, bool NORM>
__global__ __launch_bounds__(kWave) void k_iir_stream(const float* x, float* y, int64_t n,
                                                      int64_t ld_x, int64_t ld_y, SosParams p,
                                                      ScanMatrix sp, int64_t T, int C, int clip,
                                                      const double* zi, double* zf,
                                                      int64_t ld_state, int Du, int vec_x,
                                                      int vec_y) {
  constexpr int D = 2 * S;
  __shared__ __attribute__((aligned(16))) float tile[kWave * kRow];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  stream_row<S, Df2Cascade<NORM>>(x + b * ld_x, y + b * ld_y, tile, n, T, C, lane, p, clip,
                                  zi ? zi + b * ld_state : nullptr,
                                  zf ? zf + b * ld_state : nullptr, Du, vec_x, vec_y,
                                  [&](double (&prow)[D]) {
#pragma unroll
                                    for (int j = 0; j < D; ++j) prow[j] = sp.P[lane * D + j];
                                  });
}

// S == 0: y = x, clipped when asked.
__global__ __launch_bounds__(256) void k_stream_clip(const float* x, float* y, int64_t n,
                                                     int64_t ld_x, int64_t ld_y, int64_t per_row,
                                                     int clip) {
  const int64_t b = blockIdx.x / per_row;
  const int64_t i = (blockIdx.x - b * per_row) * 256 + threadIdx.x;
  if (i >= n) return;
  const float clo = clip ? -1.f : -INFINITY, chi = clip ? 1.f : INFINITY;
  y[b * ld_y + i] = clip_f32(x[b * ld_x + i], clo, chi);
}

// One block per row: the whole history is in registers before any of it is
// written (the ranges overlap when n_block < hist).
__global__ __launch_bounds__(kRollNT) void k_stream_roll(float* buf, int64_t ld, int hist,
                                                         int64_t n_block) {
  float* r = buf + (int64_t)blockIdx.x * ld;
  float v[kRollPer];
#pragma unroll
  for (int i = 0; i < kRollPer; ++i) {
    const int at = i * kRollNT + threadIdx.x;
    v[i] = at < hist ? r[n_block + at] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kRollPer; ++i) {
    const int at = i * kRollNT + threadIdx.x;
    if (at < hist) r[at] = v[i];
  }
}

template <int S>
int run_stream(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x, int64_t ld_y,
               const SosParams& p, bool norm, int clip, const double* zi, double* zf,
               int64_t ld_state, int Du, hipStream_t s) {
  const int64_t T = kTS * ceil_div(n, kMaxChunk);
  const int C = (int)ceil_div(n, T);
  ScanMatrix sp;
  const std::vector<double> P = chunk_transition(p, S, T);
  for (size_t i = 0; i < P.size(); ++i) sp.P[i] = P[i];
  const int vec_x = ((ld_x & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const int vec_y = ((ld_y & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0);
  TraceScope trace("iir_stream", s);
  if (norm)
    hipLaunchKernelGGL((k_iir_stream<S, true>), dim3((unsigned)B), dim3(kWave), 0, s, x, y, n, ld_x,
                       ld_y, p, sp, T, C, clip, zi, zf, ld_state, Du, vec_x, vec_y);
  else
    hipLaunchKernelGGL((k_iir_stream<S, false>), dim3((unsigned)B), dim3(kWave), 0, s, x, y, n,
                       ld_x, ld_y, p, sp, T, C, clip, zi, zf, ld_state, Du, vec_x, vec_y);
  DSP_LAUNCHED("k_iir_stream");
  return DSP_OK;
}

int launch_stream_cascade(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                          int64_t ld_y, const double* sos, int S, int clip, const double* zi,
                          double* zf, int64_t ld_state, hipStream_t s) {
  DSP_REQUIRE(B >= 0 && n >= 0, "bad sizes B=%lld n=%lld", (long long)B, (long long)n);
  DSP_REQUIRE(S >= 0, "S=%d is negative", S);
  if (S > DSP_STREAM_MAX_STAGES)
    return set_error(DSP_ENOTSUP, "the streaming cascade takes S <= %d stages (S=%d)",
                     DSP_STREAM_MAX_STAGES, S);
  DSP_REQUIRE(ld_x >= n && ld_y >= n, "leading dimension too small");
  DSP_REQUIRE(ld_state >= 2 * (int64_t)S, "ld_state=%lld < 2S=%d", (long long)ld_state, 2 * S);
  DSP_REQUIRE(n <= ((int64_t)1 << 30) && B <= INT32_MAX, "block too large");
  if (B == 0 || n == 0) return DSP_OK;
  DSP_REQUIRE(x && y, "null pointer");
  DSP_REQUIRE(S == 0 || sos, "null sos");
  if (S == 0) {
    if (!clip && x == y) return DSP_OK;
    const int64_t per_row = ceil_div(n, 256);
    DSP_REQUIRE(per_row * B <= INT32_MAX, "block too large");
    TraceScope trace("iir_stream", s);
    hipLaunchKernelGGL(k_stream_clip, dim3((unsigned)(per_row * B)), dim3(256), 0, s, x, y, n, ld_x,
                       ld_y, per_row, clip);
    DSP_LAUNCHED("k_stream_clip");
    return DSP_OK;
  }
  SosParams p;
  const bool norm = realize(sos, S, &p);
  const int Du = 2 * S;
#define DSP_STREAM_CASE(SP) \
  return run_stream<SP>(x, y, B, n, ld_x, ld_y, p, norm, clip, zi, zf, ld_state, Du, s)
  switch (S == 7 ? 8 : S) {  // 7 stages run as 8 with an exact identity stage
    case 1: DSP_STREAM_CASE(1);
    case 2: DSP_STREAM_CASE(2);
    case 3: DSP_STREAM_CASE(3);
    case 4: DSP_STREAM_CASE(4);
    case 5: DSP_STREAM_CASE(5);
    case 6: DSP_STREAM_CASE(6);
    default: DSP_STREAM_CASE(8);
  }
#undef DSP_STREAM_CASE
}

int stream_src_geometry(int K, int L, int M, int64_t consumed, int64_t produced, int64_t n_block,
                        int flush, int64_t* hist, int64_t* c_offset, int64_t* n_out) {
  DSP_REQUIRE(hist && c_offset && n_out, "null output pointer");
  DSP_REQUIRE(K >= 1 && (K & 1) && L >= 1 && M >= 1, "bad K=%d (odd, >= 1) L=%d M=%d", K, L, M);
  DSP_REQUIRE(L <= (1 << 24) && M <= (1 << 24), "L=%d or M=%d out of range", L, M);
  constexpr int64_t kMaxCount = (int64_t)1 << 56;
  DSP_REQUIRE(consumed >= 0 && produced >= 0 && n_block >= 0, "negative sample count");
  DSP_REQUIRE(consumed <= kMaxCount && produced <= kMaxCount && n_block <= kMaxCount,
              "sample count out of range");
  DSP_REQUIRE(!flush || n_block == 0, "a flush takes no input (n_block=%lld)", (long long)n_block);
  const int64_t h = (K + L - 1) / L - 1;
  if (h > DSP_STREAM_MAX_HIST)
    return set_error(DSP_ENOTSUP, "SRC history ceil(K/L)-1=%lld exceeds %d samples", (long long)h,
                     DSP_STREAM_MAX_HIST);
  typedef __int128 wide;
  const wide c = (K - 1) / 2;
  // outputs computable from `total` inputs: m with (m M + c) div L < total
  auto ready = [&](int64_t total) -> wide {
    const wide num = (wide)total * L - c;
    return num <= 0 ? (wide)0 : (num + M - 1) / M;
  };
  DSP_REQUIRE((wide)produced == ready(consumed),
              "produced=%lld is not what consumed=%lld inputs make computable (%lld)",
              (long long)produced, (long long)consumed, (long long)ready(consumed));
  const wide upto = flush ? ((wide)consumed * L + M - 1) / M : ready(consumed + n_block);
  *hist = h;
  *c_offset = (int64_t)((wide)produced * M + c - ((wide)consumed - h) * L);
  *n_out = (int64_t)(upto - produced);
  return DSP_OK;
}

int launch_stream_roll(float* buf, int64_t B, int64_t ld, int64_t hist, int64_t n_block,
                       hipStream_t s) {
  DSP_REQUIRE(B >= 0 && hist >= 0 && n_block >= 0, "bad sizes");
  if (hist > DSP_STREAM_MAX_HIST)
    return set_error(DSP_ENOTSUP, "history of %lld samples exceeds %d", (long long)hist,
                     DSP_STREAM_MAX_HIST);
  DSP_REQUIRE(ld >= hist + n_block, "leading dimension too small");
  DSP_REQUIRE(B <= INT32_MAX, "batch too large");
  if (B == 0 || hist == 0 || n_block == 0) return DSP_OK;
  DSP_REQUIRE(buf, "null pointer");
  TraceScope trace("stream_roll", s);
  hipLaunchKernelGGL(k_stream_roll, dim3((unsigned)B), dim3(kRollNT), 0, s, buf, ld, (int)hist,
                     n_block);
  DSP_LAUNCHED("k_stream_roll");
  return DSP_OK;
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_stream_version(void) { return 10000; }

int dsp_stream_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const double* sos_host, int32_t S, int32_t clip,
                           const double* zi, double* zf, int64_t ld_state, void* stream) {
  dsp::clear_error();
  return dsp::launch_stream_cascade(x, y, B, n, ld_x, ld_y, sos_host, S, clip, zi, zf, ld_state,
                                    static_cast<hipStream_t>(stream));
}

int dsp_stream_src_geometry(int32_t K, int32_t L, int32_t M, int64_t consumed, int64_t produced,
                            int64_t n_block, int32_t flush, int64_t* hist, int64_t* c_offset,
                            int64_t* n_out) {
  dsp::clear_error();
  return dsp::stream_src_geometry(K, L, M, consumed, produced, n_block, flush, hist, c_offset,
                                  n_out);
}

int dsp_stream_roll_f32(float* buf, int64_t B, int64_t ld, int64_t hist, int64_t n_block,
                        void* stream) {
  dsp::clear_error();
  return dsp::launch_stream_roll(buf, B, ld, hist, n_block, static_cast<hipStream_t>(stream));
}

}  // extern "C"
