// What fast convolution (fft_conv.hip) and partitioned fast convolution
// (fft_pconv.hip) share over fft_pass.h: the (history | row | zeros) view of a
// stream, the non-finite test behind the per-transform LDS flag, the history
// copy of the extra workgroups, the flagged transform's direct sum, and the
// host checks of the arguments both entry points take.
#pragma once

#include "fft_pass.h"

namespace dsp {
namespace {

// Sample i (relative to the call's x[0]) of one row's stream: h[i] for i < 0,
// the history (nullptr: zeros), x[i] below n_in, zeros from there on.  BOUNDED:
// the history holds L samples and zeros precede it; otherwise no index below
// -L is ever asked for (and L is not read).
template <bool BOUNDED>
struct ConvRow {
  const float* x;  // the row's sample 0
  const float* h;
  int64_t n_in, L;
  __device__ __forceinline__ float at(int64_t i) const {
    return i < 0 ? (h && (!BOUNDED || i >= -L) ? h[i] : 0.f) : (i < n_in ? x[i] : 0.f);
  }
};

// Row `row` of a.x [B][ld_x] behind a.hist_in [B][ld_hist], L samples each (a:
// either unit's kernel arguments).
template <bool BOUNDED, class Args>
__device__ __forceinline__ ConvRow<BOUNDED> conv_row(const Args& a, int64_t L, int64_t row) {
  return ConvRow<BOUNDED>{a.x + row * a.ld_x,
                          a.hist_in ? a.hist_in + row * a.ld_hist + L : nullptr, a.n_in, L};
}

__device__ __forceinline__ bool conv_nonfinite(float v) {
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}

// The history workgroups, blockIdx.x >= first, of NT threads each: element e =
// (row, j) of a.hist_out [B][ld_hist] is sample n_in - L + j of row's stream.
template <int NT, bool BOUNDED, class Args>
__device__ __forceinline__ void conv_copy_history(const Args& a, int64_t L, unsigned first) {
  const int64_t total = a.B * L;
  const int64_t step = (int64_t)(gridDim.x - first) * NT;
  for (int64_t e = (int64_t)(blockIdx.x - first) * NT + threadIdx.x; e < total; e += step) {
    const int64_t row = e / L, j = e - row * L;
    a.hist_out[row * a.ld_hist + j] = conv_row<BOUNDED>(a, L, row).at(a.n_in - L + j);
  }
}

// A flagged transform's output, directly: sum_t taps[t] r[i0 - t], float32
// products in a float64 accumulator.
template <class Row>
__device__ __forceinline__ void conv_direct(float* y, const Row& r, const float* taps, int K,
                                            int64_t i0) {
  double acc = 0.0;
#pragma unroll 1
  for (int tp = 0; tp < K; ++tp) acc = fma((double)taps[tp], (double)r.at(i0 - tp), acc);
  *y = (float)acc;
}

// Workgroups that copy B rows of L history samples, NT threads each: at most
// 1024, the copy is grid-strided; none without a hist_out.
inline int64_t conv_hist_groups(const float* hist_out, int64_t B, int64_t L, int NT) {
  if (!hist_out || L <= 0) return 0;
  const int64_t cg = ceil_div(B * L, 4 * NT);
  return cg < 1 ? 1 : (cg > 1024 ? 1024 : cg);
}

// Whether [p, p + n) and [q, q + m) floats share a byte.
inline bool floats_overlap(const float* p, int64_t n, const float* q, int64_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return n > 0 && m > 0 && a < b + 4 * (uintptr_t)m && b < a + 4 * (uintptr_t)n;
}

// The checks of x, y, the counts and the histories that dsp_fastconv_f32 and
// dsp_partconv_f32 share (each has checked K against its own limits first);
// need: the samples of a history row.  Nothing is dereferenced; the buffers are looked at only when
// B > 0, so that B == 0 passes with null pointers.
inline int conv_check_io(const float* x, const float* y, int64_t B, int64_t n_in, int64_t ld_x,
                         int64_t n_out, int64_t ld_y, int64_t offset, const float* hist_in,
                         const float* hist_out, int64_t ld_hist, int64_t need, int K) {
  DSP_REQUIRE(K >= 1, "K=%d < 1", K);
  DSP_REQUIRE(B >= 0 && n_in >= 0 && n_out >= 0, "negative count B=%lld n_in=%lld n_out=%lld",
              (long long)B, (long long)n_in, (long long)n_out);
  DSP_REQUIRE(offset >= 0 && offset <= K - 1, "offset=%lld outside [0, K - 1 = %d]",
              (long long)offset, K - 1);
  DSP_REQUIRE(n_in <= (int64_t(1) << 40), "n_in=%lld > 2^40", (long long)n_in);
  DSP_REQUIRE(n_out <= n_in + (K - 1) - offset, "n_out=%lld > n_in + K - 1 - offset = %lld",
              (long long)n_out, (long long)(n_in + (K - 1) - offset));
  DSP_REQUIRE(ld_x >= n_in && ld_y >= n_out, "leading dimension too small (ld_x=%lld ld_y=%lld)",
              (long long)ld_x, (long long)ld_y);
  DSP_REQUIRE((!hist_in && !hist_out) || ld_hist >= need, "ld_hist=%lld < %lld",
              (long long)ld_hist, (long long)need);
  DSP_REQUIRE(hist_in != hist_out || !hist_in, "hist_in and hist_out are one buffer");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(x || n_in == 0, "null x");
  DSP_REQUIRE(y || n_out == 0, "null y");
  const int64_t ld = ld_x > ld_y ? ld_x : ld_y;
  DSP_REQUIRE(B <= (int64_t(1) << 40) / (ld > 1 ? ld : 1), "batch too large");
  DSP_REQUIRE(!floats_overlap(x, (B - 1) * ld_x + n_in, y, (B - 1) * ld_y + n_out),
              "x and y overlap");
  return DSP_OK;
}

}  // namespace
}  // namespace dsp
