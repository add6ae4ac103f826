// Fast convolution (include/dspcore_fastconv.h): a long real FIR by
// overlap-save on fft_pass.h's in-LDS transforms, k_bluestein's shape
// (fft_dft.hip): forward FFT -> pointwise product -> conjugate -> forward FFT
// -> conjugate, all in one padded LDS buffer per transform.
//
// Framing.  N = 2^log2n, K taps, V = N - (K - 1).  Block p of a row gives its
// outputs [p V, p V + V) from the row's stream s (history before index 0,
// zeros from n_in on) at s[p V + offset - (K - 1) + n], n < N: the circular
// convolution's values n >= K - 1 are the linear one's.  Transform t = (row,
// pair q) carries blocks 2q and 2q + 1 of that row as z = x1 + i x2; the taps
// are real, so conv(z, h) = conv(x1, h) + i conv(x2, h) and no split follows:
//   A = FFT(z);  C = conj(A * Hf);  D = FFT(C) = conj(N ifft(A Hf))
//   y[2q V + n - (K-1)] = Re D[n],  y[(2q+1) V + n - (K-1)] = -Im D[n].
// A row's last odd block pairs with zeros; rows never pair with each other, so
// a row's bits depend on nothing but the row.
//
// Twiddles.  The passes form w_r = w1^r from table values only (fft_pass.h,
// TWMODE 2): powering from w1 alone, as the spectra's kernels do inside their
// 1e-5 tolerance, multiplies w1's rounding error by r and came to 1.04 of this
// header's bound at N = 16384 on an MI355X; with w2, w4, w8 from the table the
// worst case of the tests is 0.44 of it.
//
// Loads are one sample at a time (rows at any 4-byte alignment give the same
// values, hence the same bits); consecutive threads read consecutive samples.
// The re-read of the K - 1 overlap is served by L2.
//
// Non-finite input, in the same launch: pass 0's loader ORs the exponent test
// of every sample it loads into one LDS word per transform.  A flagged
// transform runs its passes like any other (the barriers are workgroup-wide)
// but stores nothing from them; its threads then write its outputs as direct
// sums over the caller's taps, float32 products in a float64 accumulator --
// the class (finite, +-inf, NaN) of np.convolve's float64 sum over each
// output's own window, and finite values good to one float32 rounding.
//
// History workgroups (the blockIdx.x after the transforms') copy the last
// K - 1 samples of (history | row) into hist_out, a buffer nothing in the
// launch reads.
#include "fft_conv_common.h"
#include "dspcore_fastconv.h"

namespace dsp {
namespace {

struct FcArgs {
  const float* x;
  float* y;
  const float* hist_in;
  float* hist_out;
  const float* taps;
  const float2* hf;
  const float2* tw;
  int64_t B, n_in, ld_x, n_out, ld_y, offset, ld_hist;
  int64_t pairs;  // transforms per row
  int K, V;
};

// Sample i >= -(K - 1) of row `row`'s stream: nothing reads further back.
using FcRow = ConvRow<false>;

__device__ __forceinline__ FcRow fc_row(const FcArgs& a, int64_t row) {
  return conv_row<false>(a, a.K - 1, row);
}

// The N samples of one block: n < nc from the history, n < nv from x, then 0.
struct FcWin {
  const float* c;  // c[n], n < nc (nullptr: zeros)
  const float* b;  // b[n], nc <= n < nv
  int nc, nv;
  __device__ __forceinline__ float at(int n) const {
    return n < nc ? (c ? c[n] : 0.f) : (n < nv ? b[n] : 0.f);
  }
};

template <int N>
__device__ __forceinline__ FcWin fc_win(const FcRow& r, int64_t s0) {
  const int64_t ncl = -s0, nvl = r.n_in - s0;
  const int nc = (int)(ncl < 0 ? 0 : (ncl > N ? N : ncl));
  const int nv = (int)(nvl < nc ? nc : (nvl > N ? N : nvl));
  return FcWin{r.h ? r.h + s0 : nullptr, r.x + s0, nc, nv};
}

// Stage 1: z from memory, C = conj(A * Hf) into LDS.
template <int N>
struct FcStage1 {
  static constexpr bool kLdsIn = false;
  FcWin w1, w2;
  const float2* hf;
  const float2* tw;
  float2* buf;
  int* flag;
  bool live, second;
  __device__ __forceinline__ const float2* twiddles() const { return tw; }
  __device__ __forceinline__ float2 load(int n) const {
    if (!live) return make_float2(0.f, 0.f);
    const float re = w1.at(n);
    const float im = second ? w2.at(n) : 0.f;
    if (conv_nonfinite(re) || conv_nonfinite(im)) *flag = 1;
    return make_float2(re, im);
  }
  __device__ __forceinline__ void store(int k, float2 v) const {
    const float2 c = cmul(v, hf[k]);
    buf[lpad(k)] = make_float2(c.x, -c.y);
  }
};

// Stage 2: D = FFT(C); the valid outputs of both blocks below n_out.
template <int N>
struct FcStage2 {
  static constexpr bool kLdsIn = true;
  float2* buf;
  const float2* tw;
  float* y;    // the pair's output 0 (block 2q's first)
  int k1, V;   // k1 = K - 1
  int n1, n2;  // outputs to store of block 2q, of block 2q + 1 (0 .. V)
  __device__ __forceinline__ const float2* twiddles() const { return tw; }
  __device__ __forceinline__ float2 load(int j) const { return buf[lpad(j)]; }
  __device__ __forceinline__ void store(int k, float2 v) const {
    const int m = k - k1;
    if (m < 0) return;
    if (m < n1) y[m] = v.x;
    if (m < n2) y[V + m] = -v.y;
  }
};

template <int LOG2N>
__global__ __launch_bounds__(Plan<LOG2N>::NT) void k_fastconv(FcArgs a, unsigned tgroups) {
  using PL = Plan<LOG2N>;
  static_assert(PL::NP >= 2, "the flag is read after a pass barrier");
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ int s_flag[PL::TPB];
  if (blockIdx.x >= tgroups) {
    conv_copy_history<PL::NT, false>(a, a.K - 1, tgroups);
    return;
  }
  const int tl = threadIdx.x / PL::TPT;
  const int j0 = threadIdx.x - tl * PL::TPT;
  const int64_t t = (int64_t)blockIdx.x * PL::TPB + tl;
  const bool live = t < a.B * a.pairs;
  float2* buf = lds + tl * PL::PADN;
  if (j0 == 0) s_flag[tl] = 0;
  Tw<LOG2N, 0> tw;
  load_tw<LOG2N, 0>(tw, a.tw, j0);
  const int64_t tt = live ? t : 0;
  const int64_t row = a.pairs == 1 ? tt : tt / a.pairs;
  const int64_t m0 = (tt - row * a.pairs) * 2 * a.V;  // the pair's first output
  const int64_t rem = a.n_out - m0;                   // >= 1 for a live transform
  const int n1 = (int)(rem < a.V ? rem : a.V);
  const int n2 = (int)(rem - a.V < 0 ? 0 : (rem - a.V < a.V ? rem - a.V : a.V));
  const FcRow r = fc_row(a, row);
  const int64_t s0 = m0 + a.offset - (a.K - 1);  // the stream index of block 2q's sample 0
  __syncthreads();  // the flag is cleared before any load sets it
  run_pass<LOG2N, 0, FcStage1<PL::N>, 2>(
      FcStage1<PL::N>{fc_win<PL::N>(r, s0), fc_win<PL::N>(r, s0 + a.V), a.hf, a.tw, buf,
                      &s_flag[tl], live, n2 > 0},
      buf, j0, tw);
  __syncthreads();  // stage 1's last pass wrote LDS
  const bool bad = s_flag[tl] != 0;
  float* y = a.y + row * a.ld_y + m0;
  const bool fft_out = live && !bad;
  run_pass<LOG2N, 0, FcStage2<PL::N>, 2>(
      FcStage2<PL::N>{buf, a.tw, y, a.K - 1, a.V, fft_out ? n1 : 0, fft_out ? n2 : 0}, buf, j0, tw);
  if (!live || !bad) return;
  // the flagged transform's outputs, directly (no barrier from here on)
  for (int m = j0; m < n1 + n2; m += PL::TPT)
    conv_direct(y + m, r, a.taps, a.K, m0 + m + a.offset);
}

constexpr int kFcMinLog2 = 6;
constexpr int kFcMaxTaps = (1 << (DSP_MAX_LOG2N - 1)) + 1;

template <int LOG2N>
int launch_fastconv_n(const FcArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N>;
  const int64_t transforms = a.B * a.pairs;
  const int64_t tg = ceil_div(transforms, PL::TPB);
  const int64_t cg = conv_hist_groups(a.hist_out, a.B, a.K - 1, PL::NT);
  DSP_REQUIRE(tg + cg <= INT32_MAX, "too many blocks in one call");
  if (tg + cg == 0) return DSP_OK;
  return launch_lds_resident<PL>(k_fastconv<LOG2N>, "k_fastconv", transforms, cg, s, a,
                                 (unsigned)tg);
}

int launch_fastconv(const FcArgs& a, int log2n, hipStream_t s) {
  return dispatch_log2n<kFcMinLog2, DSP_MAX_LOG2N>(
      log2n, [&](auto lg) { return launch_fastconv_n<decltype(lg)::value>(a, s); });
}

int fastconv_log2n(int K) {
  DSP_REQUIRE(K >= 1, "K=%d < 1", K);
  if (K > kFcMaxTaps)
    return set_error(DSP_ENOTSUP, "K=%d above %d taps (one 2^%d-point transform)", K, kFcMaxTaps,
                     DSP_MAX_LOG2N);
  int lg = kFcMinLog2;
  while (lg < DSP_MAX_LOG2N && (int64_t(1) << lg) < 4 * (int64_t)(K - 1)) ++lg;
  return lg;
}

int fastconv(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x, int64_t n_out,
             int64_t ld_y, int64_t offset, const float* hist_in, float* hist_out, int64_t ld_hist,
             const float* taps, int K, const float* hf, int log2n, const float* twiddles,
             hipStream_t s) {
  if (log2n < kFcMinLog2 || log2n > DSP_MAX_LOG2N)
    return set_error(DSP_ENOTSUP, "log2n=%d outside [%d, %d]", log2n, kFcMinLog2, DSP_MAX_LOG2N);
  const int64_t N = int64_t(1) << log2n;
  DSP_REQUIRE(K >= 1 && K <= N / 2 + 1, "K=%d outside [1, n_fft / 2 + 1 = %lld]", K,
              (long long)(N / 2 + 1));
  if (int rc = conv_check_io(x, y, B, n_in, ld_x, n_out, ld_y, offset, hist_in, hist_out, ld_hist,
                             K - 1, K))
    return rc;
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(taps && hf && twiddles, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(hf) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(twiddles) & 7) == 0,
              "hf and twiddles must be 8-byte aligned");
  const int64_t V = N - (K - 1);
  const int64_t pairs = ceil_div(n_out, 2 * V);
  const FcArgs a{x, y, hist_in, hist_out, taps, reinterpret_cast<const float2*>(hf),
                 reinterpret_cast<const float2*>(twiddles), B, n_in, ld_x, n_out, ld_y, offset,
                 ld_hist, pairs, K, (int)V};
  TraceScope trace("fastconv", s);
  return launch_fastconv(a, log2n, s);
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_fastconv_version(void) { return 10000; }

int dsp_fastconv_log2n(int32_t K) {
  dsp::clear_error();
  return dsp::fastconv_log2n(K);
}

int dsp_fastconv_f32(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x,
                     int64_t n_out, int64_t ld_y, int64_t offset, const float* hist_in,
                     float* hist_out, int64_t ld_hist, const float* taps, int32_t K,
                     const float* hf, int32_t log2n, const float* twiddles, void* stream) {
  dsp::clear_error();
  return dsp::fastconv(x, y, B, n_in, ld_x, n_out, ld_y, offset, hist_in, hist_out, ld_hist, taps,
                       K, hf, log2n, twiddles, static_cast<hipStream_t>(stream));
}

}  // extern "C"
