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
#include "fft_pass.h"
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

// Sample i >= -(K - 1) of row `row`'s stream.
struct FcRow {
  const float* x;  // the row's sample 0
  const float* h;  // h[i], i < 0: the history (nullptr: zeros)
  int64_t n_in;
  __device__ __forceinline__ float at(int64_t i) const {
    return i < 0 ? (h ? h[i] : 0.f) : (i < n_in ? x[i] : 0.f);
  }
};

__device__ __forceinline__ FcRow fc_row(const FcArgs& a, int64_t row) {
  return FcRow{a.x + row * a.ld_x,
               a.hist_in ? a.hist_in + row * a.ld_hist + (a.K - 1) : nullptr, a.n_in};
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

__device__ __forceinline__ bool fc_nonfinite(float v) {
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
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
    if (fc_nonfinite(re) || fc_nonfinite(im)) *flag = 1;
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
    // history update: element e = (row, j) of hist_out
    const int64_t k1 = a.K - 1;
    const int64_t total = a.B * k1;
    const int64_t step = (int64_t)(gridDim.x - tgroups) * PL::NT;
    for (int64_t e = (int64_t)(blockIdx.x - tgroups) * PL::NT + threadIdx.x; e < total; e += step) {
      const int64_t row = e / k1, j = e - row * k1;
      a.hist_out[row * a.ld_hist + j] = fc_row(a, row).at(a.n_in - k1 + j);
    }
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
  for (int m = j0; m < n1 + n2; m += PL::TPT) {
    const int64_t i0 = m0 + m + a.offset;
    double acc = 0.0;
#pragma unroll 1
    for (int tp = 0; tp < a.K; ++tp) acc = fma((double)a.taps[tp], (double)r.at(i0 - tp), acc);
    y[m] = (float)acc;
  }
}

constexpr int64_t kFcHistGroups = 1024;  // at most; the copy is grid-strided
constexpr int kFcMinLog2 = 6;
constexpr int kFcMaxTaps = (1 << (DSP_MAX_LOG2N - 1)) + 1;

template <int LOG2N>
int launch_fastconv_n(const FcArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N>;
  const int64_t transforms = a.B * a.pairs;
  const int64_t tg = ceil_div(transforms, PL::TPB);
  int64_t cg = 0;
  if (a.hist_out && a.K > 1) {
    cg = ceil_div(a.B * (a.K - 1), 4 * PL::NT);
    cg = cg < 1 ? 1 : (cg > kFcHistGroups ? kFcHistGroups : cg);
  }
  DSP_REQUIRE(tg + cg <= INT32_MAX, "too many blocks in one call");
  if (tg + cg == 0) return DSP_OK;
  return launch_lds_resident<PL>(k_fastconv<LOG2N>, "k_fastconv", transforms, cg, s, a,
                                 (unsigned)tg);
}

int launch_fastconv(const FcArgs& a, int log2n, hipStream_t s) {
  switch (log2n) {
    case 6: return launch_fastconv_n<6>(a, s);
    case 7: return launch_fastconv_n<7>(a, s);
    case 8: return launch_fastconv_n<8>(a, s);
    case 9: return launch_fastconv_n<9>(a, s);
    case 10: return launch_fastconv_n<10>(a, s);
    case 11: return launch_fastconv_n<11>(a, s);
    case 12: return launch_fastconv_n<12>(a, s);
    case 13: return launch_fastconv_n<13>(a, s);
    case 14: return launch_fastconv_n<14>(a, s);
    default: return set_error(DSP_ENOTSUP, "log2n=%d outside [6, 14]", log2n);
  }
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

// Whether [p, p + n) and [q, q + m) floats share a byte.
bool fc_overlap(const float* p, int64_t n, const float* q, int64_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return n > 0 && m > 0 && a < b + 4 * (uintptr_t)m && b < a + 4 * (uintptr_t)n;
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
  DSP_REQUIRE(B >= 0 && n_in >= 0 && n_out >= 0, "negative count B=%lld n_in=%lld n_out=%lld",
              (long long)B, (long long)n_in, (long long)n_out);
  DSP_REQUIRE(offset >= 0 && offset <= K - 1, "offset=%lld outside [0, K - 1 = %d]",
              (long long)offset, K - 1);
  DSP_REQUIRE(n_in <= (int64_t(1) << 40), "n_in=%lld > 2^40", (long long)n_in);
  DSP_REQUIRE(n_out <= n_in + (K - 1) - offset, "n_out=%lld > n_in + K - 1 - offset = %lld",
              (long long)n_out, (long long)(n_in + (K - 1) - offset));
  DSP_REQUIRE(ld_x >= n_in && ld_y >= n_out, "leading dimension too small (ld_x=%lld ld_y=%lld)",
              (long long)ld_x, (long long)ld_y);
  DSP_REQUIRE((!hist_in && !hist_out) || ld_hist >= K - 1, "ld_hist=%lld < K - 1 = %d",
              (long long)ld_hist, K - 1);
  DSP_REQUIRE(hist_in != hist_out || !hist_in, "hist_in and hist_out are one buffer");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(taps && hf && twiddles, "null pointer");
  DSP_REQUIRE(x || n_in == 0, "null x");
  DSP_REQUIRE(y || n_out == 0, "null y");
  DSP_REQUIRE(B <= (int64_t(1) << 40) / (ld_x > ld_y ? (ld_x > 1 ? ld_x : 1) : (ld_y > 1 ? ld_y : 1)),
              "batch too large");
  DSP_REQUIRE(!fc_overlap(x, (B - 1) * ld_x + n_in, y, (B - 1) * ld_y + n_out),
              "x and y overlap");
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
