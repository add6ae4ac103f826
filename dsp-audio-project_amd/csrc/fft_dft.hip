// Any-length DFT by Bluestein's chirp-z identity (for app.py:322-324, whose
// np.fft.fft segments have length int(1024 * L/M), e.g. 1114 = 2 * 557):
//   w[k] = exp(-i pi k^2 / n),  X[k] = w[k] * sum_j (x[j] w[j]) conj(w[k-j]),
// a circular convolution of length M = 2^m >= 2n - 1 done as two M-point
// Stockham transforms in one workgroup's LDS:
//   A = FFT(x w, zero-padded);  D = FFT(conj(A * Bf));  X[k] = w[k] conj(D[k])
// with Bf = FFT(b)/M, b[j] = b[M-j] = conj(w[j]) (j < n), from the host in
// float64 (rounded to float32).  The 1/M of the inverse transform is in Bf.
#include "fft_pass.h"

namespace dsp {
namespace {

struct BluArgs {
  const float* in;   // real rows or interleaved complex rows
  float* out;        // interleaved complex rows, n values
  int64_t B, n, ld_in, ld_out;
  int real_in;
  const float2* chirp;  // w[k], k < n
  const float2* bf;     // FFT_M(b) / M
  const float2* tw;     // exp(-2 pi i k / M), k < M/2
};

template <int N>
struct BluStage1 {
  static constexpr bool kLdsIn = false;
  const BluArgs& a;
  float2* buf;
  int64_t t;
  bool live;
  __device__ __forceinline__ float2 load(int j) const {
    if (!live || j >= a.n) return make_float2(0.f, 0.f);
    const float2 x = a.real_in ? make_float2(a.in[t * a.ld_in + j], 0.f)
                               : reinterpret_cast<const float2*>(a.in)[t * a.ld_in + j];
    return cmul(x, a.chirp[j]);
  }
  __device__ __forceinline__ void store(int k, float2 v) const {
    const float2 c = cmul(v, a.bf[k]);
    buf[lpad(k)] = make_float2(c.x, -c.y);
  }
};

template <int N>
struct BluStage2 {
  static constexpr bool kLdsIn = true;
  const BluArgs& a;
  float2* buf;
  int64_t t;
  bool live;
  __device__ __forceinline__ float2 load(int j) const { return buf[lpad(j)]; }
  __device__ __forceinline__ void store(int k, float2 v) const {
    if (live && k < a.n)
      reinterpret_cast<float2*>(a.out)[t * a.ld_out + k] =
          cmul(make_float2(v.x, -v.y), a.chirp[k]);
  }
};

template <int LOG2N>
__global__ __launch_bounds__(Plan<LOG2N>::NT) void k_bluestein(BluArgs a) {
  using PL = Plan<LOG2N>;
  static_assert(PL::NP >= 1, "Bluestein needs M >= 2");
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int tl = threadIdx.x / PL::TPT;
  const int j0 = threadIdx.x - tl * PL::TPT;
  const int64_t t = (int64_t)blockIdx.x * PL::TPB + tl;
  const bool live = t < a.B;
  float2* buf = lds + tl * PL::PADN;
  Tw<LOG2N, 0> tw;
  load_tw<LOG2N, 0>(tw, a.tw, j0);
  run_pass<LOG2N, 0>(BluStage1<PL::N>{a, buf, t, live}, buf, j0, tw);
  __syncthreads();  // stage 1's last pass wrote LDS
  run_pass<LOG2N, 0>(BluStage2<PL::N>{a, buf, t, live}, buf, j0, tw);
}

template <int LOG2N>
int launch_blu(const BluArgs& a, hipStream_t s) {
  return launch_lds_resident<Plan<LOG2N>>(k_bluestein<LOG2N>, "k_bluestein", a.B, 0, s, a);
}

}  // namespace

int bluestein_log2m(int64_t n) {
  int m = 1;
  while ((int64_t(1) << m) < 2 * n - 1) ++m;
  return m;
}

int launch_dft(const float* in, float* out, int64_t B, int64_t n, int real_in, int64_t ld_in,
               int64_t ld_out, const float* chirp, const float* chirp_fft, const float* tw_m,
               hipStream_t s) {
  DSP_REQUIRE(n >= 1 && n <= DSP_MAX_DFT, "n=%lld outside [1, %d]", (long long)n, DSP_MAX_DFT);
  DSP_REQUIRE(B >= 0 && ld_in >= n && ld_out >= n, "bad sizes");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(in && out && chirp && chirp_fft && tw_m, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                  (real_in || (reinterpret_cast<uintptr_t>(in) & 7) == 0),
              "complex buffers must be 8-byte aligned");
  BluArgs a{in, out, B, n, ld_in, ld_out, real_in, reinterpret_cast<const float2*>(chirp),
            reinterpret_cast<const float2*>(chirp_fft), reinterpret_cast<const float2*>(tw_m)};
  TraceScope trace("dft", s);
  const int lg2m = bluestein_log2m(n);
  if (lg2m > DSP_MAX_LOG2N)
    return set_error(DSP_EINVAL, "no Bluestein size for n=%lld", (long long)n);
  return dispatch_log2n<1, DSP_MAX_LOG2N>(
      lg2m, [&](auto lg) { return launch_blu<decltype(lg)::value>(a, s); });
}

}  // namespace dsp
