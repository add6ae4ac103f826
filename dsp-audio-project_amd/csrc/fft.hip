// Batched FFT and windowed magnitude spectrum for gfx950: the in-LDS Stockham
// transform (k_fft) and real-input spectrum (k_spec_real) up to 2^14 points, the
// tables that say which kernel serves which size, and the family's host entry
// points.  fft_pass.h is the pass code (algorithm, LDS layout, twiddles),
// fft_spec.hip the persistent spectrum kernels, fft_large.hip the four-step.
//
// Replaces reference modules/dsp_core.py:41-66 (fft_diezmado_en_tiempo, a
// recursive radix-2 DIT in pure Python: 2N-1 calls, each building exp(-2j*pi*k/N)
// and concatenating E + W*O, E - W*O) and dsp_core.py:74-98
// (calcular_espectro_magnitud: centre segment or zero-padded input, Hann window,
// FFT, |X[k]| for k <= N/2).  The DFT it computes is the same (natural-order
// X[k] = sum_n x[n] W_N^(nk)); only the factorisation differs.
#include "fft_pass.h"

namespace dsp {
namespace {


template <int LOG2N, int MODE>
__global__ __launch_bounds__(Plan<LOG2N>::NT) void k_fft(FftArgs a) {
  using PL = Plan<LOG2N>;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int tl = threadIdx.x / PL::TPT;
  const int j0 = threadIdx.x - tl * PL::TPT;
  const int64_t t = (int64_t)blockIdx.x * PL::TPB + tl;
  const bool live = t < a.B;
  const GlobalIO<MODE, PL::N> io{a, in_row<MODE>(a, live ? t : 0), t, live};
  if constexpr (PL::NP == 0) {
    io.store(0, io.load(0));
  } else {
    Tw<LOG2N, 0> tw;
    load_tw<LOG2N, 0>(tw, a.tw, j0);
    run_pass<LOG2N, 0>(io, lds + tl * PL::PADN, j0, tw);
  }
}

// Real-input magnitude spectrum (spectrum / STFT mode, N >= 32): the N real
// samples are packed as N/2 complex z[n] = x[2n] + i x[2n+1] (window applied),
// one N/2-point Stockham transform Z runs in LDS, and the split (real_split_mag)
// gives |X[k]| for every k <= N/2: half the butterflies and half the LDS of the
// complex transform.
template <int NH>  // NH = N/2, the complex transform's size
struct RealSpecIO {
  static constexpr bool kLdsIn = false;
  const FftArgs& a;
  InRow ir;
  float2* buf;
  bool live;
  bool pairs;  // the frame's samples start 8-byte aligned: one float2 load per pair
  __device__ __forceinline__ float2 load(int n) const {
    if (!live) return make_float2(0.f, 0.f);
    const int i = 2 * n;
    if (pairs && i + 1 < ir.valid) {
      const float2 sv = *reinterpret_cast<const float2*>(a.in + ir.base + i);
      const float2 wv = reinterpret_cast<const float2*>(a.win)[n];
      return make_float2(sv.x * wv.x, sv.y * wv.y);
    }
    const float s0 = (i < ir.valid) ? a.in[ir.base + i] : 0.f;
    const float s1 = (i + 1 < ir.valid) ? a.in[ir.base + i + 1] : 0.f;
    return make_float2(s0 * a.win[i], s1 * a.win[i + 1]);
  }
  __device__ __forceinline__ void store(int k, float2 v) const { buf[lpad(k)] = v; }
};

template <int LOG2N>  // LOG2N of the real length N
__global__ __launch_bounds__(Plan<LOG2N - 1>::NT) void k_spec_real(FftArgs a) {
  using PL = Plan<LOG2N - 1>;
  constexpr int N = 1 << LOG2N, NH = N / 2;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const int tl = threadIdx.x / PL::TPT;
  const int j0 = threadIdx.x - tl * PL::TPT;
  const int64_t t = (int64_t)blockIdx.x * PL::TPB + tl;
  const bool live = t < a.B;
  float2* buf = lds + tl * PL::PADN;
  Tw<LOG2N - 1, 0> tw;
  load_tw<LOG2N - 1, 0>(tw, a.tw, j0, 2);
  const InRow ir = in_row<kSpec>(a, live ? t : 0);
  const bool pairs = ((reinterpret_cast<uintptr_t>(a.in + ir.base) & 7) == 0) &&
                     ((reinterpret_cast<uintptr_t>(a.win) & 7) == 0);
  run_pass<LOG2N - 1, 0>(RealSpecIO<NH>{a, ir, buf, live, pairs}, buf, j0, tw);
  __syncthreads();  // the last pass stored Z into LDS
  if (!live) return;
  real_split_mag<NH, PL::TPT>(buf, a.tw, a.out + t * a.ld_out, j0);
}

template <int LOG2N>
int launch_spec_real(const FftArgs& a, hipStream_t s) {
  return launch_lds_resident<Plan<LOG2N - 1>>(k_spec_real<LOG2N>, "k_spec_real", a.B, 0, s, a);
}

template <int MODE, int LOG2N>
int launch_one(const FftArgs& a, hipStream_t s) {
  return launch_lds_resident<Plan<LOG2N>>(k_fft<LOG2N, MODE>, "k_fft", a.B, 0, s, a);
}

template <int MODE>
int dispatch(const FftArgs& a, int log2n, hipStream_t s) {
  if (log2n < 0 || log2n > DSP_MAX_LOG2N)
    return set_error(DSP_EINVAL, "log2n=%d outside [0, %d]", log2n, DSP_MAX_LOG2N);
  return dispatch_log2n<0, DSP_MAX_LOG2N>(
      log2n, [&](auto lg) { return launch_one<MODE, decltype(lg)::value>(a, s); });
}

// The spectrum and the STFT: below 32 points the complex transform, then the
// real-input kernels -- k_spec_real where the packed transform's first pass has
// radix 16, fft_spec.hip's streaming kernel where it is smaller, one wave at 4096.
int dispatch_spec(const FftArgs& a, int log2n, hipStream_t s) {
  switch (log2n) {
    case 0: return launch_one<kSpec, 0>(a, s);
    case 1: return launch_one<kSpec, 1>(a, s);
    case 2: return launch_one<kSpec, 2>(a, s);
    case 3: return launch_one<kSpec, 3>(a, s);
    case 4: return launch_one<kSpec, 4>(a, s);
    case 5: return launch_spec_real<5>(a, s);
    case 9: return launch_spec_real<9>(a, s);
    case 13: return launch_spec_real<13>(a, s);
    case 6: case 7: case 8: case 10: case 11: case 14: return launch_spec_stream(a, log2n, s);
    case 12: return launch_spec_wave12(a, s);
    default: return set_error(DSP_EINVAL, "log2n=%d outside [0, %d]", log2n, DSP_MAX_LOG2N);
  }
}

}  // namespace

int launch_spectrum(const float* x, float* mag, int64_t B, int64_t ld_x,
                    int64_t seg_start, int64_t seg_len, int log2n,
                    int64_t ld_mag, const float* window, const float* tw,
                    void* ws, size_t ws_bytes, hipStream_t s, bool repair) {
  if (log2n > DSP_MAX_LOG2N) {
    DSP_REQUIRE(log2n <= DSP_MAX_LOG2N_FOURSTEP, "log2n=%d outside [0, %d]", log2n,
                DSP_MAX_LOG2N_FOURSTEP);
    const int64_t N = int64_t(1) << log2n;
    DSP_REQUIRE(B >= 0 && seg_start >= 0 && seg_len >= 0 && seg_len <= N,
                "bad segment start=%lld len=%lld (N=%lld)", (long long)seg_start,
                (long long)seg_len, (long long)N);
    DSP_REQUIRE(ld_mag >= N / 2 + 1, "ld_mag too small");
    DSP_REQUIRE(ld_x >= seg_start + seg_len, "segment exceeds the row");
    if (B == 0) return DSP_OK;
    DSP_REQUIRE(x && mag && window && tw, "null pointer");
    FftArgs a{x, mag, B, ld_x, ld_mag, seg_start, seg_len, 0, 1, window,
              reinterpret_cast<const float2*>(tw)};
    TraceScope trace("spectrum", s);
    return run_fft4(a, kSpec, log2n, ws, ws_bytes, s);
  }
  return launch_stft(x, mag, B, ld_x, seg_start, seg_len, 0, 1, log2n, ld_mag, window, tw, s,
                     repair);
}

int launch_stft(const float* x, float* mag, int64_t B, int64_t ld_x, int64_t seg_start,
                int64_t seg_len, int64_t hop, int64_t frames, int log2n, int64_t ld_mag,
                const float* window, const float* tw, hipStream_t s, bool repair) {
  DSP_REQUIRE(log2n >= 0 && log2n <= DSP_MAX_LOG2N, "log2n=%d outside [0, %d]", log2n,
              DSP_MAX_LOG2N);
  const int64_t N = int64_t(1) << log2n;
  DSP_REQUIRE(frames >= 1 && hop >= 0 && (frames == 1 || hop >= 1), "bad framing hop=%lld "
              "frames=%lld", (long long)hop, (long long)frames);
  DSP_REQUIRE(B >= 0 && seg_start >= 0 && seg_len >= 0 && (frames > 1 || seg_len <= N),
              "bad segment start=%lld len=%lld (N=%lld)", (long long)seg_start,
              (long long)seg_len, (long long)N);
  DSP_REQUIRE(ld_mag >= N / 2 + 1, "ld_mag too small");
  DSP_REQUIRE(ld_x >= seg_start + seg_len, "segment exceeds the row");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(x && mag && window && tw, "null pointer");
  DSP_REQUIRE(B <= INT64_MAX / frames, "too many frames");
  FftArgs a{x, mag, B * frames, ld_x, ld_mag, seg_start, seg_len, hop, frames, window,
            reinterpret_cast<const float2*>(tw)};
  {
    TraceScope trace(frames == 1 ? "spectrum" : "stft", s);
    if (int rc = dispatch_spec(a, log2n, s)) return rc;
  }
  if (!repair) return DSP_OK;
  TraceScope trace("spectrum_nf", s);
  return launch_nf_small(NfArgs{x, mag, B * frames, ld_x, ld_mag, seg_start, seg_len, hop, frames,
                                window, tw, kSpec, log2n},
                         s);
}

int launch_fft(const float* in, float* out, int64_t B, int log2n, int real_in,
               int64_t ld_in, int64_t ld_out, const float* tw, void* ws, size_t ws_bytes,
               hipStream_t s) {
  DSP_REQUIRE(log2n >= 0 && log2n <= DSP_MAX_LOG2N_FFT, "log2n=%d outside [0, %d]", log2n,
              DSP_MAX_LOG2N_FFT);
  const int64_t N = int64_t(1) << log2n;
  DSP_REQUIRE(B >= 0 && ld_in >= N && ld_out >= N, "bad sizes");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(in && out && tw, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                  (real_in || (reinterpret_cast<uintptr_t>(in) & 7) == 0),
              "complex buffers must be 8-byte aligned");
  if (fft_takes_split(log2n))  // above one four-step transform (fft_split.hip)
    return launch_fft_split(in, out, B, log2n, real_in, ld_in, ld_out, tw, ws, ws_bytes, s);
  FftArgs a{in, out, B, ld_in, ld_out, 0, 0, 0, 1, nullptr, reinterpret_cast<const float2*>(tw)};
  if (log2n > DSP_MAX_LOG2N) {
    TraceScope trace("fft", s);
    return run_fft4(a, real_in ? kR2C : kC2C, log2n, ws, ws_bytes, s);
  }
  {
    TraceScope trace("fft", s);
    if (int rc = real_in ? dispatch<kR2C>(a, log2n, s) : dispatch<kC2C>(a, log2n, s)) return rc;
  }
  TraceScope trace("fft_nf", s);
  return launch_nf_small(NfArgs{in, out, B, ld_in, ld_out, 0, 0, 0, 1, nullptr, tw,
                                real_in ? kR2C : kC2C, log2n},
                         s);
}

}  // namespace dsp
