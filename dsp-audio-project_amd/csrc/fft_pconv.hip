// Partitioned fast convolution (include/dspcore_partconv.h): a real FIR of up
// to 2^20 taps by uniformly partitioned overlap-save on fft_pass.h's in-LDS
// transforms.  k_fastconv (fft_conv.hip) holds the whole FIR in one transform
// and so stops at N/2 + 1 taps; here the taps are S partitions of P = N/2, an
// input block is transformed once, and an output block is the sum of S
// spectrum products and one inverse transform.
//
// Framing.  N = 2^log2n, V = N/4, P = H = 2 V.  With u the stream at absolute
// positions (`pos` samples precede the call's x[0]; zeros before sample 0) and
// u'[a] = u[a + offset], pair q of a row is Z_q = FFT(z), z[n] = u'[q H - 3 V
// + n] + i u'[q H - 2 V + n]: blocks 2q and 2q + 1 of the same row as real and
// imaginary part, k_fastconv's pairing.  One partition delays by P = H, one
// pair, so the pairing survives the partition sum:
//   W_q = sum_{s < S} Z_(q-s) Hf[s];  D = FFT(conj(W_q)) = conj(N ifft(W_q))
//   y'[q H + m] = Re D[3 V + m],  y'[q H + V + m] = -Im D[3 V + m],  m < V
// (N - V >= P - 1 values of the circular convolution are the linear one's;
// with a delay of one block instead, odd partitions would need the other
// pairing of blocks).  The stream's first pair is floor(-offset / H): the
// samples x[0 .. offset) sit at negative u' positions.
//
// Two launches, because pair q reads spectra that other workgroups write:
//   k_partconv_fwd  per (row, pair): z from (history | row | zeros), the
//     passes in LDS, Z_q to slot q mod slots of the row's ring in HBM; the
//     loader ORs the exponent test of every sample into the pair's flag word.
//     Extra workgroups copy the time-domain history out.
//   k_partconv_mac  per (row, pair): the pass-0 loader is the partition sum,
//     bin n of Z_(q-s) and Hf[s] for s < S in ascending s (pairs before the
//     stream's first skipped), float32 complex; consecutive threads read
//     consecutive bins, 8 bytes each.  Conjugate, passes, the two blocks'
//     outputs inside [0, n_out).
//
// Non-finite input.  A pair with a flagged spectrum among its S loads nothing
// and stores nothing from its passes; its threads write its outputs as direct
// sums over the caller's taps, float32 products in a float64 accumulator, as
// k_fastconv's fallback does.  They read the K - 1 samples before the output
// from (history | row), which is why the stream carries the time-domain
// history as well as the spectra.
#include "fft_conv_common.h"
#include "dspcore_partconv.h"

namespace dsp {
namespace {

struct PcArgs {
  const float* x;
  float* y;
  const float* hist_in;
  float* hist_out;
  const float* taps;
  const float2* hf;
  const float2* tw;
  float2* spec;  // [B][slots][N]
  int* flags;    // [B][slots]
  int64_t B, n_in, ld_x, n_out, ld_y, offset, pos, ld_hist, L, slots;
  int64_t q0;      // the launch's first pair
  int64_t pairs;   // transforms per row in this launch
  int64_t qfirst;  // the stream's first pair
  int K, S;
};

// Sample i (relative to the call's x[0]) of row `row`'s stream: zeros before
// the L samples of history (the first pairs of a stream reach behind them).
using PcRow = ConvRow<true>;

__device__ __forceinline__ PcRow pc_row(const PcArgs& a, int64_t row) {
  return conv_row<true>(a, a.L, row);
}

// Forward: z from memory, Z_q to the ring.
template <int N>
struct PcFwd {
  static constexpr bool kLdsIn = false;
  PcRow r;
  int64_t i0;  // the call-relative index of z[0]'s real part
  const float2* tw;
  float2* out;  // the pair's slot
  int* flag;
  bool live;
  __device__ __forceinline__ const float2* twiddles() const { return tw; }
  __device__ __forceinline__ float2 load(int n) const {
    if (!live) return make_float2(0.f, 0.f);
    const float re = r.at(i0 + n);
    const float im = r.at(i0 + N / 4 + n);
    if (conv_nonfinite(re) || conv_nonfinite(im)) *flag = 1;
    return make_float2(re, im);
  }
  __device__ __forceinline__ void store(int k, float2 v) const {
    if (live) out[k] = v;
  }
};

template <int LOG2N>
__global__ __launch_bounds__(Plan<LOG2N>::NT) void k_partconv_fwd(PcArgs a, unsigned tgroups) {
  using PL = Plan<LOG2N>;
  static_assert(PL::NP >= 2, "the flag is read after a pass barrier");
  constexpr int N = PL::N;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ int s_flag[PL::TPB];
  if (blockIdx.x >= tgroups) {
    conv_copy_history<PL::NT, true>(a, a.L, tgroups);
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
  const int64_t q = a.q0 + (tt - row * a.pairs);
  int64_t slot = q % a.slots;
  if (slot < 0) slot += a.slots;
  const int64_t rs = row * a.slots + slot;
  __syncthreads();  // the flag is cleared before any load sets it
  run_pass<LOG2N, 0, PcFwd<N>, 2>(
      PcFwd<N>{pc_row(a, row), q * (N / 2) - 3 * (N / 4) + a.offset - a.pos, a.tw,
               a.spec + rs * N, &s_flag[tl], live},
      buf, j0, tw);
  // (pass 0's barrier lies between the loads and this read)
  if (live && j0 == 0) a.flags[rs] = s_flag[tl];
}

// Multiply-accumulate and inverse: the loader is the partition sum.
template <int N>
struct PcMac {
  static constexpr bool kLdsIn = false;
  const float2* ring;  // the row's slot 0
  const float2* z0;    // Z_q's slot
  const float2* hf;
  const float2* tw;
  float* y;            // the row's output 0
  int64_t m0;          // output index of the pair's first (may be negative)
  int64_t n_out, slots;
  int ns;              // partitions to sum (0: load nothing)
  bool store_out;
  __device__ __forceinline__ const float2* twiddles() const { return tw; }
  __device__ __forceinline__ float2 load(int n) const {
    float2 acc = make_float2(0.f, 0.f);
    const float2* __restrict__ z = z0 + n;
    const float2* __restrict__ h = hf + n;
    const float2* lo = ring + n;
#pragma unroll 4
    for (int s = 0; s < ns; ++s) {
      const float2 zv = *z, hv = *h;
      acc.x = fmaf(zv.x, hv.x, acc.x);
      acc.x = fmaf(-zv.y, hv.y, acc.x);
      acc.y = fmaf(zv.x, hv.y, acc.y);
      acc.y = fmaf(zv.y, hv.x, acc.y);
      h += N;
      z = z == lo ? lo + (slots - 1) * N : z - N;
    }
    return make_float2(acc.x, -acc.y);
  }
  __device__ __forceinline__ void store(int k, float2 v) const {
    if (!store_out || k < 3 * (N / 4)) return;
    const int64_t m1 = m0 + (k - 3 * (N / 4)), m2 = m1 + N / 4;
    if (m1 >= 0 && m1 < n_out) y[m1] = v.x;
    if (m2 >= 0 && m2 < n_out) y[m2] = -v.y;
  }
};

template <int LOG2N>
__global__ __launch_bounds__(Plan<LOG2N>::NT) void k_partconv_mac(PcArgs a) {
  using PL = Plan<LOG2N>;
  constexpr int N = PL::N;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  __shared__ int s_flag[PL::TPB];
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
  const int64_t q = a.q0 + (tt - row * a.pairs);
  const int64_t have = q - a.qfirst + 1;  // pairs of the stream up to q
  const int ns = (int)(have < a.S ? have : a.S);
  const int64_t slot = q % a.slots;  // q >= 0 where outputs are
  __syncthreads();  // the flag is cleared before any thread sets it
  // a flagged spectrum among the ns (ns <= S <= slots: at most one wrap)
  bool mine = false;
  for (int s = j0; s < ns; s += PL::TPT) {
    const int64_t sl = slot - s < 0 ? slot - s + a.slots : slot - s;
    mine |= a.flags[row * a.slots + sl] != 0;
  }
  if (mine && live) s_flag[tl] = 1;
  __syncthreads();
  const bool bad = s_flag[tl] != 0;
  const bool fft = live && !bad;
  const float2* ring = a.spec + row * a.slots * N;
  const int64_t m0 = q * (N / 2) - a.pos;
  float* y = a.y + row * a.ld_y;
  run_pass<LOG2N, 0, PcMac<N>, 2>(
      PcMac<N>{ring, ring + slot * N, a.hf, a.tw, y, m0, a.n_out, a.slots, fft ? ns : 0, fft},
      buf, j0, tw);
  if (!live || !bad) return;
  // the flagged pair's outputs, directly (no barrier from here on)
  const PcRow r = pc_row(a, row);
  for (int m = j0; m < N / 2; m += PL::TPT) {
    const int64_t mo = m0 + m;
    if (mo >= 0 && mo < a.n_out) conv_direct(y + mo, r, a.taps, a.K, mo + a.offset);
  }
}

constexpr int kPcMinLog2 = 6;

template <int LOG2N>
int launch_fwd_n(const PcArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N>;
  const int64_t transforms = a.B * a.pairs;
  const int64_t tg = ceil_div(transforms, PL::TPB);
  const int64_t cg = conv_hist_groups(a.hist_out, a.B, a.L, PL::NT);
  DSP_REQUIRE(tg + cg <= INT32_MAX, "too many blocks in one call");
  if (tg + cg == 0) return DSP_OK;
  TraceScope trace("partconv_fwd", s);
  return launch_lds_resident<PL>(k_partconv_fwd<LOG2N>, "k_partconv_fwd", transforms, cg, s, a,
                                 (unsigned)tg);
}

template <int LOG2N>
int launch_mac_n(const PcArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N>;
  const int64_t transforms = a.B * a.pairs;
  DSP_REQUIRE(ceil_div(transforms, PL::TPB) <= INT32_MAX, "too many blocks in one call");
  if (transforms == 0) return DSP_OK;
  TraceScope trace("partconv_mac", s);
  return launch_lds_resident<PL>(k_partconv_mac<LOG2N>, "k_partconv_mac", transforms, 0, s, a);
}

int launch_fwd(const PcArgs& a, int log2n, hipStream_t s) {
  return dispatch_log2n<kPcMinLog2, DSP_MAX_LOG2N>(
      log2n, [&](auto lg) { return launch_fwd_n<decltype(lg)::value>(a, s); });
}
int launch_mac(const PcArgs& a, int log2n, hipStream_t s) {
  return dispatch_log2n<kPcMinLog2, DSP_MAX_LOG2N>(
      log2n, [&](auto lg) { return launch_mac_n<decltype(lg)::value>(a, s); });
}

inline int64_t floor_div(int64_t a, int64_t b) {  // b > 0
  return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// K and log2n of every entry point; S through *S_out.
int pc_geometry(int K, int log2n, int64_t* S_out) {
  if (log2n < kPcMinLog2 || log2n > DSP_MAX_LOG2N)
    return set_error(DSP_ENOTSUP, "log2n=%d outside [%d, %d]", log2n, kPcMinLog2, DSP_MAX_LOG2N);
  DSP_REQUIRE(K >= 1 && K <= DSP_PARTCONV_MAX_TAPS, "K=%d outside [1, %d]", K,
              DSP_PARTCONV_MAX_TAPS);
  const int64_t P = int64_t(1) << (log2n - 1);
  const int64_t S = ceil_div(K, P);
  DSP_REQUIRE(S <= DSP_PARTCONV_MAX_PARTS, "K=%d taps are %lld partitions of %lld, above %d", K,
              (long long)S, (long long)P, DSP_PARTCONV_MAX_PARTS);
  *S_out = S;
  return DSP_OK;
}

int partconv_log2n(int K) {
  DSP_REQUIRE(K >= 1 && K <= DSP_PARTCONV_MAX_TAPS, "K=%d outside [1, %d]", K,
              DSP_PARTCONV_MAX_TAPS);
  int lg = kPcMinLog2;
  while (lg < DSP_MAX_LOG2N && (int64_t(1) << (lg - 1)) < K) ++lg;
  return lg;
}

size_t workspace_bytes(int64_t B, int log2n, int64_t slots) {
  const size_t per = (size_t(8) << log2n) + sizeof(int);
  return mul_sat((size_t)B, (size_t)slots, per);
}

int check_ring(int64_t B, int log2n, void* ws, size_t ws_bytes, int64_t slots, int64_t need,
               const float* twiddles) {
  DSP_REQUIRE(slots >= need, "slots=%lld < the %lld pairs this call touches", (long long)slots,
              (long long)need);
  DSP_REQUIRE(slots <= (int64_t(1) << 30), "slots=%lld > 2^30", (long long)slots);
  DSP_REQUIRE(ws && twiddles, "null pointer");
  DSP_REQUIRE(ws_bytes >= workspace_bytes(B, log2n, slots), "ws_bytes=%zu < %zu", ws_bytes,
              workspace_bytes(B, log2n, slots));
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(twiddles) & 7) == 0,
              "ws must be 16-byte and twiddles 8-byte aligned");
  return DSP_OK;
}

int partconv(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x, int64_t n_out,
             int64_t ld_y, int64_t offset, int64_t pos, const float* hist_in, float* hist_out,
             int64_t ld_hist, const float* taps, int K, const float* hf, int log2n, void* ws,
             size_t ws_bytes, int64_t slots, const float* twiddles, hipStream_t s) {
  int64_t S = 0;
  if (int rc = pc_geometry(K, log2n, &S)) return rc;
  const int64_t N = int64_t(1) << log2n, H = N / 2, L = S * H + 3 * (N / 4);
  if (int rc = conv_check_io(x, y, B, n_in, ld_x, n_out, ld_y, offset, hist_in, hist_out, ld_hist,
                             L, K))
    return rc;
  DSP_REQUIRE(pos >= 0 && pos <= (int64_t(1) << 40), "pos=%lld outside [0, 2^40]", (long long)pos);
  DSP_REQUIRE(hist_in || pos == 0, "pos=%lld > 0 without hist_in", (long long)pos);
  DSP_REQUIRE(slots >= 1, "slots=%lld < 1", (long long)slots);
  // pairs: the stream's first; the first not complete before the call; the
  // outputs' first and last; the last to transform (the outputs' last, or
  // the last that this call completes)
  const int64_t qfirst = floor_div(-offset, H);
  const int64_t qf_lo = floor_div(pos - offset, H);
  const int64_t qo_lo = pos / H;
  const int64_t qo_hi = n_out > 0 ? ceil_div(pos + n_out, H) - 1 : qo_lo - 1;
  const int64_t qdone = floor_div(pos + n_in - offset, H) - 1;
  const int64_t qf_hi = n_out > 0 && qo_hi > qdone ? qo_hi : qdone;  // >= qf_lo - 1
  int64_t lo = qf_lo;
  if (n_out > 0) {
    const int64_t back = qo_lo - S + 1 > qfirst ? qo_lo - S + 1 : qfirst;
    lo = back < lo ? back : lo;
  }
  const int64_t need = qf_hi >= lo ? qf_hi - lo + 1 : 0;
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(taps && hf, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(hf) & 7) == 0, "hf must be 8-byte aligned");
  if (int rc = check_ring(B, log2n, ws, ws_bytes, slots, need, twiddles)) return rc;
  PcArgs a{x, y, pos > 0 ? hist_in : nullptr, hist_out, taps,
           reinterpret_cast<const float2*>(hf), reinterpret_cast<const float2*>(twiddles),
           static_cast<float2*>(ws),
           reinterpret_cast<int*>(static_cast<char*>(ws) + (size_t)B * slots * N * sizeof(float2)),
           B, n_in, ld_x, n_out, ld_y, offset, pos, ld_hist, L, slots, qf_lo, qf_hi - qf_lo + 1,
           qfirst, K, (int)S};
  if (int rc = launch_fwd(a, log2n, s)) return rc;
  a.q0 = qo_lo;
  a.pairs = qo_hi - qo_lo + 1;
  return launch_mac(a, log2n, s);
}

int partconv_prime(const float* hist, int64_t B, int64_t ld_hist, int64_t pos, int K, int log2n,
                   void* ws, size_t ws_bytes, int64_t slots, const float* twiddles, hipStream_t s) {
  int64_t S = 0;
  if (int rc = pc_geometry(K, log2n, &S)) return rc;
  const int64_t N = int64_t(1) << log2n, H = N / 2, L = S * H + 3 * (N / 4);
  DSP_REQUIRE(B >= 0, "negative count B=%lld", (long long)B);
  DSP_REQUIRE(pos >= 0 && pos <= (int64_t(1) << 40), "pos=%lld outside [0, 2^40]", (long long)pos);
  DSP_REQUIRE(ld_hist >= L, "ld_hist=%lld < %lld", (long long)ld_hist, (long long)L);
  DSP_REQUIRE(slots >= 1, "slots=%lld < 1", (long long)slots);
  const int64_t qp = pos / H;
  const int64_t lo = qp - S + 1 > 0 ? qp - S + 1 : 0;
  const int64_t pairs = qp - lo;  // lo .. qp - 1
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(hist, "null hist");
  DSP_REQUIRE(B <= (int64_t(1) << 40) / ld_hist, "batch too large");
  if (int rc = check_ring(B, log2n, ws, ws_bytes, slots, pairs, twiddles)) return rc;
  if (pairs == 0) return DSP_OK;
  const PcArgs a{nullptr, nullptr, hist, nullptr, nullptr, nullptr,
                 reinterpret_cast<const float2*>(twiddles), static_cast<float2*>(ws),
                 reinterpret_cast<int*>(static_cast<char*>(ws) +
                                        (size_t)B * slots * N * sizeof(float2)),
                 B, 0, 0, 0, 0, 0, pos, ld_hist, L, slots, lo, pairs, 0, K, (int)S};
  return launch_fwd(a, log2n, s);
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_partconv_version(void) { return 10000; }

int dsp_partconv_log2n(int32_t K) {
  dsp::clear_error();
  return dsp::partconv_log2n(K);
}

int64_t dsp_partconv_hist_len(int32_t K, int32_t log2n) {
  dsp::clear_error();
  int64_t S = 0;
  if (int rc = dsp::pc_geometry(K, log2n, &S)) return rc;
  return S * (int64_t(1) << (log2n - 1)) + 3 * (int64_t(1) << (log2n - 2));
}

int64_t dsp_partconv_slots(int32_t K, int32_t log2n, int64_t n, int64_t offset) {
  dsp::clear_error();
  int64_t S = 0;
  if (int rc = dsp::pc_geometry(K, log2n, &S)) return rc;
  if (n < 0 || n > (int64_t(1) << 41) || offset < 0 || offset > K - 1)
    return dsp::set_error(DSP_EINVAL, "n=%lld or offset=%lld out of range", (long long)n,
                          (long long)offset);
  return S + dsp::ceil_div(n + offset, int64_t(1) << (log2n - 1)) + 1;
}

size_t dsp_partconv_workspace_bytes(int64_t B, int32_t log2n, int64_t slots) {
  dsp::clear_error();
  if (B < 0 || slots < 0 || log2n < dsp::kPcMinLog2 || log2n > DSP_MAX_LOG2N) {
    dsp::set_error(DSP_EINVAL, "B=%lld slots=%lld log2n=%d", (long long)B, (long long)slots, log2n);
    return 0;
  }
  return dsp::workspace_bytes(B, log2n, slots);
}

int dsp_partconv_f32(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x,
                     int64_t n_out, int64_t ld_y, int64_t offset, int64_t pos,
                     const float* hist_in, float* hist_out, int64_t ld_hist, const float* taps,
                     int32_t K, const float* hf, int32_t log2n, void* ws, size_t ws_bytes,
                     int64_t slots, const float* twiddles, void* stream) {
  dsp::clear_error();
  return dsp::partconv(x, y, B, n_in, ld_x, n_out, ld_y, offset, pos, hist_in, hist_out, ld_hist,
                       taps, K, hf, log2n, ws, ws_bytes, slots, twiddles,
                       static_cast<hipStream_t>(stream));
}

int dsp_partconv_prime_f32(const float* hist, int64_t B, int64_t ld_hist, int64_t pos, int32_t K,
                           int32_t log2n, void* ws, size_t ws_bytes, int64_t slots,
                           const float* twiddles, void* stream) {
  dsp::clear_error();
  return dsp::partconv_prime(hist, B, ld_hist, pos, K, log2n, ws, ws_bytes, slots, twiddles,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
