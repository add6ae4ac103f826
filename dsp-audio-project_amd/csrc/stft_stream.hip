// Streaming STFT magnitude (include/dspcore_stspec.h): the framing of a stream
// cut into blocks, the argument checks and the two launches of a push -- the
// frames with the carry update (k_stft_stream, over fft_pass.h's pass code),
// then the non-finite repair (fft_nf.hip) over the same two-source rows.
//
// Framing.  Frame f of a channel is s[f hop, f hop + N) of its stream s.  With
// `seen` samples so far, F(seen) = 0 for seen < N, else 1 + (seen - N) div hop
// frames are complete, and the seen - F(seen) hop < N samples from which frame
// F(seen) starts are the carry.  A push of n samples emits frames F(seen) ..
// F(seen + n) - 1 from the virtual row [carry | block], whose position 0 is
// stream position F(seen) hop.  The flush emits what design.stft_plan(total)
// still owes: one zero-padded frame when total < N or (total - N) mod hop != 0,
// else none; the frames of all calls are stft_plan(total).frames.
//
// The kernel.  The frames that one push completes, and the carry the next push
// starts from, in one launch.  Transform workgroups (blockIdx.x < tgroups) are
// k_spec_real's scheme (fft.hip): transform t = (row, frame) packs its N real
// samples as N/2 complex, pass 0 reads memory, the other passes run in LDS,
// the real split gives |X[k]|.  Only pass 0's loader differs: sample i of frame
// f is position f * hop + i of the virtual row [carry_in[row][0:carry_len] |
// block[row][0:n_block]], zero past its end (the flush's zero padding).  A pair
// that lies in one source at an 8-byte aligned address is one float2 load, any
// other pair two guarded scalar loads: the same values, so a frame's bits do
// not depend on how the stream was cut into blocks.
//
// Carry workgroups (the remaining blockIdx.x) copy row[frames * hop + j],
// j < carry_out_len, into carry_out, a buffer no workgroup of the launch
// reads.  A push is a handful of frames per channel and launch-bound, so the
// persistent prefetching kernels of fft_spec.hip (tuned for batches that fill
// the chip) are not the model here.  Non-finite input is repaired by a second
// launch (fft_nf.hip, two-source nf_input), as for dsp_stft_mag_f32.
#include "fft_pass.h"
#include "dspcore_stspec.h"

namespace dsp {
namespace {

// One launch's arguments; stspec_mag below has checked everything.
struct StspecArgs {
  const float* carry_in;
  float* carry_out;
  const float* block;
  float* mag;
  int64_t ld_carry, ld_block, ld_mag;
  int64_t B, frames, hop;
  int64_t carry_len, n_block, carry_out_len;
  const float* win;
  const float* tw;
};

template <int NH>
struct StreamSpecIO {
  static constexpr bool kLdsIn = false;
  const float* c;    // the frame's sample 0 in carry_in's row (valid for i < nc)
  const float* b;    // the frame's sample 0 in block's row (valid for nc <= i < nv)
  const float* win;
  float2* buf;
  int nc, nv;        // samples of the frame in the carry / in the row, 0 <= nc <= nv <= N
  bool live, pc, pb, pw;  // 8-byte alignment of c, b and win
  __device__ __forceinline__ float sample(int i) const {
    return i < nc ? c[i] : (i < nv ? b[i] : 0.f);
  }
  __device__ __forceinline__ float2 load(int n) const {
    if (!live) return make_float2(0.f, 0.f);
    const int i = 2 * n;
    float2 sv;
    if (pc && i + 1 < nc) {
      sv = *reinterpret_cast<const float2*>(c + i);
    } else if (pb && i >= nc && i + 1 < nv) {
      sv = *reinterpret_cast<const float2*>(b + i);
    } else {
      sv = make_float2(sample(i), sample(i + 1));
    }
    const float2 wv = pw ? reinterpret_cast<const float2*>(win)[n] : make_float2(win[i], win[i + 1]);
    return make_float2(sv.x * wv.x, sv.y * wv.y);
  }
  __device__ __forceinline__ void store(int k, float2 v) const { buf[lpad(k)] = v; }
};

template <int LOG2N>  // LOG2N of the real length N
__global__ __launch_bounds__(Plan<LOG2N - 1>::NT) void k_stft_stream(StspecArgs a,
                                                                      unsigned tgroups) {
  using PL = Plan<LOG2N - 1>;
  constexpr int N = 1 << LOG2N, NH = N / 2;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  if (blockIdx.x >= tgroups) {
    // carry update: element e = (row, j) of carry_out from the virtual row
    const int64_t total = a.B * a.carry_out_len;
    const int64_t start = a.frames * a.hop;
    const int64_t step = (int64_t)(gridDim.x - tgroups) * PL::NT;
    for (int64_t e = (int64_t)(blockIdx.x - tgroups) * PL::NT + threadIdx.x; e < total; e += step) {
      const int64_t row = e / a.carry_out_len, j = e - row * a.carry_out_len;
      const int64_t p = start + j;
      a.carry_out[row * a.ld_carry + j] = p < a.carry_len
                                              ? a.carry_in[row * a.ld_carry + p]
                                              : a.block[row * a.ld_block + (p - a.carry_len)];
    }
    return;
  }
  const int tl = threadIdx.x / PL::TPT;
  const int j0 = threadIdx.x - tl * PL::TPT;
  const int64_t t = (int64_t)blockIdx.x * PL::TPB + tl;
  const bool live = t < a.B * a.frames;
  float2* buf = lds + tl * PL::PADN;
  const float2* twt = reinterpret_cast<const float2*>(a.tw);
  Tw<LOG2N - 1, 0> tw;
  load_tw<LOG2N - 1, 0>(tw, twt, j0, 2);
  const int64_t tt = live ? t : 0;
  const int64_t row = a.frames == 1 ? tt : tt / a.frames;
  const int64_t f0 = (tt - row * a.frames) * a.hop;  // the frame's start in the virtual row
  const int64_t ncl = a.carry_len - f0, nvl = a.carry_len + a.n_block - f0;
  const int nc = (int)(ncl < 0 ? 0 : (ncl > N ? N : ncl));
  const int nv = (int)(nvl < nc ? nc : (nvl > N ? N : nvl));
  // (pointers to the frame's sample 0 in either source; each is dereferenced
  // only at the indices that lie inside its source)
  const float* c = a.carry_in + (row * a.ld_carry + f0);
  const float* b = a.block + (row * a.ld_block + (f0 - a.carry_len));
  const StreamSpecIO<NH> io{c, b, a.win, buf, nc, nv, live,
                            (reinterpret_cast<uintptr_t>(c) & 7) == 0,
                            (reinterpret_cast<uintptr_t>(b) & 7) == 0,
                            (reinterpret_cast<uintptr_t>(a.win) & 7) == 0};
  run_pass<LOG2N - 1, 0>(io, buf, j0, tw);
  __syncthreads();  // the last pass stored Z into LDS
  if (!live) return;
  real_split_mag<NH, PL::TPT>(buf, twt, a.mag + t * a.ld_mag, j0);
}

constexpr int64_t kStspecCarryGroups = 1024;  // at most; the copy is grid-strided

template <int LOG2N>
int launch_stft_stream_n(const StspecArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N - 1>;
  const int64_t tg = ceil_div(a.B * a.frames, PL::TPB);
  int64_t cg = ceil_div(a.B * a.carry_out_len, 4 * PL::NT);
  cg = cg < 1 ? 1 : (cg > kStspecCarryGroups ? kStspecCarryGroups : cg);
  DSP_REQUIRE(tg + cg <= INT32_MAX, "too many frames in one call");
  return launch_lds_resident<PL>(k_stft_stream<LOG2N>, "k_stft_stream", a.B * a.frames, cg, s, a,
                                 (unsigned)tg);
}

constexpr int kStspecMinLog2 = 5;

int launch_stft_stream(const StspecArgs& a, int log2n, hipStream_t s) {
  return dispatch_log2n<kStspecMinLog2, DSP_MAX_LOG2N>(
      log2n, [&](auto lg) { return launch_stft_stream_n<decltype(lg)::value>(a, s); });
}

constexpr int64_t kStspecMaxBlock = int64_t(1) << 30;

int64_t frames_complete(int64_t seen, int64_t N, int64_t hop) {
  return seen < N ? 0 : 1 + (seen - N) / hop;
}

int stspec_geometry(int log2n, int64_t hop, int64_t seen, int64_t n_block, int flush,
                    int64_t* carry_len, int64_t* frames, int64_t* carry_out_len) {
  DSP_REQUIRE(log2n >= 0 && log2n <= DSP_MAX_LOG2N_FOURSTEP, "log2n=%d outside [0, %d]", log2n,
              DSP_MAX_LOG2N_FOURSTEP);
  const int64_t N = int64_t(1) << log2n;
  DSP_REQUIRE(hop >= 1 && hop <= N, "hop=%lld outside [1, n_fft=%lld]", (long long)hop,
              (long long)N);
  DSP_REQUIRE(seen >= 0 && n_block >= 0, "negative count seen=%lld n_block=%lld", (long long)seen,
              (long long)n_block);
  DSP_REQUIRE(n_block <= kStspecMaxBlock, "n_block=%lld > 2^30", (long long)n_block);
  DSP_REQUIRE(seen <= INT64_MAX - kStspecMaxBlock, "seen=%lld too large", (long long)seen);
  DSP_REQUIRE(!flush || n_block == 0, "a flush takes no block (n_block=%lld)", (long long)n_block);
  const int64_t f_in = frames_complete(seen, N, hop);
  const int64_t cl = seen - f_in * hop;
  int64_t fr, col;
  if (flush) {
    fr = (seen < N || (seen - N) % hop != 0) ? 1 : 0;
    col = 0;
  } else {
    fr = frames_complete(seen + n_block, N, hop) - f_in;
    col = cl + n_block - fr * hop;
  }
  if (carry_len) *carry_len = cl;
  if (frames) *frames = fr;
  if (carry_out_len) *carry_out_len = col;
  return DSP_OK;
}

int stspec_mag(const float* carry_in, float* carry_out, int64_t ld_carry, const float* block,
               int64_t ld_block, int64_t n_block, float* mag, int64_t ld_mag, int64_t B,
               int log2n, int64_t hop, int64_t seen, int flush, const float* window,
               const float* twiddles, hipStream_t s) {
  if (log2n < kStspecMinLog2 || log2n > DSP_MAX_LOG2N)
    return set_error(DSP_ENOTSUP, "log2n=%d outside [%d, %d]", log2n, kStspecMinLog2,
                     DSP_MAX_LOG2N);
  const int64_t N = int64_t(1) << log2n;
  int64_t carry_len, frames, carry_out_len;
  if (int rc = stspec_geometry(log2n, hop, seen, n_block, flush, &carry_len, &frames,
                               &carry_out_len))
    return rc;
  DSP_REQUIRE(B >= 0, "B=%lld", (long long)B);
  DSP_REQUIRE(ld_carry >= N - 1, "ld_carry=%lld < n_fft - 1", (long long)ld_carry);
  DSP_REQUIRE(ld_mag >= N / 2 + 1, "ld_mag=%lld < n_fft / 2 + 1", (long long)ld_mag);
  DSP_REQUIRE(ld_block >= n_block, "ld_block=%lld < n_block=%lld", (long long)ld_block,
              (long long)n_block);
  DSP_REQUIRE(carry_in != carry_out || !carry_in, "carry_in and carry_out are one buffer");
  if (B == 0) return DSP_OK;
  DSP_REQUIRE(carry_out && window && twiddles, "null pointer");
  DSP_REQUIRE(carry_in || carry_len == 0, "null carry_in with %lld carried samples",
              (long long)carry_len);
  DSP_REQUIRE(block || n_block == 0, "null block");
  DSP_REQUIRE(mag || frames == 0, "null mag");
  DSP_REQUIRE(B <= (INT64_MAX >> 16) / (frames > 0 ? frames : 1), "too many frames");
  const StspecArgs a{carry_in, carry_out, block, mag, ld_carry, ld_block, ld_mag, B, frames, hop,
                     carry_len, n_block, carry_out_len, window, twiddles};
  {
    TraceScope trace("stspec", s);
    if (int rc = launch_stft_stream(a, log2n, s)) return rc;
  }
  // carry_in, block and mag are intact: the repair reads what the transform read
  TraceScope trace("stspec_nf", s);
  NfArgs nf{carry_in, mag, B * frames, ld_carry, ld_mag, 0, carry_len + n_block, hop, frames,
            window, twiddles, 2, log2n};
  nf.in2 = block ? block : carry_out;  // (never read when n_block == 0; non-null marks the form)
  nf.ld_in2 = ld_block;
  nf.split = carry_len;
  return launch_nf_small(nf, s);
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_stspec_version(void) { return 10000; }

int dsp_stspec_geometry(int32_t log2n, int64_t hop, int64_t seen, int64_t n_block, int32_t flush,
                        int64_t* carry_len, int64_t* frames, int64_t* carry_out_len) {
  dsp::clear_error();
  return dsp::stspec_geometry(log2n, hop, seen, n_block, flush, carry_len, frames, carry_out_len);
}

int dsp_stspec_mag_f32(const float* carry_in, float* carry_out, int64_t ld_carry,
                       const float* block, int64_t ld_block, int64_t n_block, float* mag,
                       int64_t ld_mag, int64_t B, int32_t log2n, int64_t hop, int64_t seen,
                       int32_t flush, const float* window, const float* twiddles, void* stream) {
  dsp::clear_error();
  return dsp::stspec_mag(carry_in, carry_out, ld_carry, block, ld_block, n_block, mag, ld_mag, B,
                         log2n, hop, seen, flush, window, twiddles,
                         static_cast<hipStream_t>(stream));
}

}  // extern "C"
