// Streaming STFT magnitude (include/dspcore_stspec.h): the framing of a stream
// cut into blocks, the argument checks and the two launches of a push -- the
// frames with the carry update (k_stft_stream, at the end of fft.hip beside the
// FFT pass code it shares with k_spec_real), then the non-finite repair
// (fft_nf.hip) over the same two-source rows.
//
// Framing.  Frame f of a channel is s[f hop, f hop + N) of its stream s.  With
// `seen` samples so far, F(seen) = 0 for seen < N, else 1 + (seen - N) div hop
// frames are complete, and the seen - F(seen) hop < N samples from which frame
// F(seen) starts are the carry.  A push of n samples emits frames F(seen) ..
// F(seen + n) - 1 from the virtual row [carry | block], whose position 0 is
// stream position F(seen) hop.  The flush emits what design.stft_plan(total)
// still owes: one zero-padded frame when total < N or (total - N) mod hop != 0,
// else none; the frames of all calls are stft_plan(total).frames.
#include "common.h"
#include "dspcore_stspec.h"

namespace dsp {
namespace {

constexpr int kStspecMinLog2 = 5;
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
