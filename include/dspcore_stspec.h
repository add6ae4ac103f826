/*
 * dspcore_stspec.h — stream spectrum of libdspcore.so: the windowed magnitude
 * spectrogram (dsp_stft_mag_f32's recipe: multiply a frame by the caller's
 * window, FFT, |X[k]| for k <= N/2) of a stream that arrives in blocks, frame
 * by frame as the samples come in.
 *
 * Conventions are dspcore.h's: data pointers are device pointers owned by the
 * caller, `stream` is a hipStream_t, the launches are asynchronous on it
 * (nothing synchronises or allocates, so a call is graph-capturable), 0 on
 * success or a negative DSP_E* code with the thread-local dsp_last_error
 * string.  This header versions on its own (dsp_stspec_version); dspcore.h,
 * dsp_version and the stream, bank and live-EQ headers are unchanged by it.
 *
 * Framing.  N = 2^log2n, 1 <= hop <= N.  Frame f of a channel is samples
 * [f hop, f hop + N) of its stream.  With `seen` samples so far,
 *     F(seen) = 0 for seen < N, else 1 + (seen - N) div hop
 * frames are complete.  A call with n_block samples emits frames F(seen) ..
 * F(seen + n_block) - 1 (at most 1 + (n_block - 1) div hop of them) and
 * carries the seen + n_block - F(seen + n_block) hop < N samples from which
 * the next frame starts.  The flush call (flush != 0, n_block == 0) emits the
 * zero-padded frame that the one-shot framing of the whole stream (1 +
 * ceil(max(0, total - N) / hop) frames) still owes: one frame when total < N
 * or (total - N) mod hop != 0, an empty stream included, else none.
 *
 * Use: two carry buffers [B][ld_carry >= N - 1] that swap roles after every
 * call (the call reads carry_in and writes carry_out; their contents before
 * the first call do not matter, seen == 0 carries nothing), a mag buffer for
 * the most frames a block can emit, the window and twiddle tables of
 * dsp_stft_mag_f32.  Keep `seen` on the host and add n_block after each call.
 */
#ifndef DSPCORE_STSPEC_H
#define DSPCORE_STSPEC_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_stspec_version(void);

/* ---------------------------------------------------------------------------
 * HOST, no device work.  For a call after `seen` samples with a block of
 * n_block samples (or the flush): *carry_len = the samples carried into it,
 * *frames = the frames it emits, *carry_out_len = the samples it carries out
 * (0 after a flush).  Any of the three pointers may be NULL.  log2n may be
 * 0 .. DSP_MAX_LOG2N_FOURSTEP here (the arithmetic has no size limit of its
 * own; dsp_stspec_mag_f32 takes 5 .. DSP_MAX_LOG2N).
 *
 * DSP_EINVAL: log2n outside that range, hop < 1 or hop > N, a negative count,
 * n_block > 2^30, flush with n_block != 0.
 * ------------------------------------------------------------------------- */
int dsp_stspec_geometry(int32_t log2n, int64_t hop, int64_t seen, int64_t n_block, int32_t flush,
                        int64_t* carry_len, int64_t* frames, int64_t* carry_out_len);

/* ---------------------------------------------------------------------------
 * The frames that the block completes, for B channels:
 *     mag[(b * frames + f) * ld_mag + k] = |FFT_N(window * frame f of row b)[k]|,
 * k <= N/2, f < frames (dsp_stspec_geometry's count for this call; the layout
 * is dsp_stft_mag_f32's), where row b is the concatenation
 *     carry_in[b * ld_carry + 0 .. carry_len) | block[b * ld_block + 0 .. n_block)
 * read as zeros past its end (only a flush frame reaches there), and frame f
 * starts f * hop samples into it.  Then carry_out[b * ld_carry + j], j <
 * carry_out_len, takes the row's samples from frames * hop on.  After every
 * successful call with B > 0 the carry is in carry_out -- also for n_block ==
 * 0 and for calls that emit no frame.  Elements of carry_out from
 * carry_out_len on, the padding of mag rows and both inputs are left as they
 * are.
 *
 * carry_in and carry_out are distinct buffers (no workgroup reads what
 * another writes); ld_carry >= N - 1; ld_mag >= N/2 + 1; ld_block >= n_block.
 * Rows of `block` may start at any 4-byte alignment (a view into a larger
 * buffer): aligned pairs are read as 8 bytes, others sample by sample, the
 * values and therefore the frames' bits are the same either way.  `window` is
 * float32 [N], `twiddles` float32 pairs exp(-2 pi i k / N), k < N/2, both as
 * for dsp_stft_mag_f32.
 *
 * Launches: one for the frames and the carry (trace name "stspec"), then the
 * non-finite repair of dsp_stft_mag_f32 over the same rows ("stspec_nf"),
 * which reads |X[0]| of every frame of this call and exits at once when all
 * are finite: a frame that holds an inf or NaN gets the reference's classes
 * (every bin +inf or NaN), frames that do not are untouched.
 *
 * DSP_ENOTSUP: log2n outside 5 .. DSP_MAX_LOG2N.  DSP_EINVAL: hop < 1 or
 * hop > N, a negative count, n_block > 2^30, flush with n_block != 0,
 * ld_carry < N - 1, ld_mag < N/2 + 1, ld_block < n_block, carry_in ==
 * carry_out, a null pointer where one is read or written.  The checks come
 * before any device work; B == 0 launches nothing.
 * ------------------------------------------------------------------------- */
int dsp_stspec_mag_f32(const float* carry_in, float* carry_out, int64_t ld_carry,
                       const float* block, int64_t ld_block, int64_t n_block,
                       float* mag, int64_t ld_mag, int64_t B, int32_t log2n, int64_t hop,
                       int64_t seen, int32_t flush, const float* window, const float* twiddles,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_STSPEC_H */
