/*
 * dspcore_stream.h — streaming entry points of libdspcore.so: the SRC -> EQ
 * chain block by block, for a live input or a signal longer than device
 * memory.  The one-shot entry points (dspcore.h) process whole rows from rest;
 * these carry the SRC's input history and the EQ's filter state from one
 * block call to the next, so that the concatenated block outputs are the
 * one-shot outputs of the concatenated input.
 *
 * Conventions are dspcore.h's: device pointers owned by the caller, `stream`
 * a hipStream_t, every launch asynchronous on it (nothing synchronises, so the
 * calls are graph-capturable), 0 on success or a negative DSP_E* code with the
 * thread-local dsp_last_error string.  This header versions on its own
 * (dsp_stream_version); dspcore.h and dsp_version are unchanged by it.
 *
 * One block of a stream is three launches:
 *   1. dsp_src_polyphase_f32 (dspcore.h, unchanged) on the staging row
 *      [hist samples of history | block] with the n_in / c_offset / n_out that
 *      dsp_stream_src_geometry names;
 *   2. dsp_stream_cascade_f32 on the SRC's output, entry state = the previous
 *      block's exit state;
 *   3. dsp_stream_roll_f32, which moves the staging row's last hist samples to
 *      its front for the next block.
 */
#ifndef DSPCORE_STREAM_H
#define DSPCORE_STREAM_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_STREAM_MAX_STAGES 8  /* biquad stages per dsp_stream_cascade_f32 call */
#define DSP_STREAM_MAX_HIST 4096 /* SRC history samples per row (ceil(K/L) - 1)   */

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_stream_version(void);

/* ---------------------------------------------------------------------------
 * Biquad cascade with entry and exit state: z = clip(cascade(x)) for [B][n]
 * float32 rows, started from the state `zi` and leaving the state after
 * exactly n samples in `zf`.  Filtering a row in blocks, each block's zf given
 * to the next as zi, gives the one-shot cascade of the whole row (the same
 * float64 recursion; the results differ by float64 rounding only, because the
 * chunking below follows the block and not the row).
 *
 * `sos_host` is a HOST array [S][5] = {b0, b1, b2, a1, a2} per stage, a0 == 1,
 * float64, 0 <= S <= DSP_STREAM_MAX_STAGES (more: DSP_ENOTSUP).  Coefficients
 * and state are float64 inside the kernel, I/O is float32.
 *
 * State.  zi and zf are DEVICE float64 [B][ld_state], ld_state >= 2S.  Row b
 * holds the delay lines of the kernels' own realisation of the cascade, direct
 * form II per stage, in the order (w1_0, w2_0, w1_1, w2_1, ...):
 *     u *= G;  per stage k:  w = u - a1 w1_k - a2 w2_k
 *                            u = g w + c1 w1_k + c2 w2_k;  w2_k = w1_k; w1_k = w
 * with g = 1, c = (b1, b2) / b0, G = prod b0 when every b0 != 0, and g = b0,
 * c = (b1, b2), G = 1 otherwise (csrc/cascade.h, dspcore/design.py:
 * state_space).  It is NOT scipy's direct-form-II-transposed `zi`, and a state
 * is valid only for the `sos` that produced it: start a new cascade from rest.
 * Coefficients that change mid-stream, and states imported from or exported
 * to lfilter, are the live EQ's (dspcore_eqlive.h), which carries lfilter's
 * own state.  zi == NULL starts from rest; zf == NULL stores nothing; zi == zf
 * (in place) is allowed, and so is x == y.  Elements [2S, ld_state) of a state
 * row are neither read nor written.
 *
 * The clip (clip != 0: to [-1, 1]) applies to the output only; the state is
 * that of the unclipped recursion, as the reference clips once after the whole
 * signal (dsp_core.py:254).
 *
 * Non-finite input behaves as in dsp_biquad_cascade_f32: outputs before the
 * row's first inf or NaN are finite, every sample after it is NaN, and the exit
 * state is all NaN, so every later block of that channel is all NaN.  A zi row
 * that holds an inf or NaN gives an all-NaN row.
 *
 * n == 0 or B == 0 launches nothing and leaves zf as it is.  S == 0: y = x
 * (clipped when asked), no state is read or written.
 *
 * One launch (trace name "iir_stream"), no workspace: one wavefront per
 * channel, the block cut into C <= 64 chunks of T = 32 ceil(n / 2048) samples
 * (lane c = chunk c); pass 1 runs the cascade over every chunk but the last
 * from rest, a wave-private scan seeded with zi (S_0 = zi, S_{c+1} = A^T S_c +
 * E_c) recovers every chunk's entry state, pass 2 reruns the chunks from them
 * and the last live lane captures zf at the row's sample n.  T depends on n
 * alone, so a row's result is bitwise independent of B.
 * ------------------------------------------------------------------------- */
int dsp_stream_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const double* sos_host, int32_t S, int32_t clip,
                           const double* zi, double* zf, int64_t ld_state, void* stream);

/* ---------------------------------------------------------------------------
 * HOST, no device work: the dsp_src_polyphase_f32 call that serves one block
 * of a stream.  The stream is the L/M polyphase SRC of dspcore.h with K taps
 * (K odd) centred at c = (K - 1) / 2; output m reads inputs up to
 * (m M + c) div L and back hist = ceil(K / L) - 1 samples from there.
 *
 * After `consumed` input and `produced` output samples, a block of n_block
 * more inputs makes output m computable iff (m M + c) div L < consumed +
 * n_block.  The call writes
 *     *hist     = ceil(K / L) - 1
 *     *n_out    = max(0, ceil(((consumed + n_block) L - c) / M)) - produced
 *     *c_offset = produced M + c - (consumed - hist) L          (always >= 0)
 * and the block is y[produced : produced + n_out] =
 *     dsp_src_polyphase_f32(staging, n_in = hist + n_block, n_out, c_offset)
 * where the staging row is [hist samples before the block | block]; at the
 * start of the stream the history is zeros (the one-shot call's zero padding).
 * n_out may be 0: nothing is launched then.
 *
 * flush != 0 ends the stream (n_block must be 0): n_in = hist,
 *     *n_out = ceil(consumed L / M) - produced,
 * the outputs whose windows reach past the last input; the kernel's zero
 * padding to the right is the one-shot call's.  The concatenated blocks are
 * bitwise the one-shot call on the whole signal (c_offset = (min(N L, K) - 1)
 * / 2, n_out = ceil(max(N L, K) / M)) whenever N L >= K.  A shorter stream
 * (N L < K) still gives ceil(N L / M) outputs centred at (K - 1) / 2 -- what
 * the one-shot call would give for the signal zero-padded to K / L samples --
 * where the one-shot call centres at (N L - 1) / 2 and returns ceil(K / M).
 *
 * `produced` must be the count `consumed` inputs make computable,
 * max(0, ceil((consumed L - c) / M)): every block call emits all it can, and
 * the hist samples kept are exactly what the next outputs still read.
 *
 * DSP_EINVAL: even or non-positive K, L or M < 1, negative counts, any other
 * `produced`, n_block != 0 with flush, a null output pointer.  DSP_ENOTSUP:
 * hist > DSP_STREAM_MAX_HIST.
 * ------------------------------------------------------------------------- */
int dsp_stream_src_geometry(int32_t K, int32_t L, int32_t M, int64_t consumed, int64_t produced,
                            int64_t n_block, int32_t flush, int64_t* hist, int64_t* c_offset,
                            int64_t* n_out);

/* ---------------------------------------------------------------------------
 * Moves the history of the staging rows to their front for the next block:
 *     buf[b][0 : hist] = buf[b][n_block : n_block + hist],  b < B
 * (rows [B][ld] float32, ld >= hist + n_block).  The ranges overlap when
 * n_block < hist; each row is read whole before it is written.  hist <=
 * DSP_STREAM_MAX_HIST (more: DSP_ENOTSUP).  hist == 0, n_block == 0 or B == 0
 * launches nothing.  One launch (trace name "stream_roll").
 * ------------------------------------------------------------------------- */
int dsp_stream_roll_f32(float* buf, int64_t B, int64_t ld, int64_t hist, int64_t n_block,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_STREAM_H */
