/*
 * dspcore_partconv.h — partitioned fast convolution of libdspcore.so: a real
 * FIR of 1 .. 2^20 float32 taps (a room response) applied to batched rows by
 * uniformly partitioned overlap-save on the in-LDS radix-16 FFT, one-shot or
 * block by block as a stream.  Where dsp_fastconv_f32 stops at the 8193 taps
 * that fit one 2^14-point transform, this cuts the taps into S partitions of
 * P = N/2, transforms every input block once and gives each output block as
 * the sum of S spectrum products followed by one inverse transform.
 *
 * Conventions are dspcore.h's: data pointers are device pointers owned by the
 * caller, `stream` is a hipStream_t, launches are asynchronous on it (nothing
 * synchronises or allocates, so a call is graph-capturable), 0 on success or a
 * negative DSP_E* code with the thread-local dsp_last_error string.  This
 * header versions on its own (dsp_partconv_version); dspcore.h, dsp_version
 * and every other header are unchanged by it.
 *
 * Geometry.  N = 2^log2n, 6 <= log2n <= DSP_MAX_LOG2N; V = N/4 outputs per
 * block; P = H = 2 V = N/2 is both the partition length and the hop of a pair
 * of blocks; S = ceil(K / P) <= 1024 partitions, the last zero-padded.
 * Positions are absolute: `pos` samples of the stream precede x[0], and with
 * u the stream (zeros before its sample 0) and u'[a] = u[a + offset], pair q
 * is the N-point transform
 *     Z_q = FFT(z),  z[n] = u'[q H - 3 V + n] + i u'[q H - 2 V + n],
 * two consecutive blocks of the SAME row as real and imaginary part; rows are
 * never paired with each other.  A partition delays by P = one pair, so with
 * Hf[s] = FFT_N(taps[s P .. s P + P)) / N
 *     W_q = sum_{s < S} Z_(q-s) Hf[s],   D = FFT(conj(W_q)),
 *     outputs [q H, q H + V) = Re D[3V ..],  [q H + V, q H + 2V) = -Im D[3V ..]
 * (the circular wrap needs N - V >= P - 1).  The stream's first pair is
 * floor(-offset / H): with offset > 0 the samples x[0 .. offset) sit at
 * negative u' positions, so pairs q < 0 are transformed as well; pairs before
 * the first are zero and are skipped in the sum.
 *
 * The spectra Z_q live in a ring in the caller's workspace: slot q mod `slots`
 * of the row, N complex float32 per slot, then one int32 flag per (row, slot).
 * A pair all of whose samples have arrived is complete and stays in the ring
 * for the S - 1 pairs after it; the last, partial pair of a call is computed
 * against zeros and computed again by the next call.
 */
#ifndef DSPCORE_PARTCONV_H
#define DSPCORE_PARTCONV_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_PARTCONV_MAX_TAPS (1 << 20)
#define DSP_PARTCONV_MAX_PARTS 1024

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_partconv_version(void);

/* ---------------------------------------------------------------------------
 * HOST, no device work.
 *
 * dsp_partconv_log2n: the default transform size for K taps, the smallest
 * log2n in 6 .. 14 whose partition holds all taps (N/2 >= K, S = 1) and 14
 * above 8192 taps (the larger the transform, the fewer spectra each output
 * reads: 32 K / N bytes).  DSP_EINVAL for K < 1 or K > 2^20.
 *
 * dsp_partconv_hist_len: samples per row of the time-domain history,
 * S H + 3 V >= K - 1: what the direct sums of the non-finite fallback (K - 1),
 * the repeat of a partial pair (up to 5 V - 1) and dsp_partconv_prime_f32
 * (all of it) read.
 *
 * dsp_partconv_slots: a ring size that suffices for every call with n_in and
 * n_out <= n at this offset, at any pos: S + ceil((n + offset) / H) + 1.
 *
 * dsp_partconv_workspace_bytes: bytes of the ring of B rows, `slots` slots
 * (spectra, then flags); SIZE_MAX where that overflows.
 *
 * Each returns a negative DSP_E* code (0 for the size) on a bad argument:
 * DSP_ENOTSUP for log2n outside 6 .. DSP_MAX_LOG2N, DSP_EINVAL for K outside
 * 1 .. 2^20, S > 1024 or a negative count.
 * ------------------------------------------------------------------------- */
int dsp_partconv_log2n(int32_t K);
int64_t dsp_partconv_hist_len(int32_t K, int32_t log2n);
int64_t dsp_partconv_slots(int32_t K, int32_t log2n, int64_t n, int64_t offset);
size_t dsp_partconv_workspace_bytes(int64_t B, int32_t log2n, int64_t slots);

/* ---------------------------------------------------------------------------
 * For B rows and every m < n_out:
 *     y[b * ld_y + m] = sum_{t < K} taps[t] * s_b[m + offset - t],
 *     s_b[i] = x[b * ld_x + i]                   for 0 <= i < n_in,
 *     s_b[i] = 0                                 for i >= n_in,
 *     s_b[i] = hist_in[b * ld_hist + L + i]      for -L <= i < 0, pos > 0,
 *     s_b[i] = 0                                 for i < 0 otherwise,
 * L = dsp_partconv_hist_len(K, log2n).  pos = 0 starts a stream: nothing of
 * the ring or of hist_in is read.  pos > 0 continues one: hist_in holds the L
 * samples before x[0] and the ring the complete pairs of the calls so far
 * (same K, log2n, offset, slots), or what dsp_partconv_prime_f32 put there.
 * offset and n_out are dsp_fastconv_f32's: offset = 0 is the causal
 * convolution, (K - 1) / 2 with n_out = n_in 'same', 0 with n_out = n_in +
 * K - 1 'full'.
 *
 * hist_out (may be NULL) receives the last L samples of (history | x row),
 *     hist_out[b * ld_hist + j] = s_b[n_in - L + j],  j < L,
 * in the first launch and also when n_out == 0.  hist_in and hist_out are
 * distinct buffers that swap roles call by call.
 *
 * `taps`: the K float32 taps.  `hf`: S * N interleaved complex float32, row s
 * = FFT_N of taps[s P .. s P + P) (the last zero-padded) divided by N,
 * computed in float64 and rounded once.  `twiddles`: dsp_fft_c2c_f32's table
 * for N.  `ws`: dsp_partconv_workspace_bytes(B, log2n, slots) bytes, 16-byte
 * aligned; a call needs slots >= the pairs it touches, which
 * dsp_partconv_slots bounds.  Rows of x may start at any 4-byte alignment; x
 * and y must not overlap.
 *
 * Properties.  For fixed (K, log2n, offset) output m of a row depends bitwise
 * only on that row's samples and on pos + m: not on B, the neighbouring rows,
 * the rows' alignment or `slots`.  A row cut into calls whose lengths are
 * multiples of H (n_out = n_in, offset 0, pos the samples so far), chained
 * through history and ring, gives bitwise the one-call result; any other cut
 * gives the same values within 2e-6 * ||taps||_2 * max|x|.
 *
 * Non-finite input.  The first launch ORs the exponent test of every sample a
 * pair loads into the pair's flag.  A pair q with a flagged spectrum among
 * Z_(q-s), s < S, does not use the transforms: its <= 2 V outputs are the
 * direct sums over the caller's float32 `taps` in ascending t, every float32
 * product exact in a float64 accumulator and the sum rounded to float32 once,
 * so each has the IEEE class (finite, +inf, -inf, NaN) np.convolve gives it in
 * float64, NaN from inf * 0 at a zero tap included.  Every other pair holds no
 * such sample in any spectrum it reads and is untouched.
 *
 * Two launches (trace names "partconv_fwd", "partconv_mac"); the second is
 * skipped when n_out == 0, both when there is nothing to do.  DSP_ENOTSUP:
 * log2n outside 6 .. DSP_MAX_LOG2N.  DSP_EINVAL: K outside 1 .. 2^20, S >
 * 1024, a negative count, offset or pos, offset > K - 1, n_out > n_in + K - 1
 * - offset, ld_x < n_in, ld_y < n_out, ld_hist < L with a history pointer
 * given, hist_in == hist_out non-NULL, hist_in NULL with pos > 0, slots too
 * few for this call, ws_bytes too small, x and y overlapping, hf, twiddles or
 * ws misaligned (8, 8, 16 bytes), a null pointer where one is read or
 * written.  The checks come before any device work; B == 0 passes them and
 * launches nothing.
 * ------------------------------------------------------------------------- */
int dsp_partconv_f32(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x,
                     int64_t n_out, int64_t ld_y, int64_t offset, int64_t pos,
                     const float* hist_in, float* hist_out, int64_t ld_hist, const float* taps,
                     int32_t K, const float* hf, int32_t log2n, void* ws, size_t ws_bytes,
                     int64_t slots, const float* twiddles, void* stream);

/* ---------------------------------------------------------------------------
 * Rebuilds the ring of a stream (offset 0) that stands at `pos` samples from
 * its time-domain history alone: one "partconv_fwd" launch transforms the
 * complete pairs floor(pos / H) - S + 1 .. floor(pos / H) - 1 (those >= 0)
 * from hist[b * ld_hist + j] = s_b[pos - L + j], j < L, bitwise as the calls
 * that streamed those samples did.  Checks as above; nothing to do is OK.
 * ------------------------------------------------------------------------- */
int dsp_partconv_prime_f32(const float* hist, int64_t B, int64_t ld_hist, int64_t pos, int32_t K,
                           int32_t log2n, void* ws, size_t ws_bytes, int64_t slots,
                           const float* twiddles, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_PARTCONV_H */
