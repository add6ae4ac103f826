/*
 * dspcore_fastconv.h — fast convolution of libdspcore.so: a long real FIR
 * (1 .. 8193 float32 taps) applied to batched rows by overlap-save on the
 * in-LDS radix-16 FFT, one-shot or block by block with the history carried.
 * Where dsp_src_polyphase_f32 (L = M = 1) pays K multiply-adds per output,
 * this pays two N-point transforms per 2 (N - K + 1) outputs.
 *
 * Conventions are dspcore.h's: data pointers are device pointers owned by the
 * caller, `stream` is a hipStream_t, the launch is asynchronous on it (nothing
 * synchronises or allocates, so a call is graph-capturable), 0 on success or a
 * negative DSP_E* code with the thread-local dsp_last_error string.  This
 * header versions on its own (dsp_fastconv_version); dspcore.h, dsp_version
 * and the stream, bank, live-EQ and stream-spectrum headers are unchanged by
 * it.
 *
 * Geometry.  N = 2^log2n, 6 <= log2n <= DSP_MAX_LOG2N; K taps, 1 <= K <=
 * N/2 + 1; V = N - (K - 1) valid outputs per block.  Block p of a row gives
 * outputs [p V, p V + V) from the N row samples that end at output index
 * p V + V - 1 + offset.  The taps are real, so one complex transform carries
 * two consecutive blocks (2p, 2p + 1) of the SAME row as its real and
 * imaginary parts (a trailing odd block pairs with zeros); rows are never
 * paired with each other.  Per transform, with Hf = FFT_N(taps, zero-padded)
 * / N from the caller:
 *     A = FFT(z),  C = conj(A * Hf),  D = FFT(C),
 *     block 2p = Re D[K-1 ..],  block 2p+1 = -Im D[K-1 ..].
 */
#ifndef DSPCORE_FASTCONV_H
#define DSPCORE_FASTCONV_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_fastconv_version(void);

/* ---------------------------------------------------------------------------
 * HOST, no device work.  The default transform size for K taps: the smallest
 * log2n in 6 .. 14 with 2^log2n >= 4 (K - 1), and 14 where only that still
 * fits (K <= 8193 = 2^13 + 1).  DSP_EINVAL for K < 1, DSP_ENOTSUP for
 * K > 8193.
 * ------------------------------------------------------------------------- */
int dsp_fastconv_log2n(int32_t K);

/* ---------------------------------------------------------------------------
 * For B rows and every m < n_out:
 *     y[b * ld_y + m] = sum_{t < K} taps[t] * s_b[m + offset - t],
 *     s_b[i] = x[b * ld_x + i]                      for 0 <= i < n_in,
 *     s_b[i] = 0                                    for i >= n_in,
 *     s_b[i] = hist_in[b * ld_hist + (K - 1) + i]   for -(K - 1) <= i < 0
 *              (0 with hist_in == NULL).
 * offset = 0 is lfilter's causal convolution; offset = (K - 1) / 2 with n_out
 * = n_in is np.convolve's mode 'same' for n_in >= K; offset = 0 with n_out =
 * n_in + K - 1 is 'full'.
 *
 * hist_out (may be NULL) receives, in the same launch as the outputs and also
 * when n_out == 0, the last K - 1 samples of (history | x row):
 *     hist_out[b * ld_hist + j] = s_b[n_in - (K - 1) + j],  j < K - 1,
 * which for n_in < K - 1 include samples of hist_in.  hist_in and hist_out are
 * distinct buffers that swap roles call by call.  Elements of hist_out from
 * K - 1 on, the padding of y's rows and every input are left as they are.
 *
 * `taps` are the K float32 taps, `hf` N interleaved complex float32 = FFT_N of
 * the zero-padded taps divided by N (computed in float64, rounded once),
 * `twiddles` the table of dsp_fft_c2c_f32 for N: exp(-2 pi i k / N), k < N/2.
 * Rows of x may start at any 4-byte alignment (samples are read one by one);
 * x and y must not overlap.
 *
 * Properties.  For fixed (K, log2n, offset) output m of a row depends bitwise
 * only on that row's samples: not on B, on the neighbouring rows or on the
 * rows' alignment.  A row cut into calls whose lengths are multiples of 2 V,
 * chained through the history, gives bitwise the one-call result (the same
 * blocks and the same pairs form either way); any other cut gives the same
 * values within 2e-6 * ||taps||_2 * max|x|.
 *
 * Non-finite input.  An inf or NaN in a block would smear NaN over all N
 * outputs of its transform.  In the SAME launch, a transform whose loaded
 * samples (either block of its pair) hold an inf or NaN -- an OR through LDS
 * of the exponent test at load time, uniform per transform -- does not use
 * the FFT result: its outputs are the direct sums over the caller's float32
 * `taps` in ascending t, every float32 product exact in a float64 accumulator
 * and the sum rounded to float32 once.  Each such output so has the IEEE class
 * (finite, +inf, -inf, NaN) of the product-then-sum over its own K-sample
 * window as np.convolve gives it in float64 on the same float32 taps, NaN from
 * inf * 0 at a zero tap included.  Outputs of transforms without a non-finite
 * sample are untouched by this.
 *
 * One launch (trace name "fastconv").  DSP_ENOTSUP: log2n outside 6 ..
 * DSP_MAX_LOG2N.  DSP_EINVAL: K < 1 or K > N/2 + 1, a negative count or
 * offset, offset > K - 1, n_out > n_in + K - 1 - offset, ld_x < n_in, ld_y <
 * n_out, ld_hist < K - 1 with a history pointer given, hist_in == hist_out
 * non-NULL, x and y overlapping, a null pointer where one is read or written.
 * The checks come before any device work; B == 0 passes them and launches
 * nothing.
 * ------------------------------------------------------------------------- */
int dsp_fastconv_f32(const float* x, float* y, int64_t B, int64_t n_in, int64_t ld_x,
                     int64_t n_out, int64_t ld_y, int64_t offset, const float* hist_in,
                     float* hist_out, int64_t ld_hist, const float* taps, int32_t K,
                     const float* hf, int32_t log2n, const float* twiddles, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_FASTCONV_H */
