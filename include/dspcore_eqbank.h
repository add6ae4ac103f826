/*
 * dspcore_eqbank.h — per-channel EQ of libdspcore.so: a bank of biquad
 * cascades, one gain set ("group") per row of the batch.  dspcore.h and
 * dspcore_stream.h run one cascade over every row; here row b runs the cascade
 * of group row_group[b], in one launch for the whole batch, with the entry and
 * exit state of dspcore_stream.h.  Rows stay independent: a row's result does
 * not depend on B, on the other rows' groups or on how a batch is split.
 *
 * Conventions are dspcore.h's: data pointers are device pointers owned by the
 * caller, `stream` is a hipStream_t, the launch is asynchronous on it (nothing
 * synchronises or allocates, so the call is graph-capturable), 0 on success or
 * a negative DSP_E* code with the thread-local dsp_last_error string.  This
 * header versions on its own (dsp_eqbank_version); dspcore.h, dsp_version,
 * dspcore_stream.h and dsp_stream_version are unchanged by it.
 *
 * Use: build the table on the host (dsp_eqbank_build), copy it to a 256-byte
 * aligned device buffer, upload one int32 group index per row, then call
 * dsp_eqbank_cascade_f32 per block with the (max_stages, max_n) the table was
 * built with.
 */
#ifndef DSPCORE_EQBANK_H
#define DSPCORE_EQBANK_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_EQBANK_MAX_STAGES 8    /* biquad stages per group */
#define DSP_EQBANK_RECORD_BYTES 2816 /* one group's record (a multiple of 256) */

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_eqbank_version(void);

/* HOST: bytes of the table of G groups, G * DSP_EQBANK_RECORD_BYTES (0 for
 * G < 1). */
size_t dsp_eqbank_bytes(int32_t G);

/* ---------------------------------------------------------------------------
 * HOST, no device work: fills bank_host (bank_bytes >= the byte count above)
 * with the records of G >= 1 groups.
 *
 * sos_host is float64 [G][ld_stages][5] = {b0, b1, b2, a1, a2} per stage,
 * a0 == 1; rows [0, stages[g]) of group g are used, 0 <= stages[g] <=
 * min(ld_stages, DSP_EQBANK_MAX_STAGES).  clip[g] != 0 clips that group's
 * output to [-1, 1].  sos_host may be NULL when every stages[g] == 0.
 *
 * max_n (1 .. 2^30) is the longest block any call on this table will take.  It
 * fixes the chunk length T = 32 ceil(max_n / 2048) of every call, so that one
 * chunk transition A^T per group serves blocks of any length up to max_n.
 *
 * A record holds what dsp_stream_cascade_f32 computes on the host per call,
 * from the same host functions (csrc/cascade.h), so the numbers are the same
 * doubles: the direct-form-II realisation c[k] = {1, b1/b0, b2/b0, a1, a2} and
 * the input gain prod b0; the group's stage count and clip flag; A^T for the
 * table's T; and the table's geometry (T, the largest stage count of the
 * table, the stage count the kernel is instantiated for), which the kernel
 * compares with the call's.  Every group is realised at the table's largest
 * stage count, shorter groups padded with the exact identity stage
 * {1, 0, 0, 0, 0}.
 *
 * DSP_EINVAL: a null pointer, G < 1, bank_bytes too small, max_n outside
 * 1 .. 2^30, a negative stage count or one above ld_stages.  DSP_ENOTSUP: a
 * group of more than DSP_EQBANK_MAX_STAGES stages, or a stage with b0 == 0
 * (every EQ band has b0 > 0; the kernel runs the normalised realisation only).
 * ------------------------------------------------------------------------- */
int dsp_eqbank_build(void* bank_host, size_t bank_bytes, const double* sos_host,
                     const int32_t* stages, const int32_t* clip, int32_t G, int32_t ld_stages,
                     int64_t max_n);

/* ---------------------------------------------------------------------------
 * y[b] = clip_g(cascade_g(x[b])) for [B][n] float32 rows, g = row_group[b],
 * started from the state zi[b] and leaving the state after exactly n samples
 * in zf[b].
 *
 * `bank` is a DEVICE copy of a built table of G groups, 256-byte aligned,
 * bank_bytes >= the table's byte count.  max_stages is the largest stages[g]
 * the table was built with and max_n its max_n; 0 <= n <= max_n (more:
 * DSP_EINVAL).  row_group is a DEVICE int32 [B].
 *
 * Chunking.  The block is cut into C = ceil(n / T) <= 64 chunks of the table's
 * T = 32 ceil(max_n / 2048) samples.  Whenever 32 ceil(n / 2048) == T that is
 * dsp_stream_cascade_f32's chunking of n, and on finite data row b is then
 * bitwise what dsp_stream_cascade_f32 gives that row alone with its group's
 * sos, clip and zi (y and zf): the identity stages pass their input through
 * exactly, their blocks of A^T do not reach the other stages' states, and
 * their terms in the scan are fma(0, finite, acc).  For other n the two differ
 * by float64 rounding before the float32 store, as any two chunkings do.
 *
 * State.  zi and zf are DEVICE float64 [B][ld_state], ld_state >= 2 *
 * max_stages.  Row b uses elements [0, 2 * stages[g]) in the order and the
 * realisation of dspcore_stream.h (the direct-form-II delay lines w1_0, w2_0,
 * w1_1, ...); the rest is neither read nor written.  zi == NULL starts from
 * rest; zf == NULL stores nothing; zi == zf (in place) and x == y are allowed.
 * The clip never touches the state.  A state is valid only for the group that
 * produced it; gains that change mid-stream are the live EQ's
 * (dspcore_eqlive.h).  Non-finite input and entry states behave as in
 * dsp_stream_cascade_f32.
 *
 * Bypass groups (stages[g] == 0): the row is copied, clipped only if clip[g],
 * and no state is read or written -- a copy path of its own, chosen per row,
 * so an inf or NaN comes back as it went in.
 *
 * The library cannot see row_group.  The kernel never reads outside the
 * table: a row whose index is not in [0, G) gets an all-NaN output row and
 * NaN in elements [0, 2 * max_stages) of its zf row, and nothing else is
 * touched.  The same answer meets a table whose geometry is not the call's
 * (max_stages, max_n).  Validate the indices on the host before the upload.
 *
 * B == 0 or n == 0 launches nothing and leaves zf as it is.  Otherwise one
 * launch for the whole batch, whatever the mix of groups and stage counts
 * (trace name "iir_bank"), no workspace: dsp_stream_cascade_f32's kernel
 * structure -- one wavefront per channel, lane c = chunk c, pass 1 from rest,
 * a wave-private scan seeded with zi, pass 2 from the carried states -- with
 * the coefficients and the lane's row of A^T read from the row's record.
 *
 * DSP_EINVAL: negative sizes, ld_x or ld_y < n, n > max_n, ld_state < 2 *
 * max_stages, max_stages outside 0 .. DSP_EQBANK_MAX_STAGES, G < 1, bank_bytes
 * too small, a misaligned bank, a null pointer where one is read.
 * ------------------------------------------------------------------------- */
int dsp_eqbank_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const void* bank, size_t bank_bytes, int32_t G,
                           int32_t max_stages, int64_t max_n, const int32_t* row_group,
                           const double* zi, double* zf, int64_t ld_state, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_EQBANK_H */
