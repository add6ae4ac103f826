/*
 * dspcore_eqlive.h — live EQ of libdspcore.so: a bank of biquad cascades whose
 * gains may change from one block of a stream to the next without a click.
 * dspcore_stream.h and dspcore_eqbank.h carry each band's state as the delay
 * lines of the kernels' own direct form II, which mean something only for the
 * coefficients that produced them.  Here every band ("slot") carries the state
 * of scipy.signal.lfilter's direct form II transposed, which is a state of the
 * signal: the next block may run other coefficients from it, exactly as
 *     v, s[k] = lfilter(b_k, a_k, v, zi=s[k])
 * does with a new (b_k, a_k) per call.
 *
 * Conventions are dspcore.h's: data pointers are device pointers owned by the
 * caller, `stream` is a hipStream_t, the launch is asynchronous on it (nothing
 * synchronises or allocates, so the call is graph-capturable), 0 on success or
 * a negative DSP_E* code with the thread-local dsp_last_error string.  This
 * header versions on its own (dsp_eqlive_version); dspcore.h, dsp_version and
 * the stream and bank headers with their versions are unchanged by it.
 *
 * Use: a live EQ has a fixed number of slots (1 .. DSP_EQLIVE_MAX_SLOTS), each
 * one biquad per group; a slot that is switched off runs a flat section (b ==
 * a, b0 == 1), not no section, so that what it still holds rings out through
 * its poles.  Build the table on the host (dsp_eqlive_build), copy it to a
 * 256-byte aligned device buffer, upload one int32 group index per row, call
 * dsp_eqlive_cascade_f32 per block with the state in place (zi == zf).  To
 * change the gains, build a new table and overwrite the device buffers in
 * stream order between two blocks; the state tensor stays as it is.
 */
#ifndef DSPCORE_EQLIVE_H
#define DSPCORE_EQLIVE_H

#include "dspcore.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSP_EQLIVE_MAX_SLOTS 8       /* biquad slots per group */
#define DSP_EQLIVE_RECORD_BYTES 2560 /* one group's record (a multiple of 256) */

/* Version of this header's entry points (major*10000 + minor*100 + patch). */
int dsp_eqlive_version(void);

/* HOST: bytes of the table of G groups, G * DSP_EQLIVE_RECORD_BYTES (0 for
 * G < 1). */
size_t dsp_eqlive_bytes(int32_t G);

/* ---------------------------------------------------------------------------
 * HOST, no device work: fills table_host (bytes >= the byte count above) with
 * the records of G >= 1 groups of `slots` sections each, 1 <= slots <=
 * DSP_EQLIVE_MAX_SLOTS.
 *
 * sos_host is float64 [G][slots][5] = {b0, b1, b2, a1, a2} per slot, a0 == 1.
 * Any b0 is allowed, 0 included.  clip[g] != 0 clips that group's output to
 * [-1, 1].  copy[g] != 0 makes the group a copy: its rows are y = x (clipped
 * when clip[g]), no state is read or written and an inf or NaN comes back as
 * it went in -- for rows whose every slot is flat and whose state is at rest,
 * which the caller tracks (a flat section at rest passes its input exactly, so
 * the copy is the same finite result at no arithmetic).
 *
 * max_n (1 .. 2^30) is the longest block any call on this table will take.  It
 * fixes the chunk length T = 32 ceil(max_n / 2048) of every call.
 *
 * A record holds, per slot, {b0, d1, d2, a1, a2} with d1 = b1 - a1 b0 and
 * d2 = b2 - a2 b0 (float64): the kernel steps the observable canonical form
 *     y   = b0 u + s1
 *     s1' = d1 u + (s2 - a1 s1)
 *     s2' = d2 u - a2 s1
 * which is lfilter's recursion (s1' = b1 u - a1 y + s2, s2' = b2 u - a2 y)
 * with y substituted, on lfilter's own state.  A flat slot has d1 == d2 == 0
 * exactly, so at rest it stays at rest and y == u exactly.  The record also
 * holds the clip and copy flags, the transition A^T of the 2 * slots state
 * system over T samples, and the table's geometry (T, slots, the slot count the
 * kernel is instantiated for: 7 runs as 8 with a section that passes its input
 * through), which the kernel compares with the call's.
 *
 * DSP_EINVAL: a null pointer, G < 1, slots < 1, bytes too small, max_n outside
 * 1 .. 2^30.  DSP_ENOTSUP: slots > DSP_EQLIVE_MAX_SLOTS.
 * ------------------------------------------------------------------------- */
int dsp_eqlive_build(void* table_host, size_t bytes, const double* sos_host, const int32_t* clip,
                     const int32_t* copy, int32_t G, int32_t slots, int64_t max_n);

/* ---------------------------------------------------------------------------
 * y[b] = clip_g(cascade_g(x[b])) for [B][n] float32 rows, g = row_group[b],
 * started from the state zi[b] and leaving the state after exactly n samples
 * in zf[b].
 *
 * `table` is a DEVICE copy of a built table of G groups, 256-byte aligned,
 * bytes >= the table's byte count; slots and max_n are what it was built with;
 * 0 <= n <= max_n (more: DSP_EINVAL).  row_group is a DEVICE int32 [B].  G may
 * count records that no row points to (a buffer sized for the most groups a
 * stream will ever need, the unused records zero): they are never read.
 *
 * State.  zi and zf are DEVICE float64 [B][ld_state], ld_state >= 2 * slots.
 * Row b holds (s1_0, s2_0, s1_1, s2_1, ...): slot k's pair is scipy's `zi` of
 * that band, direct form II transposed.  It can be imported from and exported
 * to lfilter band by band, and it is valid for any coefficients: a block run
 * with other gains continues the same signal.  zi == NULL starts from rest;
 * zf == NULL stores nothing; zi == zf (in place) and x == y are allowed.
 * Elements [2 * slots, ld_state) are neither read nor written.  The clip never
 * touches the state.
 *
 * Non-finite input behaves as in dsp_stream_cascade_f32: outputs before the
 * row's first inf or NaN are finite, every sample after it is NaN, the exit
 * state is all NaN, and a zi row that holds an inf or NaN gives an all-NaN
 * row.  Copy groups pass inf and NaN through.
 *
 * The library cannot see row_group.  The kernel never reads outside the
 * table: a row whose index is not in [0, G) gets an all-NaN output row and NaN
 * in elements [0, 2 * slots) of its zf row, and nothing else is touched.  The
 * same answer meets a record whose geometry is not the call's (slots, max_n).
 *
 * B == 0 or n == 0 launches nothing and leaves zf as it is.  Otherwise one
 * launch for the whole batch (trace name "iir_live"), no workspace:
 * dsp_eqbank_cascade_f32's kernel structure -- one wavefront per channel, lane
 * c = chunk c of T samples, pass 1 from rest, a wave-private scan seeded with
 * zi, pass 2 from the carried states, the exit state captured at sample n.
 *
 * DSP_EINVAL: negative sizes, ld_x or ld_y < n, n > max_n, ld_state < 2 *
 * slots, slots outside 1 .. DSP_EQLIVE_MAX_SLOTS, G < 1, bytes too small, a
 * misaligned table, a null pointer where one is read.
 * ------------------------------------------------------------------------- */
int dsp_eqlive_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const void* table, size_t bytes, int32_t G,
                           int32_t slots, int64_t max_n, const int32_t* row_group,
                           const double* zi, double* zf, int64_t ld_state, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DSPCORE_EQLIVE_H */
