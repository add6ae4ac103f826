// Device code shared by the streaming cascade (iir_stream.hip), the EQ bank
// (iir_bank.hip) and the live EQ (iir_live.hip): one wavefront filters one
// channel's block of n samples, cut into C <= 64 chunks of T samples (lane c =
// chunk c), from an entry state to an exit state.  The first two kernels differ
// only in where the coefficients and the chunk transition A^T come from; the
// arithmetic below is the same instructions in the same order for both, so a
// row's result is bitwise the same through either.  The realisation -- what
// the two state words of a stage mean and how one sample steps them -- is a
// policy R: R::Params is what a pass reads, R::step<S>(u, s1, s2, p) one
// sample through the S stages.
#pragma once

#include "cascade.h"

namespace dsp {
namespace {

constexpr int kTS = 32;          // samples per tile step
constexpr int kRow = kTS + 1;    // LDS row stride in floats (conflict-free column reads)
constexpr int kLoads = kTS / 4;  // 4-sample vectors per thread per tile
constexpr int kMaxChunk = 2048;  // T = 32 ceil(n / 2048) gives C <= 64 up to n = 2^30

__device__ __forceinline__ void wave_fence() { asm volatile("" ::: "memory"); }

// The direct form II of cascade.h (iir_stream.hip, iir_bank.hip): s1, s2 are
// the delay lines w1, w2.
template <bool NORM>
struct Df2Cascade {
  using Params = SosParams;
  template <int S>
  static __device__ __forceinline__ double step(double u, double (&s1)[S], double (&s2)[S],
                                                const Params& p) {
    return cascade_step<S, NORM>(u, s1, s2, p);
  }
};

// Tile [t0, t0 + 32) of the wave's 64 chunk rows: thread tid loads vector
// (tid & 7) of rows i * 8 + (tid >> 3) (8 threads per row, 128 contiguous
// bytes).  Row r starts at sample r * T of the channel.  Samples at or past n
// reach nothing that is stored (outputs past the row's end are dropped, zf is
// captured at sample n, the last chunk's pass-1 state is unused), so they are
// not masked.  vec (rows 16-byte aligned, ld % 4 == 0): branch-free -- a
// vector with a sample below n is loaded whole (ld % 4 == 0 and ld >= n keep
// it inside the row pitch), others load the row's first vector.  Otherwise
// guarded scalar loads.
__device__ __forceinline__ void fetch(float4 (&v)[kLoads], const float* xr, int64_t n, int64_t T,
                                      int t0, int tid, int vec) {
  const int c4 = (tid & 7) * 4;
  if (vec) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int at = (i * (kWave / 8) + (tid >> 3)) * (int)T + t0 + c4;
      v[i] = *reinterpret_cast<const float4*>(at < n ? xr + at : xr);
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int at = (i * (kWave / 8) + (tid >> 3)) * (int)T + t0 + c4;
      v[i].x = at + 0 < n ? xr[at + 0] : 0.f;
      v[i].y = at + 1 < n ? xr[at + 1] : 0.f;
      v[i].z = at + 2 < n ? xr[at + 2] : 0.f;
      v[i].w = at + 3 < n ? xr[at + 3] : 0.f;
    }
  }
}

__device__ __forceinline__ void tile_put(float* tile, const float4 (&v)[kLoads], int tid) {
  const int c4 = (tid & 7) * 4;
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    float* d = tile + (i * (kWave / 8) + (tid >> 3)) * kRow + c4;
    d[0] = v[i].x;
    d[1] = v[i].y;
    d[2] = v[i].z;
    d[3] = v[i].w;
  }
}

__device__ __forceinline__ void tile_store(float* yr, const float* tile, int64_t n, int64_t T,
                                           int t0, int tid, int vec) {
  const int c4 = (tid & 7) * 4;
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int r = i * (kWave / 8) + (tid >> 3);
    const int at = r * (int)T + t0 + c4;
    const float* s = tile + r * kRow + c4;
    if (vec && at + 3 < n) {
      *reinterpret_cast<float4*>(yr + at) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
      if (at + 0 < n) yr[at + 0] = s[0];
      if (at + 1 < n) yr[at + 1] = s[1];
      if (at + 2 < n) yr[at + 2] = s[2];
      if (at + 3 < n) yr[at + 3] = s[3];
    }
  }
}

// One pass of the wave over its 64 chunk rows, tile by tile, the next tile's
// loads in flight during the current tile's arithmetic.  APPLY: outputs are
// clipped and stored, and the lane with a non-null `zf` stores its delay
// lines after local sample `cap` - 1 (wave uniform, 1 <= cap <= T) there --
// straight from the loop, under a wave-uniform test of the sample index, so
// the exit state costs no registers in the tiles that do not hold it.  xr may
// equal yr: a tile is read before it is written and tiles do not overlap.
template <int S, class R, bool APPLY>
__device__ __forceinline__ void stream_pass(const float* xr, float* yr, float* tile, int64_t n,
                                            int64_t T, int lane, double (&s1)[S], double (&s2)[S],
                                            const typename R::Params& p, int clip, int vec_x,
                                            int vec_y, int cap, double* zf, int Du) {
  float* my = tile + lane * kRow;
  float4 v[kLoads];
  fetch(v, xr, n, T, 0, lane, vec_x);
  const float clo = clip ? -1.f : -INFINITY, chi = clip ? 1.f : INFINITY;
  for (int t0 = 0; t0 < (int)T; t0 += kTS) {
    wave_fence();  // readers of the previous tile are done
    tile_put(tile, v, lane);
    wave_fence();
    if (t0 + kTS < (int)T) fetch(v, xr, n, T, t0 + kTS, lane, vec_x);
    if constexpr (APPLY) {
#pragma unroll 8
      for (int j = 0; j < kTS; ++j) {
        const float out = (float)R::template step<S>((double)my[j], s1, s2, p);
        my[j] = clip_f32(out, clo, chi);
        if (t0 + j + 1 == cap && zf) {  // the row's last sample: the exit state, unclipped
          double f[2 * S];
#pragma unroll
          for (int k = 0; k < S; ++k) {
            f[2 * k] = s1[k];
            f[2 * k + 1] = s2[k];
          }
          nf_poison(f);
#pragma unroll
          for (int i = 0; i < 2 * S; ++i)
            if (i < Du) zf[i] = f[i];
        }
      }
      wave_fence();
      tile_store(yr, tile, n, T, t0, lane, vec_y);
    } else {
#pragma unroll 8
      for (int j = 0; j < kTS; ++j) (void)R::template step<S>((double)my[j], s1, s2, p);
    }
  }
  wave_fence();
}

// One channel's block through the S-stage cascade `p`: pass 1 from rest, the
// scan seeded with the entry state, pass 2 from the carried states.
//   tile:       the wave's kWave * kRow floats of LDS (the scan reuses it);
//   zi_row:     the channel's entry state (null: rest), zf_row its exit state
//               (null: not stored); Du <= 2S components of either are used;
//   load_prow:  fills a lane's row of A^T (called by lanes below D = 2S).
// Everything is wave-private: LDS instructions of one wave execute in program
// order, so the tile hand-offs and the scan need compiler fences only.
template <int S, class R, class PROW>
__device__ __forceinline__ void stream_row(const float* xr, float* yr, float* tile, int64_t n,
                                           int64_t T, int C, int lane,
                                           const typename R::Params& p, int clip,
                                           const double* zi_row, double* zf_row, int Du,
                                           int vec_x, int vec_y, PROW load_prow) {
  constexpr int D = 2 * S;
  static_assert(kWave * D * 2 <= kWave * kRow, "the scan must fit in the tile");
  double* scan = reinterpret_cast<double*>(tile);  // [C][D]: slot c = S_c

  double s1[S], s2[S];
#pragma unroll
  for (int k = 0; k < S; ++k) s1[k] = s2[k] = 0.0;

  // ---- pass 1: end state from rest of every chunk (the last one's is unused)
  if (C > 1)
    stream_pass<S, R, false>(xr, yr, tile, n, T, lane, s1, s2, p, clip, vec_x, vec_y, 0, nullptr,
                             0);
  double e[D];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    e[2 * k] = s1[k];
    e[2 * k + 1] = s2[k];
  }
  nf_poison(e);  // a chunk whose input held an inf or NaN hands NaN on

  // ---- scan: slot 0 = zi, slot c + 1 = A^T slot c + E_c
  if (lane + 1 < C) {
#pragma unroll
    for (int i = 0; i < D; ++i) scan[(lane + 1) * D + i] = e[i];
  }
  const bool row_lane = lane < D;
  double prow[D];
  if (row_lane) {
    scan[lane] = (zi_row && lane < Du) ? zi_row[lane] : 0.0;
    load_prow(prow);
  }
  wave_fence();
  if (row_lane) {  // a non-finite entry state becomes all NaN
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) t = fma(scan[j], 0.0, t);
    wave_fence();  // every lane has read slot 0
    if (!__builtin_isfinite(t)) scan[lane] = __builtin_nan("");
  }
  wave_fence();
  for (int cc = 0; cc + 1 < C; ++cc) {
    if (row_lane) {
      double acc = scan[(cc + 1) * D + lane];
#pragma unroll
      for (int j = 0; j < D; ++j) acc = fma(prow[j], scan[cc * D + j], acc);
      wave_fence();
      scan[(cc + 1) * D + lane] = acc;
    }
    wave_fence();
  }
  const int src = lane < C ? lane : 0;  // lanes past the row: any finite-or-not state, never stored
#pragma unroll
  for (int k = 0; k < S; ++k) {
    s1[k] = scan[src * D + 2 * k];
    s2[k] = scan[src * D + 2 * k + 1];
  }
  wave_fence();  // states read before the tile is reused

  // ---- pass 2: outputs from the carried states; lane C - 1 stores zf
  const int cap = (int)(n - (int64_t)(C - 1) * T);
  double* zo = (zf_row && lane == C - 1) ? zf_row : nullptr;
  stream_pass<S, R, true>(xr, yr, tile, n, T, lane, s1, s2, p, clip, vec_x, vec_y, cap, zo, Du);
}

}  // namespace
}  // namespace dsp
