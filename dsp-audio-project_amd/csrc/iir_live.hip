// Live EQ (include/dspcore_eqlive.h): a bank of biquad cascades whose state
// survives a change of the coefficients, so the gains may move between two
// blocks of a stream without a click.
//
// k_iir_live has the structure of k_iir_bank (iir_bank.hip) -- one wavefront
// per channel, lane c = chunk c of the table's T samples, pass 1 from rest, the
// wave-private scan seeded with zi, pass 2 from the carried states with the
// exit state captured at sample n (stream_pass.h, shared) -- and differs in the
// realisation.  The streaming kernels carry the delay lines of a direct form
// II with the b0 gains pulled out (cascade.h), which mean something only for
// the coefficients that produced them.  Here stage k carries (s1, s2) of
// lfilter's direct form II transposed, a state of the signal, stepped in the
// observable canonical form
//     y   = fma(b0, u, s1)
//     s1' = fma(d1, u, fma(-a1, s1, s2))      d1 = b1 - a1 b0
//     s2' = fma(d2, u, -a2 * s1)              d2 = b2 - a2 b0   (host, float64)
// which is lfilter's s1' = b1 u - a1 y + s2, s2' = b2 u - a2 y with y
// substituted: the state update does not wait for y, and a flat section (b ==
// a, b0 == 1) has d1 == d2 == 0 exactly, so at rest it stays exactly at rest
// and y == u exactly (b1 u - a1 y leaves rounding residue there).
//
// Non-finite input.  lfilter turns an inf into NaN one sample later (b1 u -
// a1 y = inf - inf for the peaking sections); the d-form would keep a signed
// inf in s1 for a sample or two, which the clip would turn into +-1.  The
// first stage therefore reads s2 through fma(u, 0, s2): s2 for a finite u (to
// the sign of a zero), NaN for an inf or NaN, so its s1 -- and with it every
// later output and state of the row -- is NaN from the next sample on, as in
// k_iir_stream.  One FMA per sample on top of the five per stage.
//
// As in k_iir_bank the record address depends on blockIdx.x and
// row_group[blockIdx.x] alone and the table and the index array are
// __restrict__, so the coefficients come through the scalar cache into scalar
// registers (iir_bank.hip's header explains why that matters).
#include <cstring>
#include <vector>

#include "cascade.h"
#include "dspcore_eqlive.h"
#include "stream_pass.h"

namespace dsp {
namespace {

constexpr int kLiveStride = 2 * DSP_EQLIVE_MAX_SLOTS;  // row stride of a record's A^T

// {b0, d1, d2, a1, a2} per slot; slots past the table's own pass their input
// through ({1, 0, 0, 0, 0}, at rest for ever).
struct LiveParams {
  double c[DSP_EQLIVE_MAX_SLOTS][5];
};

// One group.  The geometry fields are the table's, repeated in every record:
// the kernel compares them with the call's, which the host cannot do for a
// device table.  An all-zero record (T == 0) matches no call.
struct alignas(256) LiveRecord {
  LiveParams p;
  int32_t clip;
  int32_t copy;   // y = x: every slot flat and the row's state at rest (the caller's word)
  int32_t inst;   // slot count the kernel is instantiated for
  int32_t slots;  // slot count of the table
  int64_t T;      // chunk length of every call on the table
  // A^T over T samples at `inst` slots, row stride kLiveStride
  double P[kLiveStride * kLiveStride];
};
static_assert(sizeof(LiveRecord) == DSP_EQLIVE_RECORD_BYTES, "record size is part of the ABI");

// The realisation policy of stream_pass.h: s1, s2 are lfilter's zi per stage.
struct LiveDf2t {
  using Params = LiveParams;
  template <int S>
  static __device__ __forceinline__ double step(double u, double (&s1)[S], double (&s2)[S],
                                                const Params& p) {
    const double s20 = fma(u, 0.0, s2[0]);  // NaN for a non-finite u
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const double y = fma(p.c[k][0], u, s1[k]);
      const double n1 = fma(p.c[k][1], u, fma(-p.c[k][3], s1[k], k == 0 ? s20 : s2[k]));
      s2[k] = fma(p.c[k][2], u, -p.c[k][4] * s1[k]);
      s1[k] = n1;
      u = y;
    }
    return u;
  }
};

// One step of the same state system on the host: X <- A X + B u, state order
// (s1_0, s2_0, s1_1, ...).
void live_state_step(const LiveParams& p, int S, double* X, double u) {
  for (int k = 0; k < S; ++k) {
    const double* c = p.c[k];
    const double s1 = X[2 * k], s2 = X[2 * k + 1];
    const double y = c[0] * u + s1;
    X[2 * k] = c[1] * u + (s2 - c[3] * s1);
    X[2 * k + 1] = c[2] * u - c[4] * s1;
    u = y;
  }
}

// 1..6 and 8 are instantiated (as run_bank's): 7 runs as 8.
int inst_slots(int slots) { return slots == 7 ? 8 : slots; }

int64_t live_chunk(int64_t max_n) { return kTS * ceil_div(max_n, kMaxChunk); }

// A row that cannot be served: all NaN, y and the state.
__device__ __forceinline__ void nan_row(float* yr, int64_t n, double* zf_row, int Du, int lane) {
  for (int64_t i = lane; i < n; i += kWave) yr[i] = __builtin_nanf("");
  if (zf_row && lane < Du) zf_row[lane] = __builtin_nan("");
}

template <int S>
__global__ __launch_bounds__(kWave) void k_iir_live(const float* x, float* y, int64_t n,
                                                    int64_t ld_x, int64_t ld_y,
                                                    const LiveRecord* __restrict__ table, int G,
                                                    const int32_t* __restrict__ row_group,
                                                    int64_t T, int C, const double* zi, double* zf,
                                                    int64_t ld_state, int slots, int vec_x,
                                                    int vec_y) {
  constexpr int D = 2 * S;
  __shared__ __attribute__((aligned(16))) float tile[kWave * kRow];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* xr = x + b * ld_x;
  float* yr = y + b * ld_y;
  double* zf_row = zf ? zf + b * ld_state : nullptr;

  const int g = row_group[b];  // wave uniform: the address depends on blockIdx.x alone
  const bool known = g >= 0 && g < G;
  const LiveRecord* rec = table + (known ? g : 0);
  if (!known || rec->T != T || rec->inst != S || rec->slots != slots) {
    nan_row(yr, n, zf_row, 2 * slots, lane);
    return;
  }
  const int clip = rec->clip;
  if (rec->copy) {  // y = x, clipped when asked; no state
    const float clo = clip ? -1.f : -INFINITY, chi = clip ? 1.f : INFINITY;
    for (int64_t i = lane; i < n; i += kWave) yr[i] = clip_f32(xr[i], clo, chi);
    return;
  }
  LiveParams p;  // what the instantiated stages read, before any store of this wave
#pragma unroll
  for (int k = 0; k < S; ++k) {
#pragma unroll
    for (int j = 0; j < 5; ++j) p.c[k][j] = rec->p.c[k][j];
  }
  stream_row<S, LiveDf2t>(xr, yr, tile, n, T, C, lane, p, clip,
                          zi ? zi + b * ld_state : nullptr, zf_row, 2 * slots, vec_x, vec_y,
                          [&](double (&prow)[D]) {
                            const double* row = rec->P + lane * kLiveStride;
#pragma unroll
                            for (int j = 0; j < D; ++j) prow[j] = row[j];
                          });
}

int live_build(void* table_host, size_t bytes, const double* sos, const int32_t* clip,
               const int32_t* copy, int32_t G, int32_t slots, int64_t max_n) {
#pragma clang fp contract(off)  // d1, d2 are the plain float64 expressions, on every host
  DSP_REQUIRE(G >= 1, "G=%d groups (>= 1)", G);
  DSP_REQUIRE(table_host && sos && clip && copy, "null pointer");
  DSP_REQUIRE(slots >= 1, "slots=%d (>= 1)", slots);
  if (slots > DSP_EQLIVE_MAX_SLOTS)
    return set_error(DSP_ENOTSUP, "the live EQ takes <= %d slots (slots=%d)",
                     DSP_EQLIVE_MAX_SLOTS, slots);
  DSP_REQUIRE(max_n >= 1 && max_n <= ((int64_t)1 << 30), "max_n=%lld outside 1 .. 2^30",
              (long long)max_n);
  DSP_REQUIRE(bytes >= mul_sat((size_t)G, sizeof(LiveRecord)),
              "bytes=%zu < %d records of %zu bytes", bytes, G, sizeof(LiveRecord));
  const int inst = inst_slots(slots), D = 2 * inst;
  const int64_t T = live_chunk(max_n);
  LiveRecord* out = static_cast<LiveRecord*>(table_host);
  for (int g = 0; g < G; ++g) {
    LiveRecord r;
    std::memset(static_cast<void*>(&r), 0, sizeof(r));
    for (int k = 0; k < DSP_EQLIVE_MAX_SLOTS; ++k) {
      double* c = r.p.c[k];
      c[0] = 1.0;
      if (k >= slots) continue;
      const double* s = sos + ((size_t)g * slots + k) * 5;
      const double a1b0 = s[3] * s[0], a2b0 = s[4] * s[0];
      c[0] = s[0];
      c[1] = s[1] - a1b0;
      c[2] = s[2] - a2b0;
      c[3] = s[3];
      c[4] = s[4];
    }
    r.clip = clip[g] != 0;
    r.copy = copy[g] != 0;
    r.inst = inst;
    r.slots = slots;
    r.T = T;
    const std::vector<double> A =
        state_matrix(D, [&](double* X, double u) { live_state_step(r.p, inst, X, u); });
    const std::vector<double> P = chunk_transition(A, D, T);
    for (int i = 0; i < D; ++i)
      for (int j = 0; j < D; ++j) r.P[i * kLiveStride + j] = P[(size_t)i * D + j];
    std::memcpy(static_cast<void*>(out + g), &r, sizeof(r));
  }
  return DSP_OK;
}

template <int S>
void run_live(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x, int64_t ld_y,
              const LiveRecord* table, int G, const int32_t* row_group, int64_t T,
              const double* zi, double* zf, int64_t ld_state, int slots, hipStream_t s) {
  const int C = (int)ceil_div(n, T);
  const int vec_x = ((ld_x & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const int vec_y = ((ld_y & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0);
  hipLaunchKernelGGL((k_iir_live<S>), dim3((unsigned)B), dim3(kWave), 0, s, x, y, n, ld_x, ld_y,
                     table, G, row_group, T, C, zi, zf, ld_state, slots, vec_x, vec_y);
}

int launch_live(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x, int64_t ld_y,
                const void* table, size_t bytes, int32_t G, int32_t slots, int64_t max_n,
                const int32_t* row_group, const double* zi, double* zf, int64_t ld_state,
                hipStream_t s) {
  DSP_REQUIRE(B >= 0 && n >= 0, "bad sizes B=%lld n=%lld", (long long)B, (long long)n);
  DSP_REQUIRE(G >= 1, "G=%d groups (>= 1)", G);
  DSP_REQUIRE(slots >= 1 && slots <= DSP_EQLIVE_MAX_SLOTS, "slots=%d outside 1 .. %d", slots,
              DSP_EQLIVE_MAX_SLOTS);
  DSP_REQUIRE(max_n >= 1 && max_n <= ((int64_t)1 << 30), "max_n=%lld outside 1 .. 2^30",
              (long long)max_n);
  DSP_REQUIRE(n <= max_n, "n=%lld > the table's max_n=%lld", (long long)n, (long long)max_n);
  DSP_REQUIRE(ld_x >= n && ld_y >= n, "leading dimension too small");
  DSP_REQUIRE(ld_state >= 2 * (int64_t)slots, "ld_state=%lld < 2 slots=%d", (long long)ld_state,
              2 * slots);
  DSP_REQUIRE(B <= INT32_MAX, "batch too large");
  DSP_REQUIRE(bytes >= mul_sat((size_t)G, sizeof(LiveRecord)),
              "bytes=%zu < %d records of %zu bytes", bytes, G, sizeof(LiveRecord));
  if (B == 0 || n == 0) return DSP_OK;
  DSP_REQUIRE(x && y && table && row_group, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(table) & 255) == 0,
              "the table is not 256-byte aligned");
  const LiveRecord* recs = static_cast<const LiveRecord*>(table);
  const int64_t T = live_chunk(max_n);
  TraceScope trace("iir_live", s);
#define DSP_LIVE_CASE(SP)                                                                  \
  run_live<SP>(x, y, B, n, ld_x, ld_y, recs, G, row_group, T, zi, zf, ld_state, slots, s); \
  break
  switch (inst_slots(slots)) {
    case 1: DSP_LIVE_CASE(1);
    case 2: DSP_LIVE_CASE(2);
    case 3: DSP_LIVE_CASE(3);
    case 4: DSP_LIVE_CASE(4);
    case 5: DSP_LIVE_CASE(5);
    case 6: DSP_LIVE_CASE(6);
    default: DSP_LIVE_CASE(8);
  }
#undef DSP_LIVE_CASE
  DSP_LAUNCHED("k_iir_live");
  return DSP_OK;
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_eqlive_version(void) { return 10000; }

size_t dsp_eqlive_bytes(int32_t G) {
  return G < 1 ? 0 : dsp::mul_sat((size_t)G, sizeof(dsp::LiveRecord));
}

int dsp_eqlive_build(void* table_host, size_t bytes, const double* sos_host, const int32_t* clip,
                     const int32_t* copy, int32_t G, int32_t slots, int64_t max_n) {
  dsp::clear_error();
  return dsp::live_build(table_host, bytes, sos_host, clip, copy, G, slots, max_n);
}

int dsp_eqlive_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const void* table, size_t bytes, int32_t G,
                           int32_t slots, int64_t max_n, const int32_t* row_group,
                           const double* zi, double* zf, int64_t ld_state, void* stream) {
  dsp::clear_error();
  return dsp::launch_live(x, y, B, n, ld_x, ld_y, table, bytes, G, slots, max_n, row_group, zi,
                          zf, ld_state, static_cast<hipStream_t>(stream));
}

}  // extern "C"
