// Per-channel EQ (include/dspcore_eqbank.h): a bank of biquad cascades, row b
// of the batch runs the cascade of group row_group[b].
//
// k_iir_bank is k_iir_stream (iir_stream.hip) with the coefficients and the
// chunk transition read from a device table instead of the kernel arguments:
// one wavefront per channel, lane c = chunk c of the table's T samples, pass 1
// from rest, the wave-private scan seeded with zi, pass 2 from the carried
// states with the exit state captured at sample n (stream_pass.h, shared).
// The record address depends on blockIdx.x and row_group[blockIdx.x] alone:
// the index is loaded once and is wave uniform, and the table and the index
// array are __restrict__ (nothing the kernel stores can alias them -- without
// that the compiler must assume the y stores of the other branches do, and
// takes the coefficients through vector loads into ~60 more VGPRs), so the
// coefficients come through the scalar cache into scalar registers, where
// k_iir_stream's kernel arguments sit.  The lanes below D load their row of
// A^T as vector loads.
//
// One launch serves a bank of mixed stage counts: the kernel is instantiated
// for the table's largest count and the host pads every shorter group with
// the identity stage {1, 0, 0, 0, 0} that realize() emits (w = u, v = w
// exactly; its block of A^T is nilpotent and no other stage's state reads it;
// its terms in the scan are fma(0, finite, acc)), as the 7 -> 8 case of
// k_iir_stream already does.  A bypass group (no stage) is a copy, chosen by a
// wave-uniform test: an identity stage would turn the sample after an inf
// into NaN (fma(-0.0, inf, u)).
#include <cstring>
#include <vector>

#include "cascade.h"
#include "dspcore_eqbank.h"
#include "stream_pass.h"

namespace dsp {
namespace {

constexpr int kPStride = 2 * DSP_EQBANK_MAX_STAGES;  // row stride of a record's A^T

// One group.  The geometry fields are the table's, repeated in every record:
// the kernel compares them with the call's, which the host cannot do for a
// device table.
struct alignas(256) BankRecord {
  SosParams p;         // NORM realisation, identity stages past `stages`
  int32_t stages;      // the group's own stage count (0: bypass)
  int32_t clip;
  int32_t inst;        // stage count the kernel is instantiated for
  int32_t max_stages;  // largest stage count of the table
  int64_t T;           // chunk length of every call on the table
  double P[kPStride * kPStride];  // A^T over T samples at `inst` stages, row stride kPStride
};
static_assert(sizeof(BankRecord) == DSP_EQBANK_RECORD_BYTES, "record size is part of the ABI");

// 1..6 and 8 are instantiated (as run_stream's): 7 runs as 8, an all-bypass
// table as 1 (no row reaches the cascade).
int inst_stages(int max_stages) { return max_stages == 0 ? 1 : (max_stages == 7 ? 8 : max_stages); }

int64_t bank_chunk(int64_t max_n) { return kTS * ceil_div(max_n, kMaxChunk); }

// A row that cannot be served: all NaN, y and the state.
__device__ __forceinline__ void nan_row(float* yr, int64_t n, double* zf_row, int Dmax, int lane) {
  for (int64_t i = lane; i < n; i += kWave) yr[i] = __builtin_nanf("");
  if (zf_row && lane < Dmax) zf_row[lane] = __builtin_nan("");
}

template <int S>
__global__ __launch_bounds__(kWave) void k_iir_bank(const float* x, float* y, int64_t n,
                                                    int64_t ld_x, int64_t ld_y,
                                                    const BankRecord* __restrict__ bank, int G,
                                                    const int32_t* __restrict__ row_group,
                                                    int64_t T, int C, const double* zi, double* zf,
                                                    int64_t ld_state, int Dmax, int vec_x,
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
  const BankRecord* rec = bank + (known ? g : 0);
  if (!known || rec->T != T || rec->inst != S || 2 * rec->max_stages != Dmax) {
    nan_row(yr, n, zf_row, Dmax, lane);
    return;
  }
  const int stages = rec->stages, clip = rec->clip;
  if (stages == 0) {  // bypass: y = x, clipped when asked; no state
    const float clo = clip ? -1.f : -INFINITY, chi = clip ? 1.f : INFINITY;
    for (int64_t i = lane; i < n; i += kWave) yr[i] = clip_f32(xr[i], clo, chi);
    return;
  }
  SosParams p;  // what the instantiated stages read, before any store of this wave
#pragma unroll
  for (int k = 0; k < S; ++k) {
#pragma unroll
    for (int j = 0; j < 5; ++j) p.c[k][j] = rec->p.c[k][j];
  }
  p.G = rec->p.G;
  stream_row<S, Df2Cascade<true>>(xr, yr, tile, n, T, C, lane, p, clip,
                                  zi ? zi + b * ld_state : nullptr, zf_row, 2 * stages, vec_x,
                                  vec_y, [&](double (&prow)[D]) {
                                    const double* row = rec->P + lane * kPStride;
#pragma unroll
                                    for (int j = 0; j < D; ++j) prow[j] = row[j];
                                  });
}

int bank_build(void* bank_host, size_t bank_bytes, const double* sos, const int32_t* stages,
               const int32_t* clip, int32_t G, int32_t ld_stages, int64_t max_n) {
  DSP_REQUIRE(G >= 1, "G=%d groups (>= 1)", G);
  DSP_REQUIRE(bank_host && stages && clip, "null pointer");
  DSP_REQUIRE(ld_stages >= 0, "ld_stages=%d is negative", ld_stages);
  DSP_REQUIRE(max_n >= 1 && max_n <= ((int64_t)1 << 30), "max_n=%lld outside 1 .. 2^30",
              (long long)max_n);
  DSP_REQUIRE(bank_bytes >= mul_sat((size_t)G, sizeof(BankRecord)),
              "bank_bytes=%zu < %d records of %zu bytes", bank_bytes, G, sizeof(BankRecord));
  int max_stages = 0;
  for (int g = 0; g < G; ++g) {
    DSP_REQUIRE(stages[g] >= 0, "group %d: stages=%d is negative", g, stages[g]);
    if (stages[g] > DSP_EQBANK_MAX_STAGES)
      return set_error(DSP_ENOTSUP, "group %d: the EQ bank takes <= %d stages (stages=%d)", g,
                       DSP_EQBANK_MAX_STAGES, stages[g]);
    DSP_REQUIRE(stages[g] <= ld_stages, "group %d: stages=%d > ld_stages=%d", g, stages[g],
                ld_stages);
    max_stages = std::max(max_stages, (int)stages[g]);
  }
  DSP_REQUIRE(max_stages == 0 || sos, "null sos");
  const int inst = inst_stages(max_stages), D = 2 * inst;
  const int64_t T = bank_chunk(max_n);
  BankRecord* out = static_cast<BankRecord*>(bank_host);
  for (int g = 0; g < G; ++g) {
    const int S = stages[g];
    const double* gs = S ? sos + (size_t)g * ld_stages * 5 : nullptr;
    BankRecord r;
    std::memset(static_cast<void*>(&r), 0, sizeof(r));
    if (!realize(gs, S, &r.p))
      return set_error(DSP_ENOTSUP, "group %d: a stage with b0 == 0 (the EQ bank runs the "
                       "normalised realisation)", g);
    r.stages = S;
    r.clip = clip[g] != 0;
    r.inst = inst;
    r.max_stages = max_stages;
    r.T = T;
    if (S) {
      const std::vector<double> P = chunk_transition(r.p, inst, T);
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) r.P[i * kPStride + j] = P[(size_t)i * D + j];
    }
    std::memcpy(static_cast<void*>(out + g), &r, sizeof(r));
  }
  return DSP_OK;
}

template <int S>
void run_bank(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x, int64_t ld_y,
              const BankRecord* bank, int G, const int32_t* row_group, int64_t T,
              const double* zi, double* zf, int64_t ld_state, int Dmax, hipStream_t s) {
  const int C = (int)ceil_div(n, T);
  const int vec_x = ((ld_x & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0);
  const int vec_y = ((ld_y & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0);
  hipLaunchKernelGGL((k_iir_bank<S>), dim3((unsigned)B), dim3(kWave), 0, s, x, y, n, ld_x, ld_y,
                     bank, G, row_group, T, C, zi, zf, ld_state, Dmax, vec_x, vec_y);
}

int launch_bank(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x, int64_t ld_y,
                const void* bank, size_t bank_bytes, int32_t G, int32_t max_stages, int64_t max_n,
                const int32_t* row_group, const double* zi, double* zf, int64_t ld_state,
                hipStream_t s) {
  DSP_REQUIRE(B >= 0 && n >= 0, "bad sizes B=%lld n=%lld", (long long)B, (long long)n);
  DSP_REQUIRE(G >= 1, "G=%d groups (>= 1)", G);
  DSP_REQUIRE(max_stages >= 0 && max_stages <= DSP_EQBANK_MAX_STAGES,
              "max_stages=%d outside 0 .. %d", max_stages, DSP_EQBANK_MAX_STAGES);
  DSP_REQUIRE(max_n >= 1 && max_n <= ((int64_t)1 << 30), "max_n=%lld outside 1 .. 2^30",
              (long long)max_n);
  DSP_REQUIRE(n <= max_n, "n=%lld > the bank's max_n=%lld", (long long)n, (long long)max_n);
  DSP_REQUIRE(ld_x >= n && ld_y >= n, "leading dimension too small");
  DSP_REQUIRE(ld_state >= 2 * (int64_t)max_stages, "ld_state=%lld < 2 max_stages=%d",
              (long long)ld_state, 2 * max_stages);
  DSP_REQUIRE(B <= INT32_MAX, "batch too large");
  DSP_REQUIRE(bank_bytes >= mul_sat((size_t)G, sizeof(BankRecord)),
              "bank_bytes=%zu < %d records of %zu bytes", bank_bytes, G, sizeof(BankRecord));
  if (B == 0 || n == 0) return DSP_OK;
  DSP_REQUIRE(x && y && bank && row_group, "null pointer");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(bank) & 255) == 0, "the bank is not 256-byte aligned");
  const BankRecord* recs = static_cast<const BankRecord*>(bank);
  const int64_t T = bank_chunk(max_n);
  const int Dmax = 2 * max_stages;
  TraceScope trace("iir_bank", s);
#define DSP_BANK_CASE(SP)                                                                      \
  run_bank<SP>(x, y, B, n, ld_x, ld_y, recs, G, row_group, T, zi, zf, ld_state, Dmax, s); \
  break
  switch (inst_stages(max_stages)) {
    case 1: DSP_BANK_CASE(1);
    case 2: DSP_BANK_CASE(2);
    case 3: DSP_BANK_CASE(3);
    case 4: DSP_BANK_CASE(4);
    case 5: DSP_BANK_CASE(5);
    case 6: DSP_BANK_CASE(6);
    default: DSP_BANK_CASE(8);
  }
#undef DSP_BANK_CASE
  DSP_LAUNCHED("k_iir_bank");
  return DSP_OK;
}

}  // namespace
}  // namespace dsp

extern "C" {

int dsp_eqbank_version(void) { return 10000; }

size_t dsp_eqbank_bytes(int32_t G) {
  return G < 1 ? 0 : dsp::mul_sat((size_t)G, sizeof(dsp::BankRecord));
}

int dsp_eqbank_build(void* bank_host, size_t bank_bytes, const double* sos_host,
                     const int32_t* stages, const int32_t* clip, int32_t G, int32_t ld_stages,
                     int64_t max_n) {
  dsp::clear_error();
  return dsp::bank_build(bank_host, bank_bytes, sos_host, stages, clip, G, ld_stages, max_n);
}

int dsp_eqbank_cascade_f32(const float* x, float* y, int64_t B, int64_t n, int64_t ld_x,
                           int64_t ld_y, const void* bank, size_t bank_bytes, int32_t G,
                           int32_t max_stages, int64_t max_n, const int32_t* row_group,
                           const double* zi, double* zf, int64_t ld_state, void* stream) {
  dsp::clear_error();
  return dsp::launch_bank(x, y, B, n, ld_x, ld_y, bank, bank_bytes, G, max_stages, max_n,
                          row_group, zi, zf, ld_state, static_cast<hipStream_t>(stream));
}

}  // extern "C"
