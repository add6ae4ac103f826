// Four-step FFT for N = 2^15 .. 2^DSP_MAX_LOG2N_FOURSTEP (beyond one workgroup's
// LDS): N = NA * NB, n = n1 + NB n2, k = k2 + NA k1 (n1, k1 < NB; n2, k2 < NA)
//   step A: Y[n1][k2] = W_N^(n1 k2) * sum_n2 x[n1 + NB n2] W_NA^(n2 k2)
//           -> workspace[k2][n1]
//   step B: X[k2 + NA k1] = sum_n1 Y[n1][k2] W_NB^(n1 k1)
// Each workgroup runs KC sub-transforms of consecutive columns (step A) or
// rows (step B) in LDS with the one-launch Stockham passes; the HBM side of
// both steps moves KC consecutive complex values per index (8 -- 64 B -- or
// 16 for the three-pass split's megabyte-strided passes), staged through LDS
// so that every global access is a run of consecutive addresses.  Up to 2^22
// two launches (sub-transforms up to 2^11); from 2^23 step B is itself a
// four-step (run_fft6_row).  The sub-transforms' twiddles come from the
// caller's W_N table at stride N/NA (N/NB), the inter-step twiddle W_N^m from
// the same table (m < N/2, else its negation), above 2^20 points as the
// product of two factors from small contiguous tables (tw_fetch).  The
// workspace holds Y: B x N complex (two launches) or Y, Y': 2 x N (three).
#include "fft_pass.h"

namespace dsp {
namespace {

// W_N^m for any m from the table exp(-2 pi i k / N), k < N/2.
__device__ __forceinline__ float2 tw_full(const float2* __restrict__ tw, int64_t m, int64_t N) {
  m &= N - 1;
  const float2 w = tw[m < N / 2 ? m : m - N / 2];
  return m < N / 2 ? w : make_float2(-w.x, -w.y);
}

constexpr int kCols = 8;
// Columns per workgroup for a sub-transform of 2^LOG2 points: KC images of
// (N + N/16 + 1) complex values within 160 KB of LDS.
__host__ __device__ constexpr int kcols_for(int log2) {
  return log2 <= 11 ? kCols : log2 == 12 ? 4 : log2 == 13 ? 2 : 1;
}

struct Fft4Args {
  FftArgs a;          // in / out / rows / segment / window / W_N table
  float2* ws;         // B x N complex
  int64_t N;          // NA * NB
  uint32_t* hdr;      // per row: non-finite flag, list length (fft_nf.hip); NULL: none
  int64_t tws = 1;    // a.tw is the table of N * tws points (nested inner steps)
  int64_t nest = 0;   // step B of a nested inner transform: the outer NA (run_fft6_row)
  const float2* twc = nullptr;  // N * tws > 2^20: W^(i << tsh), i < (N * tws) >> tsh
  int tsh = 0;
};

// The inter-step twiddle W_Nt^m, Nt = N * tws.  Up to 2^20 points one read of
// the caller's table; above, W^m = W^(hi << tsh) W^lo with lo < 2^tsh, tsh =
// ceil(log2 Nt / 2): the fine factor from the table's first 2^tsh entries, the
// coarse one from the 2^(log2 Nt - tsh) entries k_tw_coarse gathered into the
// workspace -- both contiguous and L2-resident, where the workgroup's W^(n1 k2)
// alone are scattered over the whole table (one line fetched per 8-byte
// twiddle: round 5 measured the 2^28 four-step at 0.49 TB/s).  One more
// rounding (~1 ulp of 1), far inside the FFT's 1e-5.  In two halves, so that
// the table loads can be issued long before the value is needed (a select or
// product on the loaded values would make the compiler wait for them at
// once): w = sgn * a * b.
struct TwLoad {
  float2 a, b;
  float sgn;
};
__device__ __forceinline__ TwLoad tw_fetch(const Fft4Args& f, int64_t m) {
  // branch-free (a branch would join the loaded values through copies, which
  // wait for them): without the coarse table b is the table's W^0 = 1
  const int64_t Nt = f.N * f.tws;
  m &= Nt - 1;
  const bool split = f.twc != nullptr, up = !split && m >= Nt / 2;
  const float2* pa = split ? f.twc : f.a.tw;
  const int64_t ia = split ? m >> f.tsh : (up ? m - Nt / 2 : m);
  const int64_t ib = split ? m & ((int64_t(1) << f.tsh) - 1) : 0;
  return TwLoad{pa[ia], f.a.tw[ib], up ? -1.f : 1.f};
}
__device__ __forceinline__ float2 tw_finish(const TwLoad& t) {
  const float2 w = make_float2(t.a.x * t.b.x - t.a.y * t.b.y, t.a.x * t.b.y + t.a.y * t.b.x);
  return make_float2(t.sgn * w.x, t.sgn * w.y);
}

__global__ __launch_bounds__(256) void k_tw_coarse(const float2* __restrict__ tw, float2* twc,
                                                   int64_t N, int tsh) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (N >> tsh)) twc[i] = tw_full(tw, i << tsh, N);
}

// Four-step sizes whose twiddles go through the coarse table, its shift and
// its size in bytes.
constexpr int kLog2TwSplit = 20;
inline int tw_shift(int log2n) { return (log2n + 1) / 2; }
inline size_t tw_coarse_bytes(int log2n) {
  return log2n > kLog2TwSplit ? (size_t(1) << (log2n - tw_shift(log2n))) * sizeof(float2) : 0;
}
int build_tw_coarse(const float2* tw, float2* twc, int log2n, hipStream_t s) {
  const int64_t n = int64_t(1) << (log2n - tw_shift(log2n));
  hipLaunchKernelGGL(k_tw_coarse, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, tw, twc,
                     int64_t(1) << log2n, tw_shift(log2n));
  DSP_LAUNCHED("k_tw_coarse");
  return DSP_OK;
}

// Step A's input (f.hdr set): a non-finite value raises the row's flag for the
// non-finite repair (fft_nf.hip) and, for the complex transforms, reads as
// zero, so that the output holds the DFT of the finite part -- the values the
// reference gives the components that no inf or NaN reaches.  (The spectrum's
// bins all become +inf or NaN; the repair rewrites every one.)
template <int LOG2A, int MODE, int KC = kcols_for(LOG2A)>
__global__ __launch_bounds__(KC * Plan<LOG2A>::TPT) void k_fft4_a(Fft4Args f) {
  using PL = Plan<LOG2A>;
  constexpr int NA = PL::N, NT = KC * PL::TPT, TS = PL::PADN + 1;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const FftArgs& a = f.a;
  const int64_t NB = f.N / NA;
  const int64_t b = blockIdx.y;
  // XCD-aware: the workgroups the dispatcher sends to one XCD (every 8th) take
  // consecutive column groups, so the two 64-byte halves of a 128-byte line
  // are fetched into the same L2
  int64_t gx = blockIdx.x;
  if ((gridDim.x & 7) == 0) gx = (gx & 7) * (gridDim.x >> 3) + (gx >> 3);
  const int64_t c0 = gx * KC;
  const InRow ir = in_row<MODE>(a, b);
  // every load of the tile issued before the first use (PER per thread, in
  // registers), then the non-finite scan, then LDS: a loop that stored each
  // value as it arrived waited out one HBM round trip per value (round 5)
  constexpr int PER = KC * NA / NT;
  static_assert(PER * NT == KC * NA, "tile split");
  float2 v[PER];
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int i = threadIdx.x + it * NT;
    v[it] = load_input<MODE>(a, ir, (int)(c0 + i % KC + NB * (i / KC)), true);
  }
  if (f.hdr) {
    // (the spectrum only flags: s * w is non-finite exactly when the sample s
    // is, w in [0, 1])
    bool nf = false;
#pragma unroll
    for (int it = 0; it < PER; ++it) {
      if (!__builtin_isfinite(v[it].x)) {
        nf = true;
        if constexpr (MODE != kSpec) v[it].x = 0.f;
      }
      if constexpr (MODE != kSpec) {
        if (!__builtin_isfinite(v[it].y)) {
          nf = true;
          v[it].y = 0.f;
        }
      }
    }
    if (nf) f.hdr[2 * b] = 1u;
  }
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int i = threadIdx.x + it * NT;
    lds[(i % KC) * TS + lpad(i / KC)] = v[it];
  }
  const int tl = threadIdx.x / PL::TPT, j0 = threadIdx.x - tl * PL::TPT;
  Tw<LOG2A, 0> tw;
  load_tw<LOG2A, 0>(tw, a.tw, j0, f.N / NA * f.tws);
  // The inter-step twiddles W_Nt^(n1 k2) of this thread's outputs: its column
  // n1 is fixed and k2 = r0 + it S, so three table values -- W^(n1 r0),
  // W^(n1 S), W^(4 n1 S) -- and products: W^(n1 (r0 + 4 q S)) by q - 1
  // multiplications by W^(4 n1 S), then W^(n1 S j), j = 1..3 (at most 6
  // roundings more than the table, ~4e-7; the passes' own twiddles chain up
  // to 15).  Their loads go out here, behind the passes' twiddles, so that
  // they are in flight under the passes (the barriers below wait for LDS
  // only).  Round 5: the epilogue loaded them itself, 4 outputs at a time --
  // 4 table round trips per tile, which held step A at ~2.1 TB/s against step
  // B's 4.6; fetched here as 4 anchors + W^(n1 S), 2^28 4.43 -> 3.55 ms; as
  // these 3, 3.38 ms (fewer scattered table reads).
  constexpr int S = NT / KC;
  static_assert(PER % 4 == 0 && NT % KC == 0, "twiddle anchors");
  const int c = threadIdx.x % KC, r0 = threadIdx.x / KC;
  const int64_t n1 = c0 + c;
  const TwLoad a0_l = tw_fetch(f, n1 * r0 * f.tws);
  const TwLoad s4_l = tw_fetch(f, n1 * 4 * S * f.tws);
  const TwLoad s1_l = tw_fetch(f, n1 * S * f.tws);
  lds_barrier();
  run_pass<LOG2A, 0>(LdsIO<NA>{lds + tl * TS}, lds + tl * TS, j0, tw);
  lds_barrier();
  const float2 s1 = tw_finish(s1_l), s2 = cmul(s1, s1), s3 = cmul(s2, s1), s4 = tw_finish(s4_l);
  float2 anc[PER / 4];
  anc[0] = tw_finish(a0_l);
#pragma unroll
  for (int q = 1; q < PER / 4; ++q) anc[q] = cmul(anc[q - 1], s4);
  float2* y = f.ws + b * f.N;
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int k2 = r0 + it * S;
    const float2 w0 = anc[it / 4];
    const float2 w = it % 4 == 0 ? w0 : cmul(w0, it % 4 == 1 ? s1 : it % 4 == 2 ? s2 : s3);
    y[(int64_t)k2 * NB + n1] = cmul(lds[c * TS + lpad(k2)], w);
  }
}

// Step B.  Nested (run_fft6_row, f.nest = the outer NA): the KC rows of a
// workgroup are one inner row r = blockIdx.y of KC consecutive outer rows k2 =
// blockIdx.x KC + c, so that the natural-order output k of (k2, r), X[k2 +
// nest k], is written in runs of KC consecutive addresses, and the workgroups
// that write the other halves of those lines are dispatched to the same XCD
// at the same time (blockIdx.x remapped as in step A).
template <int LOG2B, int MODE, int KC = kcols_for(LOG2B)>
__global__ __launch_bounds__(KC * Plan<LOG2B>::TPT) void k_fft4_b(Fft4Args f) {
  using PL = Plan<LOG2B>;
  constexpr int NB = PL::N, NT = KC * PL::TPT, TS = PL::PADN + 1;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  const FftArgs& a = f.a;
  const int64_t NA = f.N / NB;
  // source row of lane group c: ws + src0 + c * src_c; output k1 of it at
  // out0 + c * out_c + k1 * out_k (complex / magnitude units)
  int64_t src0, src_c, out0, out_c, out_k;
  if (f.nest) {
    int64_t gx = blockIdx.x;
    if ((gridDim.x & 7) == 0) gx = (gx & 7) * (gridDim.x >> 3) + (gx >> 3);
    const int64_t k2 = gx * KC, r = blockIdx.y;
    src0 = k2 * f.N + r * NB;
    src_c = f.N;
    out0 = k2 + f.nest * r;
    out_c = 1;
    out_k = f.nest * NA;
  } else {
    const int64_t b = blockIdx.y, r0 = (int64_t)blockIdx.x * KC;  // first k2 row
    src0 = b * f.N + r0 * NB;
    src_c = NB;
    out0 = b * a.ld_out + r0;
    out_c = 1;
    out_k = NA;
  }
  const float2* y = f.ws + src0;
  constexpr int PER = KC * NB / NT;
  static_assert(PER * NT == KC * NB, "tile split");
  float2 v[PER];
#pragma unroll
  for (int it = 0; it < PER; ++it) {  // all loads in flight before the first LDS write
    const int i = threadIdx.x + it * NT;
    v[it] = y[(i / NB) * src_c + (i % NB)];
  }
#pragma unroll
  for (int it = 0; it < PER; ++it) {
    const int i = threadIdx.x + it * NT;
    lds[(i / NB) * TS + lpad(i % NB)] = v[it];
  }
  const int tl = threadIdx.x / PL::TPT, j0 = threadIdx.x - tl * PL::TPT;
  Tw<LOG2B, 0> tw;
  load_tw<LOG2B, 0>(tw, a.tw, j0, f.N / NB * f.tws);
  __syncthreads();
  run_pass<LOG2B, 0>(LdsIO<NB>{lds + tl * TS}, lds + tl * TS, j0, tw);
  __syncthreads();
  // the spectrum keeps k <= N_outer / 2 (row-relative index: out - row base)
  const int64_t onh = f.N * (f.nest ? f.nest : 1) / 2;
  const int64_t rel0 = f.nest ? out0 : out0 - (int64_t)blockIdx.y * a.ld_out;
  for (int i = threadIdx.x; i < KC * NB; i += NT) {
    const int c = i % KC, k1 = i / KC;
    const int64_t d = c * out_c + k1 * out_k;
    const float2 v = lds[c * TS + lpad(k1)];
    if constexpr (MODE == kSpec) {
      if (rel0 + d <= onh) a.out[out0 + d] = cabsf_(v);
    } else {
      reinterpret_cast<float2*>(a.out)[out0 + d] = v;
    }
  }
}

template <int LOG2A, int LOG2B, int MODE>
int launch_fft4(const Fft4Args& f, hipStream_t s) {
  using PA = Plan<LOG2A>;
  using PB = Plan<LOG2B>;
  static_assert(LOG2A >= 4 && LOG2B >= LOG2A, "split");
  // step A's columns 16 wide (128-byte runs) where two images fit a CU's LDS:
  // batched 2^15 .. 2^18, 3.5-4.1 -> 4.1-4.3 TB/s (round 5,
  // profiles/r05_fft_large.txt); step B reads whole rows either way
  constexpr int KA = LOG2A <= 9 ? 16 : kcols_for(LOG2A), KB = kcols_for(LOG2B);
  const size_t sa = (size_t)KA * (PA::PADN + 1) * sizeof(float2);
  const size_t sb = (size_t)KB * (PB::PADN + 1) * sizeof(float2);
  if (int rc = allow_lds(k_fft4_a<LOG2A, MODE, KA>, sa)) return rc;
  if (int rc = allow_lds(k_fft4_b<LOG2B, MODE>, sb)) return rc;
  const unsigned rows = (unsigned)f.a.B;
  hipLaunchKernelGGL((k_fft4_a<LOG2A, MODE, KA>), dim3((unsigned)(PB::N / KA), rows),
                     dim3(KA * PA::TPT), sa, s, f);
  DSP_LAUNCHED("k_fft4_a");
  hipLaunchKernelGGL((k_fft4_b<LOG2B, MODE>), dim3((unsigned)(PA::N / KB), rows),
                     dim3(KB * PB::TPT), sb, s, f);
  DSP_LAUNCHED("k_fft4_b");
  return DSP_OK;
}

template <int MODE>
int dispatch4(const Fft4Args& f, int log2n, hipStream_t s) {
  switch (log2n) {
    case 15: return launch_fft4<7, 8, MODE>(f, s);
    case 16: return launch_fft4<8, 8, MODE>(f, s);
    case 17: return launch_fft4<8, 9, MODE>(f, s);
    case 18: return launch_fft4<9, 9, MODE>(f, s);
    case 19: return launch_fft4<9, 10, MODE>(f, s);
    case 20: return launch_fft4<10, 10, MODE>(f, s);
    case 21: return launch_fft4<10, 11, MODE>(f, s);
    case 22: return launch_fft4<11, 11, MODE>(f, s);  // (2^23 and up: run_fft6_row)
    default: return set_error(DSP_EINVAL, "log2n=%d outside [0, %d]", log2n, DSP_MAX_LOG2N_FOURSTEP);
  }
}

// Three-pass (nested) four-step from N = 2^23 up to 2^30 (round 5; the
// reference's recursion has no size limit, dsp_core.py:41-66): N = NA * NB
// with NB = NB1 * NB2, so that no sub-transform exceeds 2^11 points and every
// HBM access is a run of 8 or 16 consecutive complex values (the two-step
// split of 2^24 and up needs sub-transforms of 2^12..2^14, 4..1 columns):
//   step A   (k_fft4_a<LA>): the NB columns of NA points of the row, the
//            twiddle W_N^(n1 k2) on the way out -> Y[k2][n1] (rows of NB);
//   step A'  (k_fft4_a<LA1>, complex): the NA rows' columns of NB1 points
//            with W_NB = W_N^NA (table stride tws = NA) -> Y'[k2][..];
//   step B'  (k_fft4_b<LB2>, nest = NA): rows of NB2 points, 8 or 16 outer
//            rows k2 per workgroup, natural-order output k of row k2 ->
//            X[k2 + NA k].
// Steps A and B' touch HBM at megabyte strides, A' at kilobyte ones.  One row
// at a time (the workspace is 2 N complex whatever B).  From 2^23: the
// two-pass split's 2^12..2^14-point sub-transforms move 4..1 columns per
// access; with the twiddle loads under the passes (k_fft4_a) round 5 measured
// 0.092 vs 0.111 ms at 2^23, 0.211 vs 0.274 at 2^24 and the two-pass faster at
// 2^22, 0.052 vs 0.057 ms (profiles/r05_fft_large.txt).
constexpr int kLog2Nested = 23;
static_assert(kLog2Nested > DSP_MAX_LOG2N + 1 && kLog2Nested <= DSP_MAX_LOG2N_FOURSTEP, "nest from");

template <int LA, int LA1, int LB2, int MODE>
int run_fft6_row(const FftArgs& row, float2* Y, float2* Y2, const float2* twc, uint32_t* hdr,
                 hipStream_t s) {
  constexpr int64_t N = int64_t(1) << (LA + LA1 + LB2);
  constexpr int64_t NA = int64_t(1) << LA, NB = N / NA;
  // 16 columns (128-byte runs) for the two passes whose HBM side is strided
  // by megabytes where the LDS image fits twice per CU (up to 2^9 points):
  // tools/stride_probe.hip copies such columns at 4.4 TB/s in 128-byte runs,
  // 2.9 in 64-byte runs; the middle pass (kilobyte strides, 5.0) keeps 8
  constexpr int KA = LA <= 9 ? 16 : kCols, K1 = kcols_for(LA1);
  constexpr int KB = LB2 <= 9 ? 16 : kCols;
  static_assert(NA % KB == 0 && (NB >> LA1) % K1 == 0, "3-pass split");
  using PA = Plan<LA>;
  using P1 = Plan<LA1>;
  using PB = Plan<LB2>;
  const size_t sa = (size_t)KA * (PA::PADN + 1) * sizeof(float2);
  const size_t s1 = (size_t)K1 * (P1::PADN + 1) * sizeof(float2);
  const size_t sb = (size_t)KB * (PB::PADN + 1) * sizeof(float2);
  if (int rc = allow_lds(k_fft4_a<LA, MODE, KA>, sa)) return rc;
  if (int rc = allow_lds(k_fft4_a<LA1, kC2C>, s1)) return rc;
  if (int rc = allow_lds(k_fft4_b<LB2, MODE, KB>, sb)) return rc;
  Fft4Args fa{row, Y, N, hdr};
  fa.twc = twc;
  fa.tsh = tw_shift(LA + LA1 + LB2);
  hipLaunchKernelGGL((k_fft4_a<LA, MODE, KA>), dim3((unsigned)(NB / KA), 1), dim3(KA * PA::TPT),
                     sa, s, fa);
  DSP_LAUNCHED("k_fft4_a");
  // the inner transforms over the NA rows of Y: complex in, W_NB from the W_N
  // table at stride NA
  const FftArgs inner{reinterpret_cast<const float*>(Y), row.out, NA, NB, row.ld_out, 0, 0, 0, 1,
                      nullptr, row.tw};
  Fft4Args f1{inner, Y2, NB, nullptr};
  f1.tws = NA;
  f1.twc = twc;
  f1.tsh = fa.tsh;
  hipLaunchKernelGGL((k_fft4_a<LA1, kC2C>), dim3((unsigned)((NB >> LA1) / K1), (unsigned)NA),
                     dim3(K1 * P1::TPT), s1, s, f1);
  DSP_LAUNCHED("k_fft4_a");
  Fft4Args fb = f1;
  fb.nest = NA;
  hipLaunchKernelGGL((k_fft4_b<LB2, MODE, KB>), dim3((unsigned)(NA / KB), (unsigned)(NB >> LB2)),
                     dim3(KB * PB::TPT), sb, s, fb);
  DSP_LAUNCHED("k_fft4_b");
  return DSP_OK;
}

template <int MODE>
int dispatch6(const FftArgs& row, int log2n, float2* Y, float2* Y2, const float2* twc,
              uint32_t* hdr, hipStream_t s) {
  switch (log2n) {
    case 23: return run_fft6_row<7, 8, 8, MODE>(row, Y, Y2, twc, hdr, s);
    case 24: return run_fft6_row<8, 8, 8, MODE>(row, Y, Y2, twc, hdr, s);
    // the strided passes (A, B') at most 2^9 where the split allows (16
    // columns, 128-byte runs), the middle one takes the rest; round 5 measured
    // 4.93 -> 4.46 ms at 2^28 against an even split with 8 columns, 2^30's
    // 9 / 11 / 10 at 20.1 vs 20.7 ms for 10 / 10 / 10 (profiles/r05_fft_large.txt)
    case 25: return run_fft6_row<8, 9, 8, MODE>(row, Y, Y2, twc, hdr, s);
    case 26: return run_fft6_row<9, 8, 9, MODE>(row, Y, Y2, twc, hdr, s);
    case 27: return run_fft6_row<9, 9, 9, MODE>(row, Y, Y2, twc, hdr, s);
    case 28: return run_fft6_row<9, 10, 9, MODE>(row, Y, Y2, twc, hdr, s);
    case 29: return run_fft6_row<9, 11, 9, MODE>(row, Y, Y2, twc, hdr, s);
    case 30: return run_fft6_row<9, 11, 10, MODE>(row, Y, Y2, twc, hdr, s);
    default: return set_error(DSP_EINVAL, "log2n=%d outside the three-pass range", log2n);
  }
}

constexpr int64_t kMaxRows4 = 65535;  // grid y extent of the four-step kernels

// Four-step transform of B rows, in launches of <= kMaxRows4 rows.
template <int MODE>
int run_fft4_as(const FftArgs& a, int log2n, void* ws, size_t ws_bytes, hipStream_t s) {
  DSP_REQUIRE(log2n <= DSP_MAX_LOG2N_FOURSTEP, "log2n=%d outside [0, %d]", log2n,
              DSP_MAX_LOG2N_FOURSTEP);
  const size_t need = fourstep_workspace_bytes(a.B, log2n);
  DSP_REQUIRE(ws && ws_bytes >= need, "FFT workspace too small: %zu < %zu bytes", ws_bytes, need);
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "FFT workspace not 8-byte aligned");
  const int64_t B = a.B;
  const int64_t N = int64_t(1) << log2n;
  if (log2n >= kLog2Nested) {
    float2* Y = static_cast<float2*>(ws);
    float2* twc = Y + 2 * N;
    uint32_t* hdr = reinterpret_cast<uint32_t*>(twc + tw_coarse_bytes(log2n) / sizeof(float2));
    if (int rc = build_tw_coarse(a.tw, twc, log2n, s)) return rc;
    DSP_HIP(hipMemsetAsync(hdr, 0, (size_t)B * 2 * sizeof(uint32_t), s));
    for (int64_t b = 0; b < B; ++b) {
      FftArgs row = a;
      row.B = 1;
      row.in = a.in + b * a.ld_in * (MODE == kC2C ? 2 : 1);
      row.out = a.out + b * a.ld_out * (MODE == kSpec ? 1 : 2);
      if (int rc = dispatch6<MODE>(row, log2n, Y, Y + N, twc, hdr + 2 * b, s)) return rc;
      const NfArgs nfa{row.in, row.out, 1, row.ld_in, row.ld_out, row.seg_start, row.seg_len,
                       row.hop, row.frames, row.win, reinterpret_cast<const float*>(row.tw), MODE,
                       log2n};
      if (int rc = launch_nf_large(nfa, hdr + 2 * b, reinterpret_cast<uint64_t*>(Y), N, s))
        return rc;
    }
    return DSP_OK;
  }
  float2* twc = tw_coarse_bytes(log2n) ? static_cast<float2*>(ws) + B * N : nullptr;
  uint32_t* hdr = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + (size_t)B * N * 8 +
                                              tw_coarse_bytes(log2n));
  if (twc)
    if (int rc = build_tw_coarse(a.tw, twc, log2n, s)) return rc;
  for (int64_t b0 = 0; b0 < B; b0 += kMaxRows4) {
    FftArgs part = a;
    part.B = B - b0 < kMaxRows4 ? B - b0 : kMaxRows4;
    part.in = a.in + b0 * a.ld_in * (MODE == kC2C ? 2 : 1);
    part.out = a.out + b0 * a.ld_out * (MODE == kSpec ? 1 : 2);
    DSP_HIP(hipMemsetAsync(hdr, 0, (size_t)part.B * 2 * sizeof(uint32_t), s));
    Fft4Args f{part, static_cast<float2*>(ws), N, hdr};
    f.twc = twc;
    f.tsh = tw_shift(log2n);
    if (int rc = dispatch4<MODE>(f, log2n, s)) return rc;
    // the rows' non-finite inputs, listed in the freed Y rows
    const NfArgs nfa{part.in, part.out, part.B, part.ld_in, part.ld_out, part.seg_start,
                     part.seg_len, part.hop, part.frames, part.win,
                     reinterpret_cast<const float*>(part.tw), MODE, log2n};
    if (int rc = launch_nf_large(nfa, hdr, static_cast<uint64_t*>(ws), N, s)) return rc;
  }
  return DSP_OK;
}

}  // namespace

// Two-pass sizes: [Y: B x N complex][coarse twiddles][non-finite header: 2
// words per row of a launch part].  Three-pass (run_fft6_row, one row at a
// time): [Y: N][Y': N complex][coarse twiddles][header: 2 words per row].
// The coarse twiddle table (tw_fetch) above 2^20 points: 2^floor(log2n / 2)
// complex.
size_t fourstep_workspace_bytes(int64_t B, int log2n) {
  if (B <= 0 || log2n <= DSP_MAX_LOG2N || log2n > DSP_MAX_LOG2N_FOURSTEP) return 0;
  const bool three = log2n >= kLog2Nested;
  const size_t rows = three ? (size_t)B : (size_t)(B < kMaxRows4 ? B : kMaxRows4);
  const size_t data = mul_sat(three ? 2 : (size_t)B, (size_t)1 << log2n, sizeof(float2));
  return add_sat(add_sat(data, tw_coarse_bytes(log2n)), mul_sat(rows, 2, sizeof(uint32_t)));
}

// The FFT's workspace (dsp_fft_workspace_bytes): the four-step's for one
// transform, the radix-2 split's (fft_split.hip) above it -- the larger of the
// two where a test hook (dsp_fft_split_log2n) sends four-step sizes through
// the split.
size_t fft_workspace_bytes(int64_t B, int log2n) {
  if (B <= 0 || log2n <= DSP_MAX_LOG2N || log2n > DSP_MAX_LOG2N_FFT) return 0;
  const size_t four = fourstep_workspace_bytes(B, log2n);
  const size_t split = fft_takes_split(log2n) ? fft_split_workspace_bytes(log2n) : 0;
  return four > split ? four : split;
}

int run_fft4(const FftArgs& a, int mode, int log2n, void* ws, size_t ws_bytes, hipStream_t s) {
  return mode == kSpec   ? run_fft4_as<kSpec>(a, log2n, ws, ws_bytes, s)
         : mode == kR2C ? run_fft4_as<kR2C>(a, log2n, ws, ws_bytes, s)
                        : run_fft4_as<kC2C>(a, log2n, ws, ws_bytes, s);
}

}  // namespace dsp
