// The two persistent magnitude-spectrum kernels for gfx950, which fft.hip's
// dispatch_spec sends their sizes: k_spec_stream, workgroups that walk their
// transforms with the next one's samples in flight, and the one-wave k_spec_wave12.
#include "fft_pass.h"

namespace dsp {
namespace {

// Streaming magnitude spectrum (round 3; the default for N = 2^6 .. 2^14 with a
// first pass of radix < 16): the same real-input transform as k_spec_real,
// but a persistent grid in which every workgroup walks its transforms in a
// loop and keeps the next transform's segment in flight while the current one
// runs its LDS passes, with 16-byte loads:
//   * pass 0 is remapped so that thread j0 owns the NB0 consecutive
//     butterflies NB0*j0 .. NB0*j0+NB0-1 (pass 0 has no twiddles, so any
//     butterfly-to-thread map works): for every r its inputs are NB0
//     consecutive complex values = 2*NB0 consecutive real samples, i.e. NB0/2
//     float4 loads per lane, contiguous across the wave;
//   * the window (the same for every transform) is re-read from L1/L2;
//   * the prefetched float4s of transform t+G are issued right after the
//     window multiply of transform t, so HBM latency hides under t's LDS
//     passes and split (the round-2 kernel issued each transform's loads only
//     when its workgroup started: SQ_WAIT_ANY / SQ_WAVE_CYCLES = 0.71).
// Rows whose segment start is not 16-byte aligned, or frames past the
// segment's end, take per-sample guarded loads (same values).
template <int LOG2N>
struct SpecStream {
  using PL = Plan<LOG2N - 1>;                 // the N/2-point complex transform
  static constexpr int N = 1 << LOG2N, NH = N / 2;
  static constexpr int R0 = PL::radix(0);
  static constexpr int NB0 = PL::RMAX / R0;    // pass-0 butterflies per thread
  static constexpr int S0 = NH / R0;           // pass-0 input stride (complex)
  static constexpr int NQ = NB0 / 2;           // float4s per r
  static_assert(NB0 >= 2 && NB0 % 2 == 0, "pass 0 needs >= 2 butterflies per thread");
};

// The transform's pass-0 samples as float4s through a raw buffer resource
// over its frame: one VGPR offset for all loads (the r strides go to the
// SGPR/immediate offsets), and bytes past the frame's valid samples -- or the
// whole frame of a dead transform -- read as zeros (the hardware checks every
// dword against num_records), which is the zero padding of dsp_core.py:81-82.
template <int LOG2N>
__device__ __forceinline__ void spec_stream_load(const FftArgs& a, const InRow& ir, bool live,
                                                 int j0, f32x4_t (&raw)[SpecStream<LOG2N>::NQ]
                                                                         [SpecStream<LOG2N>::R0]) {
  using SS = SpecStream<LOG2N>;
  const int64_t valid = live ? (ir.valid < SS::N ? (ir.valid > 0 ? ir.valid : 0) : SS::N) : 0;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) + (live ? ir.base : 0), 0, (int)(valid * 4), 0x00020000);
  const int vo = 4 * 2 * SS::NB0 * j0;  // bytes
#pragma unroll
  for (int r = 0; r < SS::R0; ++r)
#pragma unroll
    for (int q = 0; q < SS::NQ; ++q)
      raw[q][r] = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 4 * 2 * (2 * q + r * SS::S0), 2);
}

constexpr int kSpecWaves = 3;  // waves per SIMD the streaming kernel is compiled for
constexpr int kSpecTpbx = 2;   // transforms per workgroup (1: same at 32768 ch, 8 % slower at 4096)
template <int LOG2N, int TPBX>
__global__ __launch_bounds__(TPBX * Plan<LOG2N - 1>::TPT)
__attribute__((amdgpu_waves_per_eu(kSpecWaves))) void k_spec_stream(FftArgs a, int64_t units) {
  using SS = SpecStream<LOG2N>;
  using PL = typename SS::PL;
  constexpr int NH = SS::NH, R0 = SS::R0, NB0 = SS::NB0, NQ = SS::NQ;
  extern __shared__ __attribute__((aligned(16))) float2 lds[];
  int tl = threadIdx.x / PL::TPT;
  // A transform of >= 64 threads is whole waves: tl is wave-uniform, and saying
  // so keeps the frame's buffer resource in SGPRs (otherwise every buffer load
  // sits in a readfirstlane waterfall loop).
  if constexpr (PL::TPT % 64 == 0) tl = __builtin_amdgcn_readfirstlane(tl);
  const int j0 = threadIdx.x - tl * PL::TPT;
  float2* buf = lds + tl * PL::PADN;
  f32x4_t raw[NQ][R0];
  int64_t u = blockIdx.x;
  {
    const int64_t t = u * TPBX + tl;
    const bool live = u < units && t < a.B;
    spec_stream_load<LOG2N>(a, in_row<kSpec>(a, live ? t : 0), live, j0, raw);
  }
  for (; u < units; u += gridDim.x) {
    // An opaque copy of the thread's index per iteration: every LDS / table
    // address below depends only on it, and hoisting them out of the loop
    // costs ~120 VGPRs (206 vs 84 without the loop).
    int jj = j0;
    asm volatile("" : "+v"(jj));
    const int64_t t = u * TPBX + tl;
    const bool live = t < a.B;
    // window the transform's samples (packed even/odd as complex; the window
    // is re-read from L1/L2 here rather than held in 32 VGPRs across the
    // passes) ...
    // (opaque per-iteration table pointers: otherwise the loop-invariant
    // window and twiddle loads -- and the twiddle powers computed from them --
    // are hoisted out of the loop into ~100 VGPRs; they are L1 hits)
    const float* winp = a.win;
    const float2* twp = a.tw;
    asm volatile("" : "+s"(winp), "+s"(twp));
    Tw<LOG2N - 1, 0> tw;
    load_tw<LOG2N - 1, 0>(tw, twp, jj, 2);
    float2 v[NB0][R0];
#pragma unroll
    for (int r = 0; r < R0; ++r)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const f32x4_t w =
            *reinterpret_cast<const f32x4_t*>(winp + 2 * (NB0 * jj + 2 * q + r * SS::S0));
        const f32x4_t x = raw[q][r];
        v[2 * q][r] = make_float2(x.x * w.x, x.y * w.y);
        v[2 * q + 1][r] = make_float2(x.z * w.z, x.w * w.w);
      }
    // ... and put the next one in flight
    {
      const int64_t un = u + gridDim.x;
      const int64_t tn = un * TPBX + tl;
      const bool ln = un < units && tn < a.B;
      spec_stream_load<LOG2N>(a, in_row<kSpec>(a, ln ? tn : 0), ln, jj, raw);
    }
    // pass 0 (radix R0, no twiddles) into LDS in Stockham order
#pragma unroll
    for (int b = 0; b < NB0; ++b) {
      dft<R0>(v[b]);
      const int jb = NB0 * jj + b;
#pragma unroll
      for (int r = 0; r < R0; ++r) buf[lpad(jb * R0 + r)] = v[b][r];
    }
    __syncthreads();
    if constexpr (PL::NP > 1)
      run_pass<LOG2N - 1, 1, LdsIO<NH>, true>(LdsIO<NH>{buf}, buf, jj, tw);
    __syncthreads();  // the last pass stored Z into LDS
    if (live) real_split_mag<NH, PL::TPT>(buf, twp, a.out + t * a.ld_out, jj);
    __syncthreads();  // the split's LDS reads precede the next transform's pass 0
  }
}

template <int LOG2N>
int launch_spec_stream_n(const FftArgs& a, hipStream_t s) {
  using PL = Plan<LOG2N - 1>;
  constexpr int TPBX = kSpecTpbx;
  const size_t shm = (size_t)TPBX * PL::PADN * sizeof(float2);
  if (int rc = allow_lds(k_spec_stream<LOG2N, TPBX>, shm)) return rc;
  const int64_t units = ceil_div(a.B, TPBX);
  const int res = resident_groups<k_spec_stream<LOG2N, TPBX>>(TPBX * PL::TPT, shm);
  DSP_REQUIRE(res > 0, "occupancy query failed");
  const unsigned grid = (unsigned)(units < res ? units : res);
  hipLaunchKernelGGL((k_spec_stream<LOG2N, TPBX>), dim3(grid), dim3(TPBX * PL::TPT), shm, s, a,
                     units);
  DSP_LAUNCHED("k_spec_stream");
  return DSP_OK;
}

// One-wave 4096-point magnitude spectrum (round 3; the default for log2n = 12,
// the benchmark's n_fft).  A wave owns
// one transform at a time and never waits on another wave: the 2048 packed
// values c[n] = x[2n] w[2n] + i x[2n+1] w[2n+1] sit 32 per lane and the
// 2048-point transform is a 32 x 64 four-step split
//   n = 64 n1 + n2 (lane n2 holds n1 = 0..31),   k = k1 + 32 k2
//   A  B[n2][k1] = W_2048^(n2 k1) DFT32_n1(c[64 n1 + n2])         registers
//   T  lane L = 2 k1 + h takes Y[k1][2m + h], m < 32                LDS, 2 planes of 8 KB
//   B  F_h[j] = DFT32_m(...);  Z[k1 + 32 j] = F_0 + W_64^j F_1,
//      Z[k1 + 32 (j + 32)] = F_0 - W_64^j F_1                        registers + DPP pair swap
// so lane L ends with Z[K], K = k1 + 1024 h + 32 j (j < 32).  The real split
//   X[K] = s - i W_4096^K d,  s = Z[K] + conj Z[-K],  d = Z[K] - conj Z[-K]
// (with Z already halved: the 1/2 rides on the step-A twiddles) takes Z[-K]
// from lane (1 - L) mod 64, register 31 - j, by one bpermute per component;
// lanes 0 and 1, each other's partners at register 32 - j, take the previous
// bpermute's value (and their own Z at j = 0).  For fixed j, |X[K]| is two runs
// of 32 consecutive floats across the wave.  Per transform and lane: 32 sample
// loads (b64) and 5 twiddle loads, 32 window reads from the workgroup's LDS
// copy, 128 transpose accesses, 64 bpermutes, 64 DPP moves, 32 stores, no
// barrier: 35 % fewer VALU instructions than k_spec_stream's three LDS
// Stockham passes (which need a workgroup barrier each), DESIGN.md section 3.3.
constexpr int kWaveRow = 66;               // transpose row stride (floats): conflict-free both ways
constexpr int kWaveLds = 32 * kWaveRow;    // floats of LDS per wave
constexpr int kWavePerGroup = 16;         // one workgroup per CU (see k_spec_wave12)

// W_128^j = exp(-2 pi i j / 128) for a compile-time j in [0, 128).  oz: an
// opaque zero OR-ed into the bits, so that the constants are formed where they
// are used (SALU) instead of hoisted out of the caller's loop: hoisted, the
// wave kernel's ~100 constant SGPRs spilled through v_writelane/v_readlane,
// ~160 VALU instructions per transform.
__device__ __forceinline__ pf2 w128(int j, int oz = 0) {
  constexpr float c[33] = {
      1.000000000e+00f, 9.987954562e-01f, 9.951847267e-01f, 9.891765100e-01f,
      9.807852804e-01f, 9.700312532e-01f, 9.569403357e-01f, 9.415440652e-01f,
      9.238795325e-01f, 9.039892931e-01f, 8.819212643e-01f, 8.577286100e-01f,
      8.314696123e-01f, 8.032075315e-01f, 7.730104534e-01f, 7.409511254e-01f,
      7.071067812e-01f, 6.715589548e-01f, 6.343932842e-01f, 5.956993045e-01f,
      5.555702330e-01f, 5.141027442e-01f, 4.713967368e-01f, 4.275550934e-01f,
      3.826834324e-01f, 3.368898534e-01f, 2.902846773e-01f, 2.429801799e-01f,
      1.950903220e-01f, 1.467304745e-01f, 9.801714033e-02f, 4.906767433e-02f,
      0.0f};  // cos(pi j / 64)
  const float sgn = j < 64 ? 1.f : -1.f;  // W_128^(j+64) = -W_128^j
  j &= 63;
  const float cs = j <= 32 ? c[j] : -c[64 - j];
  const float sn = j <= 32 ? c[32 - j] : c[j - 32];
  return pf2{__int_as_float(__float_as_int(sgn * cs) | oz),
             __int_as_float(__float_as_int(-sgn * sn) | oz)};
}

// a * W_128^j for a compile-time j; exact for multiples of 32.
__device__ __forceinline__ pf2 pw128(pf2 a, int j, int oz = 0) {
  j &= 127;
  if (j == 0) return a;
  if (j == 32) return pmi(a);
  if (j == 64) return -a;
  if (j == 96) return -pmi(a);
  return pcmul(a, w128(j, oz));
}

__device__ __forceinline__ void pdft4(pf2& a0, pf2& a1, pf2& a2, pf2& a3) {
  const pf2 t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, d = a1 - a3;
  a0 = t0 + t2;
  a1 = vadd_mi(t1, d);
  a2 = t0 - t2;
  a3 = vsub_mi(t1, d);
}

// In-place 16- and 32-point DFTs, natural order in and out (dft<16>'s 4 x 4
// split; 32 = 2 x 16 with a radix-2 combine).
__device__ __forceinline__ void pdft16(pf2 (&v)[16], int oz = 0) {
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) pdft4(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
#pragma unroll
  for (int k1 = 1; k1 < 4; ++k1)
#pragma unroll
    for (int n2 = 1; n2 < 4; ++n2) v[4 * k1 + n2] = pw128(v[4 * k1 + n2], 8 * n2 * k1, oz);
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) pdft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
  pf2 o[16];
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) o[k1 + 4 * k2] = v[4 * k1 + k2];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = o[i];
}

__device__ __forceinline__ void pdft32(pf2 (&v)[32], int oz = 0) {
  pf2 e[16], o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    e[i] = v[2 * i];
    o[i] = v[2 * i + 1];
  }
  pdft16(e, oz);
  pdft16(o, oz);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const pf2 t = pw128(o[k], 4 * k, oz);
    v[k] = e[k] + t;
    v[k + 16] = e[k] - t;
  }
}

// Orders this wave's LDS accesses (they execute in order within a wave; this
// keeps the compiler from moving them across the exchange).
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float swap_pair(float v) {  // the value of lane L ^ 1
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float bperm(int addr, float v) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// Frame t's samples, lane's pairs (x[128 n1 + 2 lane], x[128 n1 + 2 lane + 1]),
// through a raw buffer resource over the frame: samples past the frame's valid
// range read as zeros (the zero padding of dsp_core.py:81-82).
__device__ __forceinline__ void wave_frame_load(const FftArgs& a, int64_t t, int lane,
                                                u32x2_t (&raw)[32]) {
  constexpr int N = 4096;
  const InRow ir = in_row<kSpec>(a, t);
  const int64_t valid = ir.valid < N ? (ir.valid > 0 ? ir.valid : 0) : N;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.in) + ir.base, 0, (int)(valid * 4), 0x00020000);
#pragma unroll
  for (int n1 = 0; n1 < 32; ++n1)
    raw[n1] = __builtin_amdgcn_raw_buffer_load_b64(rs, 8 * lane, 512 * n1, 2);
}

// The lane's index in its wave, recomputed (mbcnt) and opaque: a fresh copy
// per use site instead of one register live through the whole loop.
__device__ __forceinline__ int lane_now() {
  int l = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  asm volatile("" : "+v"(l));
  return l;
}

// One 4096-point transform t of the wave: raw = its frame's sample pairs
// (wave_frame_load), wl0 = the window in LDS, buf = the wave's transpose
// buffer.  Lane-derived values are recomputed (lane_now) in each phase
// instead of held through it: 4 waves per SIMD need <= 128 VGPRs.
__device__ __forceinline__ void w12_transform(const FftArgs& a, int64_t t, const u32x2_t (&raw)[32],
                                              const pf2* wl0, float* buf) {
  constexpr int N = 4096, NH = 2048;
  // (and of the window and twiddle addresses: hoisted, the window's 32 LDS
  // reads hold 64 VGPRs and the twiddles ~20)
  int z0 = 0;
  asm volatile("" : "+s"(z0));
  const pf2* win = wl0 + z0;
  pf2 v[32];
  const int l1 = lane_now();
  // (the window's LDS reads in groups of 8: all 32 in flight would hold 64
  // VGPRs beside the samples)
#pragma unroll
  for (int n1 = 0; n1 < 32; ++n1) {
    if (n1 % 8 == 0) asm volatile("" ::: "memory");
    v[n1] = pf2{__uint_as_float(raw[n1][0]), __uint_as_float(raw[n1][1])} * win[64 * n1 + l1];
  }
  // A: DFT over n1, then W_2048^(lane k1) / 2 (W_2048^m = W_4096^(2m); the
  // powers come from the table every 8 steps and by products in between)
  pdft32(v, z0);
  {
    // the step's twiddles, loaded only now (live through the DFT above
    // they cost ~10 VGPRs at its peak)
    int z1 = 0;
    asm volatile("" : "+s"(z1));
    const pf2* twp = reinterpret_cast<const pf2*>(a.tw) + z1;
    const int l2 = lane_now();
    const pf2 wl = twp[2 * l2];               // W_2048^lane
    pf2 w8[3];                                // W_2048^(8 lane k) / 2, k = 1..3
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const int m = (16 * l2 * k) & (N - 1);
      w8[k - 1] = (m < NH ? 0.5f : -0.5f) * twp[m & (NH - 1)];
    }
    pf2 p = 0.5f * wl;
    v[0] *= 0.5f;
#pragma unroll
    for (int k = 1; k < 32; ++k) {
      if (k % 8 == 0) {
        p = w8[k / 8 - 1];
      } else if (k > 1) {
        p = vcmul(p, wl);
      }
      v[k] = vcmul(v[k], p);
    }
  }
  // T: Y[k1][n2] -> lane 2 k1 + h reads Y[k1][2m + h], one plane at a time
  const int l3 = lane_now();
  const int rd = (l3 >> 1) * kWaveRow + (l3 & 1);  // transpose read base
  wave_lds_order();
#pragma unroll
  for (int k = 0; k < 32; ++k) buf[k * kWaveRow + l3] = v[k].x;
  wave_lds_order();
#pragma unroll
  for (int m = 0; m < 32; ++m) v[m].x = buf[rd + 2 * m];
  wave_lds_order();
#pragma unroll
  for (int k = 0; k < 32; ++k) buf[k * kWaveRow + l3] = v[k].y;
  wave_lds_order();
#pragma unroll
  for (int m = 0; m < 32; ++m) v[m].y = buf[rd + 2 * m];
  // B: DFT over m, then the radix-2 step across the lane pair: lane h = 1
  // scales its F_1 by W_64^j, the pair swaps, and Z = own * (+-1) + other
  pdft32(v, z0);
  const int l4 = lane_now();
  // (the lane's parity as an opaque float: the combine's 31 per-lane
  // twiddles are loop-invariant, and hoisting them would hold 62 VGPRs)
  const float hf = (float)(l4 & 1);
  const pf2 hh = pf2{hf, hf};
  const float sg = (l4 & 1) ? -1.f : 1.f;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    pf2 u = v[j];
    if (j > 0) {
      const pf2 one = pf2{1.f, 0.f};
      u = vcmul(u, one + hh * (w128(2 * j, z0) - one));  // h ? W_64^j : 1
    }
    v[j] = u * sg + pf2{swap_pair(u.x), swap_pair(u.y)};
  }
  // real split and |X[K]|; W_4096^K = W_4096^K0 W_128^j
  int z2 = 0;
  asm volatile("" : "+s"(z2));
  const int l5 = lane_now();
  const int src = ((1 - l5) & 63) << 2;     // bpermute address of Z[-K]'s lane
  const int K0 = (l5 >> 1) + 1024 * (l5 & 1);
  const pf2 wb = (reinterpret_cast<const pf2*>(a.tw) + z2)[K0];  // W_4096^K0
  float* mr = a.out + t * a.ld_out;
  pf2 prev = v[0];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const pf2 q = pf2{bperm(src, v[31 - j].x), bperm(src, v[31 - j].y)};
    const pf2 zm = l5 < 2 ? prev : q;
    prev = q;
    const pf2 zk = v[j];
    const pf2 sm = pf2{zk.x + zm.x, zk.y - zm.y};
    const pf2 d = pf2{zk.x - zm.x, zk.y + zm.y};
    const pf2 x = vcfma(d, pw128(wb, j + 32, z0), sm);  // s - i W d  (-i W_128^j = W_128^(j+32))
    mr[K0 + 32 * j] = cabsf_(make_float2(x.x, x.y));
  }
  if (l5 == 0) mr[NH] = 2.f * fabsf(v[0].x - v[0].y);  // X[N/2] = Re Z[0] - Im Z[0]
}

// A workgroup is a whole CU's 16 waves sharing one LDS copy of the window
// (16 KB + 16 transpose buffers = 151 KB), 4 waves per SIMD at <= 128 VGPRs
// (lane-derived values recomputed per phase, twiddles loaded where used; 4
// VGPRs spill, 20 B per lane); round 3's 4-wave groups held the LDS to 3
// groups = 3 waves per SIMD: 0.190 vs 0.1955 ms at config 4, 0.0295 vs 0.030
// at config 3 (profiles/r04_spec_ab.txt).  Measured and not adopted: the next
// frame in flight in 64 more VGPRs (2 waves per SIMD): 0.211 vs 0.193 ms at
// config 4 (round 3: 0.199 vs 0.194; profiles/r05_spec_pf_ab.txt); the waves
// of a SIMD starting 0.25 .. 1.5 us apart (round 5) or 4 .. 12 us apart (round
// 4): neutral / slower.  The memory-only floor of this launch (frame loads
// and |X| stores, no transform) is 0.166 ms at config 4 and 22.6 us at config
// 3, against 0.194 / 0.0305 ms with the transform (profiles/r05_spec_floor.txt).
__global__ __launch_bounds__(64 * kWavePerGroup) void k_spec_wave12(FftArgs a) {
  constexpr int N = 4096;
  extern __shared__ __attribute__((aligned(16))) float ldsf[];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the window, once per workgroup (LDS latency instead of an L2 round trip
  // per transform), then one transpose buffer per wave
  for (int i = threadIdx.x; i < N / 4; i += 64 * kWavePerGroup)
    reinterpret_cast<f32x4_t*>(ldsf)[i] = reinterpret_cast<const f32x4_t*>(a.win)[i];
  __syncthreads();
  const pf2* wl0 = reinterpret_cast<const pf2*>(ldsf);
  float* buf = ldsf + N + wv * kWaveLds;
  const int64_t nw = (int64_t)gridDim.x * kWavePerGroup;
  u32x2_t raw[32];
  for (int64_t t = (int64_t)blockIdx.x * kWavePerGroup + wv; t < a.B; t += nw) {
    wave_frame_load(a, t, lane_now(), raw);
    w12_transform(a, t, raw, wl0, buf);
  }
}

}  // namespace

int launch_spec_stream(const FftArgs& a, int log2n, hipStream_t s) {
  switch (log2n) {  // sizes whose packed transform's first pass has radix < 16
    case 6: return launch_spec_stream_n<6>(a, s);
    case 7: return launch_spec_stream_n<7>(a, s);
    case 8: return launch_spec_stream_n<8>(a, s);
    case 10: return launch_spec_stream_n<10>(a, s);
    case 11: return launch_spec_stream_n<11>(a, s);
    case 14: return launch_spec_stream_n<14>(a, s);
    default: return set_error(DSP_EINVAL, "no streaming spectrum kernel for log2n=%d", log2n);
  }
}

int launch_spec_wave12(const FftArgs& a, hipStream_t s) {
  const size_t shm = (size_t)(4096 + kWavePerGroup * kWaveLds) * sizeof(float);
  if (int rc = allow_lds(k_spec_wave12, shm)) return rc;
  const int res = resident_groups<k_spec_wave12>(64 * kWavePerGroup, shm);
  DSP_REQUIRE(res > 0, "occupancy query failed");
  const int64_t groups = ceil_div(a.B, kWavePerGroup);
  const unsigned grid = (unsigned)(groups < res ? groups : res);
  hipLaunchKernelGGL(k_spec_wave12, dim3(grid), dim3(64 * kWavePerGroup), shm, s, a);
  DSP_LAUNCHED("k_spec_wave12");
  return DSP_OK;
}

}  // namespace dsp
