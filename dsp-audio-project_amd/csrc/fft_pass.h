// The in-LDS FFT pass code for gfx950 that every transform family shares:
// Stockham autosort passes of radix 16 held in registers, one LDS exchange per
// pass.  Included by fft.hip (k_fft, k_spec_real), fft_spec.hip (k_spec_stream,
// k_spec_wave12), fft_large.hip (the four-step), fft_dft.hip (Bluestein),
// stft_stream.hip (k_stft_stream) and, through fft_conv_common.h, fft_conv.hip
// (k_fastconv) and fft_pconv.hip (k_partconv_fwd, k_partconv_mac), and by
// nothing else.
//
// Algorithm (per transform of N = 2^log2n points):
//   passes p = 0..P-1 with radices R_p (16, except a first pass of 2, 4 or 8
//   when log2n is not a multiple of 4) and Ns = R_0 * ... * R_(p-1):
//     for every butterfly j < N/R_p, with m = j mod Ns:
//       v[r] = in[j + r*N/R_p] * W_N^(m*r*N/(Ns*R_p))      r < R_p
//       v    = DFT_R(v)                                    (registers)
//       out[(j - m)*R_p + m + r*Ns] = v[r]
//   The output is in natural order after the last pass (Stockham autosort).
// A radix-16 pass is a 4 x 4 split with compile-time W_16 constants, so a
// 4096-point transform is 3 LDS round trips instead of the 12 stages of a
// radix-2 kernel.  The first pass reads HBM directly (window and zero padding
// applied on load) and the last pass writes HBM directly (index j + r*Ns:
// coalesced), so the transform touches LDS P-1 times.
//
// LDS: one padded buffer per transform, element i at i + (i >> 4): pass-0
// writes (stride R) and the strided reads then spread over the 64 banks.
// Twiddles: w1 = W_N^(m*N/(Ns*R)) from the caller's fp64-computed table
// exp(-2*pi*i*k/N), k < N/2 (rounded to fp32), and w_r = w1^r by at most four
// complex products (error ~4 ulp, far inside the 1e-5 tolerance).
// Small transforms (N < 4096) pack 256 / (N/16) transforms per workgroup.
// The spectrum mode also runs a framed STFT: transform t = (row, frame) reads
// the window-weighted frame starting hop*frame samples into the row's segment.
#pragma once

#include <type_traits>

#include "common.h"

namespace dsp {

// (outside the unnamed namespace: the launchers below take it across units)
struct FftArgs {
  const float* in;     // real rows (kR2C, kSpec) or interleaved complex rows (kC2C)
  float* out;          // complex rows (kC2C, kR2C) or magnitudes (kSpec)
  int64_t B, ld_in, ld_out;      // B = transforms (rows x frames for kSpec)
  int64_t seg_start, seg_len;    // kSpec: valid samples [seg_start, seg_start + seg_len)
  int64_t hop, frames;           // kSpec: frame f of a row starts hop*f after seg_start
  const float* win;              // kSpec
  const float2* tw;              // exp(-2 pi i k / N), k < N/2
};

// The launchers that fft.hip's entry points reach in fft_spec.hip and (above
// 2^14 points; mode: an FftMode) fft_large.hip, each with its kernels' log2n switch.
int launch_spec_stream(const FftArgs& a, int log2n, hipStream_t s);
int launch_spec_wave12(const FftArgs& a, hipStream_t s);
int run_fft4(const FftArgs& a, int mode, int log2n, void* ws, size_t ws_bytes, hipStream_t s);

namespace {

enum FftMode { kC2C = 0, kR2C = 1, kSpec = 2 };

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float2 cadd(float2 a, float2 b) {
  return make_float2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ float2 csub(float2 a, float2 b) {
  return make_float2(a.x - b.x, a.y - b.y);
}
__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}

// Complex values as 2-float vectors: every add, product and fma below is one
// v_pk_*_f32 (a complex product is a pk_mul and a pk_fma with operand
// swizzles), half the VALU instructions of the float2-struct code.
typedef float pf2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pf2 pcmul(pf2 a, pf2 w) { return a.xx * w + a.yy * pf2{-w.y, w.x}; }
__device__ __forceinline__ pf2 pmi(pf2 a) { return pf2{a.y, -a.x}; }  // a * (-i)

// The same with register operands, spelled out: the compiler builds the
// swapped, negated copy of w ({-w.y, w.x}) with a move and an xor, where the
// VOP3P operand selects and negations do it for free.
//   a * w:      t = (a.x w.x, a.x w.y);  r = t + (-a.y w.y, a.y w.x)
//   s + d * w:  the same with s as the first accumulator
//   t -+ i d:   (t.x +- d.y, t.y -+ d.x)  (t + (-i) d and t - (-i) d)
__device__ __forceinline__ pf2 vcmul(pf2 a, pf2 w) {
  pf2 t, r;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(a), "v"(w));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
      : "=v"(r) : "v"(a), "v"(w), "v"(t));
  return r;
}
__device__ __forceinline__ pf2 vcfma(pf2 d, pf2 w, pf2 s) {
  pf2 t, r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(d), "v"(w), "v"(s));
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"
      : "=v"(r) : "v"(d), "v"(w), "v"(t));
  return r;
}
__device__ __forceinline__ pf2 vadd_mi(pf2 t, pf2 d) {
  pf2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(t), "v"(d));
  return r;
}
__device__ __forceinline__ pf2 vsub_mi(pf2 t, pf2 d) {
  pf2 r;
  asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(t), "v"(d));
  return r;
}


// Variable-twiddle products and the radix-4 butterfly through the packed
// helpers above (the float2 expressions made the compiler build each swapped,
// negated twiddle copy with a move and an xor).
__device__ __forceinline__ float2 cmulv(float2 a, float2 w) {
  const pf2 r = vcmul(pf2{a.x, a.y}, pf2{w.x, w.y});
  return make_float2(r.x, r.y);
}

// |v|.  sqrtf is correctly rounded, which the compiler expands around
// v_sqrt_f32 into ~14 instructions (denormal scaling and a two-sided fma
// correction); the bare instruction is within 1 ulp, 2^-23 relative, far inside
// the spectra's 1e-5 tolerance, and drops ~450 of the ~2900 VALU instructions
// a 4096-point magnitude spectrum takes per wave.
__device__ __forceinline__ float cabsf_(float2 v) {
  const float p = fmaf(v.x, v.x, v.y * v.y);
  return __builtin_amdgcn_sqrtf(p);
}

// a * W_16^q for a compile-time q (after unrolling); exact for q % 4 == 0.
__device__ __forceinline__ float2 w16mul(float2 a, int q) {
  constexpr float c1 = 0.92387953251128674f;  // cos(pi/8)
  constexpr float s1 = 0.38268343236508977f;  // sin(pi/8)
  constexpr float h = 0.70710678118654752f;   // sqrt(1/2)
  switch (q & 15) {
    case 0: return a;
    case 1: return cmul(a, make_float2(c1, -s1));
    case 2: return cmul(a, make_float2(h, -h));
    case 3: return cmul(a, make_float2(s1, -c1));
    case 4: return make_float2(a.y, -a.x);
    case 5: return cmul(a, make_float2(-s1, -c1));
    case 6: return cmul(a, make_float2(-h, -h));
    case 7: return cmul(a, make_float2(-c1, -s1));
    case 8: return make_float2(-a.x, -a.y);
    case 9: return cmul(a, make_float2(-c1, s1));
    case 10: return cmul(a, make_float2(-h, h));
    case 11: return cmul(a, make_float2(-s1, c1));
    case 12: return make_float2(-a.y, a.x);
    case 13: return cmul(a, make_float2(s1, c1));
    case 14: return cmul(a, make_float2(h, h));
    default: return cmul(a, make_float2(c1, s1));
  }
}

__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2);
  const float2 t2 = cadd(a1, a3), d = csub(a1, a3);
  a0 = cadd(t0, t2);
  a2 = csub(t0, t2);
  const pf2 r1 = vadd_mi(pf2{t1.x, t1.y}, pf2{d.x, d.y});  // t1 + (a1 - a3) * (-i)
  const pf2 r3 = vsub_mi(pf2{t1.x, t1.y}, pf2{d.x, d.y});
  a1 = make_float2(r1.x, r1.y);
  a3 = make_float2(r3.x, r3.y);
}

// In-place forward DFT of R points, natural order in and out.
template <int R>
__device__ __forceinline__ void dft(float2 (&v)[R]) {
  if constexpr (R == 2) {
    const float2 a = v[0];
    v[0] = cadd(a, v[1]);
    v[1] = csub(a, v[1]);
  } else if constexpr (R == 4) {
    dft4(v[0], v[1], v[2], v[3]);
  } else if constexpr (R == 8) {
    // n = 2 n1 + n2, k = k1 + 4 k2
    dft4(v[0], v[2], v[4], v[6]);
    dft4(v[1], v[3], v[5], v[7]);
    float2 o[8];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
      const float2 y0 = v[2 * k1], y1 = w16mul(v[2 * k1 + 1], 2 * k1);
      o[k1] = cadd(y0, y1);
      o[k1 + 4] = csub(y0, y1);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = o[i];
  } else if constexpr (R == 16) {
    // n = 4 n1 + n2, k = k1 + 4 k2
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) dft4(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
    // Y[n2][k1] sits at v[4 k1 + n2]
#pragma unroll
    for (int k1 = 1; k1 < 4; ++k1)
#pragma unroll
      for (int n2 = 1; n2 < 4; ++n2) v[4 * k1 + n2] = w16mul(v[4 * k1 + n2], n2 * k1);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) dft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
    float2 o[16];
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
      for (int k2 = 0; k2 < 4; ++k2) o[k1 + 4 * k2] = v[4 * k1 + k2];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = o[i];
  }
}

// ---------------------------------------------------------------------------
// Compile-time plan
// ---------------------------------------------------------------------------
template <int LOG2N>
struct Plan {
  static constexpr int N = 1 << LOG2N;
  static constexpr int NP = LOG2N == 0 ? 0 : (LOG2N + 3) / 4;
  static constexpr int RMAX = LOG2N >= 4 ? 16 : N;
  static constexpr int TPT = N / RMAX;                      // threads per transform
  static constexpr int TPB = TPT >= 256 ? 1 : 256 / TPT;    // transforms per block
  static constexpr int NT = TPB * TPT;
  static constexpr int PADN = N + (N >> 4);
  static constexpr int radix(int p) {
    return (p == 0 && (LOG2N & 3) != 0) ? (1 << (LOG2N & 3)) : RMAX;
  }
  static constexpr int ns(int p) { return p == 0 ? 1 : ns(p - 1) * radix(p - 1); }
};

__device__ __forceinline__ int lpad(int i) { return i + (i >> 4); }

// Where transform t reads its input: element n is in[base + n] (complex or real
// element units); kSpec frames also carry their valid length.
struct InRow {
  int64_t base;
  int64_t valid;  // kSpec: samples of the frame inside the segment
};

template <int MODE>
__device__ __forceinline__ InRow in_row(const FftArgs& a, int64_t t) {
  if constexpr (MODE == kSpec) {
    const int64_t row = a.frames == 1 ? t : t / a.frames;
    const int64_t f0 = (t - row * a.frames) * a.hop;  // frame start within the segment
    return InRow{row * a.ld_in + a.seg_start + f0, a.seg_len - f0};
  } else {
    return InRow{t * a.ld_in, 0};
  }
}

// Value n of the transform as the first pass reads it.
template <int MODE>
__device__ __forceinline__ float2 load_input(const FftArgs& a, const InRow& r, int n, bool live) {
  if (!live) return make_float2(0.f, 0.f);
  if constexpr (MODE == kC2C) {
    return reinterpret_cast<const float2*>(a.in)[r.base + n];
  } else if constexpr (MODE == kR2C) {
    return make_float2(a.in[r.base + n], 0.f);
  } else {
    const float s = (n < r.valid) ? a.in[r.base + n] : 0.f;
    return make_float2(s * a.win[n], 0.f);
  }
}

template <int MODE, int N>
__device__ __forceinline__ void store_output(const FftArgs& a, int64_t t, int k, float2 v,
                                             bool live) {
  if (!live) return;
  if constexpr (MODE == kSpec) {
    if (k <= N / 2) a.out[t * a.ld_out + k] = cabsf_(v);
  } else {
    reinterpret_cast<float2*>(a.out)[t * a.ld_out + k] = v;
  }
}

// w1 of every butterfly of pass P (the twiddle loads are issued before pass 0 so
// their latency hides under it instead of after each barrier).
template <int LOG2N, int P>
struct Tw {
  float2 w[Plan<LOG2N>::NP > P + 1 ? Plan<LOG2N>::RMAX / Plan<LOG2N>::radix(P + 1) : 1];
  Tw<LOG2N, P + 1> next;
};
template <int LOG2N>
struct Tw<LOG2N, 15> {};

// tstr: stride into the caller's table (2 when the table is for 2N points,
// N_total / N for a sub-transform of a four-step FFT).
template <int LOG2N, int P>
__device__ __forceinline__ void load_tw(Tw<LOG2N, P>& tw, const float2* __restrict__ table,
                                        int j0, int64_t tstr = 1) {
  using PL = Plan<LOG2N>;
  if constexpr (P + 1 < PL::NP) {
    constexpr int R = PL::radix(P + 1);
    constexpr int NS = PL::ns(P + 1);
#pragma unroll
    for (int b = 0; b < PL::RMAX / R; ++b) {
      const int m = (j0 + b * PL::TPT) & (NS - 1);
      tw.w[b] = table[(int64_t)m * (PL::N / (NS * R)) * tstr];
    }
    load_tw<LOG2N, P + 1>(tw.next, table, j0, tstr);
  }
}

// IO policies of a transform: load(n) feeds the first pass, store(k, v) takes
// the last pass's natural-order output.  kLdsIn: load() reads the LDS buffer
// the passes work in, so the first pass also waits before writing.
template <int MODE, int N>
struct GlobalIO {
  static constexpr bool kLdsIn = false;
  const FftArgs& a;
  InRow ir;
  int64_t t;
  bool live;
  __device__ __forceinline__ float2 load(int n) const { return load_input<MODE>(a, ir, n, live); }
  __device__ __forceinline__ void store(int k, float2 v) const {
    store_output<MODE, N>(a, t, k, v, live);
  }
};

// TWMODE, how a radix-16 pass forms w_r = w1^r: 0 by powering from w1 (w_r =
// w_(r-1) w1 or w_(r/2)^2); 1 (few live registers) w2, w4, w8 by squaring and
// w_r as the product of the powers in r's binary digits; 2 the same product
// with w2, w4, w8 read from the table as well (io.twiddles(), the table the Tw
// was loaded from at stride 1: 8 m N / (16 Ns) < N/2), so that no twiddle is
// more than three products away from correctly rounded values -- powering
// multiplies w1's rounding error by r.
template <int LOG2N, int P, class IO, int TWMODE = 0>
__device__ __forceinline__ void run_pass(const IO& io, float2* buf, int j0,
                                         const Tw<LOG2N, P - 1 < 0 ? 0 : P - 1>& tw) {
  constexpr bool LOWREG = TWMODE != 0;
  using PL = Plan<LOG2N>;
  constexpr int N = PL::N;
  constexpr int R = PL::radix(P);
  constexpr int NS = PL::ns(P);
  constexpr int NB = PL::RMAX / R;  // butterflies per thread
  constexpr int STRIDE = N / R;
  constexpr bool FIRST = P == 0, LAST = P == PL::NP - 1;
  float2 v[NB][R];
  float2 tp[NB][3];  // TWMODE 2: w2, w4, w8, in flight under the LDS reads
  if constexpr (TWMODE == 2 && NS > 1) {
    static_assert(R == 16, "passes after the first are radix 16");
    const float2* __restrict__ table = io.twiddles();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int i1 = ((j0 + b * PL::TPT) & (NS - 1)) * (N / (NS * R));
#pragma unroll
      for (int e = 0; e < 3; ++e) tp[b][e] = table[i1 << (e + 1)];
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int j = j0 + b * PL::TPT;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int n = j + r * STRIDE;
      v[b][r] = FIRST ? io.load(n) : buf[lpad(n)];
    }
  }
  // every read of this pass precedes its (in-place) writes (a barrier for LDS
  // only: one that also drained global loads would wait out the four-step's
  // twiddle loads that are meant to be in flight under the passes)
  if constexpr (!FIRST || IO::kLdsIn) lds_barrier();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int j = j0 + b * PL::TPT;
    const int m = j & (NS - 1);
    if constexpr (NS > 1 && !LOWREG) {
      float2 w[R];
      w[1] = tw.w[b];
#pragma unroll
      for (int r = 2; r < R; ++r) w[r] = (r & 1) ? cmulv(w[r - 1], w[1]) : cmulv(w[r / 2], w[r / 2]);
#pragma unroll
      for (int r = 1; r < R; ++r) v[b][r] = cmulv(v[b][r], w[r]);
    } else if constexpr (NS > 1) {
      // Few live registers: w1, w2, w4, w8 by squaring, w_r as the product of
      // the powers in r's binary digits, applied as soon as it is formed.
      float2 p2[4];
      p2[0] = tw.w[b];
#pragma unroll
      for (int e = 1; e < 4; ++e) {
        if constexpr (TWMODE == 2) p2[e] = tp[b][e - 1];
        else p2[e] = cmulv(p2[e - 1], p2[e - 1]);
      }
#pragma unroll
      for (int r = 1; r < R; ++r) {
        float2 w = make_float2(1.f, 0.f);
        bool first = true;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((r >> e) & 1) {
            w = first ? p2[e] : cmulv(w, p2[e]);
            first = false;
          }
        v[b][r] = cmulv(v[b][r], w);
      }
    }
    dft<R>(v[b]);
    const int base = (j - m) * R + m;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = base + r * NS;
      if constexpr (LAST) io.store(k, v[b][r]);
      else buf[lpad(k)] = v[b][r];
    }
  }
  if constexpr (!LAST) lds_barrier();
  if constexpr (P + 1 < PL::NP) {
    if constexpr (P == 0) run_pass<LOG2N, P + 1, IO, TWMODE>(io, buf, j0, tw);
    else run_pass<LOG2N, P + 1, IO, TWMODE>(io, buf, j0, tw.next);
  }
}

// Transform entirely in LDS (passes after the first, four-step sub-transforms).
template <int N>
struct LdsIO {
  static constexpr bool kLdsIn = true;
  float2* buf;
  __device__ __forceinline__ float2 load(int n) const { return buf[lpad(n)]; }
  __device__ __forceinline__ void store(int k, float2 v) const { buf[lpad(k)] = v; }
};

// The real split of a packed real-input transform (k_spec_real, k_spec_stream,
// k_stft_stream): buf holds the NH = N/2-point transform Z of z[n] = x[2n] +
// i x[2n+1], tw the table W_N^k, k < N/2, and with
//   E = (Z[k] + conj Z[NH-k]) / 2,  O = (Z[k] - conj Z[NH-k]) / (2i)
//   X[k] = E + W_N^k O,  X[NH-k] = conj(E - W_N^k O)
// thread j0 of the transform's TPT writes |X[k]|, |X[NH-k]| for k = j0, j0 + TPT,
// ... <= NH/2 to mr: one (k, NH-k) pair at a time, |X[NH]| = |Re Z[0] - Im Z[0]|.
template <int NH, int TPT>
__device__ __forceinline__ void real_split_mag(const float2* buf, const float2* tw, float* mr,
                                               int j0) {
  for (int k = j0; k <= NH / 2; k += TPT) {
    const float2 zk = buf[lpad(k)];
    const float2 zm = buf[lpad((NH - k) & (NH - 1))];
    const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    const float2 w = tw[k < NH ? k : 0];  // k <= NH/2 < N/2 always
    const float2 wo = cmulv(o, w);
    const float2 xk = cadd(e, wo), xm = csub(e, wo);
    mr[k] = cabsf_(xk);
    if (k > 0 && k < NH / 2) mr[NH - k] = cabsf_(xm);
    if (k == 0) mr[NH] = fabsf(zk.x - zk.y);
  }
}

// Host: the launch of a kernel whose workgroups hold PL::TPB transforms in LDS
// (PL::PADN complex each), one per PL::TPT threads: `transforms` of them, then
// `extra` more workgroups (k_stft_stream's carry copy; else 0).
template <class PL, class Kern, class... Args>
int launch_lds_resident(Kern kernel, const char* name, int64_t transforms, int64_t extra,
                        hipStream_t s, const Args&... args) {
  const size_t shm = (size_t)PL::TPB * PL::PADN * sizeof(float2);
  if (int rc = allow_lds(kernel, shm)) return rc;
  const unsigned grid = (unsigned)(ceil_div(transforms, PL::TPB) + extra);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(PL::NT), shm, s, args...);
  DSP_LAUNCHED(name);
  return DSP_OK;
}

// Host: f(std::integral_constant<int, L>{}) for L = log2n in [LO, HI], the
// launchers' switch over their kernels' template argument; DSP_ENOTSUP outside.
template <int LO, int HI, int L = LO, class F>
int dispatch_log2n(int log2n, F&& f) {
  if constexpr (L > HI) {
    return set_error(DSP_ENOTSUP, "log2n=%d outside [%d, %d]", log2n, LO, HI);
  } else {
    if (log2n == L) return f(std::integral_constant<int, L>{});
    return dispatch_log2n<LO, HI, L + 1>(log2n, f);
  }
}

}  // namespace
}  // namespace dsp
