// Single-pass SRC -> biquad cascade, the default path of dsp_chain_f32 (gfx950).
//
// Replaces, for a batch of channels, reference app.py:164-167:
//   y = conversion_tasa_muestreo(x, fs, M, L)   modules/dsp_core.py:133-173
//   z = sistema_ecualizador(y, fs', gains)      modules/dsp_core.py:216-254
// in ONE launch that reads x once and writes y and z once: HBM traffic is the
// algorithmic 4*N_in + 8*N_out bytes per channel, against 4*N_in + 4*N_out
// (SRC kernel) + 4*N_in*rows/shift + 8*N_out (two-pass cascade) for the
// two-launch chain.
//
// Decomposition.  A workgroup is ONE wavefront and owns a tile of 64*TSUB
// consecutive outputs of one channel; lane l owns the sub-chunk of TSUB
// outputs l*TSUB .. l*TSUB + TSUB-1 of the tile, TSUB = 32*L/M, i.e. exactly
// 32 new input samples per lane.  Because TSUB*M is a multiple of L, every
// lane (and every tile) sees the same polyphase pattern: output i of a
// sub-chunk reads x[32*l + qi(i) - t] with branch phi(i) (compile-time), so
// the taps are wave-uniform (scalar loads) and each lane runs
//   1. SRC: y[i] = sum_u P[phi(i)][TT-1-u] * w[qi(i) + u] from its 72-sample
//      window, read from the tile's x window in LDS (one coalesced load per
//      tile, padded so the 64 lanes' ds_read_b128 are conflict-free).  Same
//      per-output FMA order as k_src_reg: y is bitwise the SRC kernel's.
//   2. pass 1: the sub-chunk's zero-state end state.  The sums run in float32
//      (v_pk_fma_f32, 6 per sample) in INPUT-NORMAL coordinates xi = P^-1 w
//      (P P^T = the cascade's state covariance under unit white noise, so every
//      coordinate has unit variance and the float32 sums do not cancel):
//      e_l = sum_i Gc[i] y[i], Gc[i] = P^-1 A^(TSUB-1-i) B (wave-uniform);
//      then one float64 change of basis E'_l = Q e_l, Q = T^-1 P (lower
//      triangular, 78 FMAs per lane), into block-diagonal coordinates (below);
//   3. carry: the tile's entry state m_in comes from the previous tile of the
//      same channel (chained hand-off, below); a blocked scan of the 64
//      lanes' E' through LDS (tile_cascade) gives every sub-chunk's entry
//      state m_l = v_(l-1), v_l = D^TSUB v_(l-1) + E'_l, v_(-1) = m_in;
//   4. v_63 (the tile's end state) is published for the next tile;
//   5. y leaves through LDS as coalesced float4 stores; the lane's DF2 state
//      is s_l = T m_l and pass 2 reruns the cascade over the sub-chunk from it,
//      clips, and z leaves the same way.
//
// Block-diagonal coordinates.  The cascade's state matrix A is block lower
// triangular (stage k is driven by stage k-1's output) with 2x2 diagonal
// blocks A_kk.  With T block unit lower triangular solving A T = T D,
// D = diag(A_kk) (Sylvester equations A_ii X - X A_jj = C for the off-diagonal
// blocks, solvable when no two stages share a pole pair), A^N = T D^N T^-1 and
// powers of D are six independent 2x2 powers: the carry costs 4 FMAs per block
// per scan level instead of a dense 12x12 product.  Stages that only pad the
// cascade to six (exact identities) have states no output depends on; their
// coordinates are dropped.  The host computes T, D's powers and checks the
// conditioning in float64; a cascade without a well-conditioned T takes the
// two-launch chain.
// y never returns from HBM, and there is no second pass over x.
//
// Chained hand-off.  Workgroups are numbered tile-major (id = tile*B + b), so
// tile t-1 of a channel was dispatched B workgroups before tile t; at B >= the
// chip's resident wave count its end state is normally published long before
// tile t needs it.  A workgroup waits only on a lower id, and ids are
// dispatched in order, so every wait ends.  The state (12 doubles) and its
// flag are agent-scope atomics (global loads/stores with sc1: coherent at
// device scope across the XCDs' L2s, per location).  The producer lane stores
// the payload, waits vmcnt(0) (every payload store acknowledged) and only then
// stores the flag; the consumer polls the flag and issues the payload loads
// only after a poll returned 1 (a control dependency on a returned value, and
// asm memory clobbers keep the compiler from hoisting them).  Ordering between
// the payload and the flag therefore rests on the gfx950 ISA, not on C++
// release/acquire: the memory model's agent-scope release/acquire fences add
// buffer_wbl2 sc1 / buffer_inv sc1 (L2 write-back / invalidate), which the
// atomics do not need and which measured 5.8x slower (config 4: 37.7 vs
// 6.55 ms, profiles/r03_handoff_fence_ab.txt).  The consumer clears the flag, so a completed launch leaves
// the flag array zero for the next one (the caller zero-fills the workspace
// once).  Round 4: the producer raises its flag once the state stores are
// acknowledged but after its y stores are issued (a counted vmcnt), and
// k_chain_tile's consumer polls once before its x window loads: if the flag
// is already up (the common case: the producer ran a dispatch generation
// earlier), the state comes by an sc1 LDS-DMA issued after that poll, behind
// the SRC and pass 1 (chain_tile_body); else it waits as described.  A wait that polls more than the thread's spin limit
// (dsp_chain_spin_limit; default 2^23 polls with s_sleep 2 between them,
// ~0.4 s: a broken dispatch order, or a GPU time-sliced between processes)
// gives up: it sets the workspace's status word (dsp_chain_status reports it,
// Chain.run raises) and leaves the flag for the workspace reset; z of that
// launch is wrong, nothing hangs.
//
// Rows are bitwise independent of the batch size: the geometry depends on
// (L, M, K) only.  Where a row's last tile fills at most half a wave, the last
// tiles of two channels share one (k_chain_tile_pair, below): per lane the
// same arithmetic, so the same rows.
//
// This file holds the kernels and their launcher (launch_chain_tile); the host
// planner (which kernel, which mode by default, the tables) is chain_plan.hip.
#include <algorithm>

#include "cascade.h"
#include "chain_plan.h"
#include "chain_pp.h"
#include "chain_tile.h"

namespace dsp {
namespace {

// One tile of the L3/M2 kernel (REPAIR: the rerun with the non-finite path).
// MODE: 0 the chained hand-off, 1 / 2 launch 1 / 3 of the three-launch mode
// (chain_tile.h, AggEntry / GivenEntry).
template <class GEO, bool DLY, bool REPAIR, int MODE = 0>
__device__ __forceinline__ void chain_tile_body(const TileArgs& a, float* lds, int lane, int64_t b,
                                                int64_t tile) {
  constexpr int TS = GEO::TSUB;
  const int64_t m0 = tile * GEO::TILE;  // first output of the tile
  const tt_ptr mt = (tt_ptr)a.tt;       // wave-uniform: scalar loads

  // Early hand-off (not in the repair rerun): lane 0 polls the previous
  // tile's flag once now, ahead of the x window loads; if it is raised, the
  // state follows by an agent-scope (sc1) LDS-DMA into the slot after the
  // window -- issued after the poll returned, as the hand-off protocol
  // requires -- and arrives behind the SRC and pass 1 instead of two global
  // round trips after them.  Otherwise tile_cascade waits as before.
  uint32_t fl = 0;
  if (!REPAIR && MODE == 0 && tile > 0 && lane == 0)
    fl = load_flag(a.flags + b * a.ntiles + tile - 1);

  // ---- x window of the tile -> padded LDS image (x == 0 outside [0, n_in))
  {
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + b * a.ld_x, 0, (int)(a.n_in * 4), 0x00020000);
    const int64_t xs0 = m0 * GEO::M / GEO::L + a.cq - (GEO::TT - 1);  // multiple of 4
    constexpr int NF = GEO::NWIN / 4;
    // The lane's float4s f = lane + 64 k: buffer byte (xs0 + 4 f) * 4 = off0 +
    // 1024 k and LDS float xpad(4 f) = l0 + 288 k (lane < 64), one address
    // register each with k in the instructions' offsets.
    const int off0 = (int)(xs0 * 4) + 16 * lane;
    float* const l0 = lds + 4 * lane + 4 * (lane >> 3);
#pragma unroll
    for (int k = 0; k < (NF + kWave - 1) / kWave; ++k) {
      if ((k + 1) * kWave <= NF || lane + kWave * k < NF) {
        // "Negative" offsets (tile 0) are >= 2^31 as unsigned: out of range, zeros.
        const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx, off0 + 1024 * k, 0, kStream);
        *reinterpret_cast<f32x4*>(l0 + 288 * k) = v;
      }
    }
    static_assert(xpad(4 * (kWave + 7)) - xpad(4 * 7) == 288, "xpad: 288 floats per 64 float4s");
  }
  fence();  // one wave: its LDS operations execute in order
  EarlyEntry early{false, reinterpret_cast<const double*>(lds + GEO::LDSF)};
  if (!REPAIR && MODE == 0 && tile > 0 && __builtin_amdgcn_readfirstlane(fl) == 1u) {
    early.early = true;
    if (lane < 2 * kD) {
      const int64_t prev = b * a.ntiles + tile - 1;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint32_t*>(
                                                               a.states + prev * kD) + lane),
          (__attribute__((address_space(3))) void*)(lds + GEO::LDSF), 4, 0, kSc1);
    }
  }

  // ---- 1. SRC: the lane's TSUB outputs, in parts (register pressure)
  float y[TS];
  {
    const float* xw = lds + 36 * lane;
    static_assert(TS == 48, "SRC parts of 48 / 24 outputs");
    // DLY: one part of 48 (its delay outputs need no accumulators: 128 VGPRs,
    // no scratch); the plain kernel in two parts of 24 (one part would spill).
    if constexpr (DLY) {
      src_part<GEO, 0, 48, true>(xw, mt, y);
      pin(y);
    } else {
      src_part<GEO, 0, 24, false>(xw, mt, y);
      pin(y);
      src_part<GEO, 24, 24, false>(xw, mt, y);
      pin(y);
    }
  }
  if constexpr (REPAIR) {
    // each output's reference sums over its window (window_sums, nf_fix)
    auto fix = [&](float (&yy)[TS], double (&v)[kD]) {
      const float thr = mt->flush_thr;
      fix_outputs(a, mt, b, m0 + TS * lane, yy, v, [&](int i, float& nf, float& fin) {
        const int j = i * GEO::M + GEO::CR;
        const int base = kLS * lane + j / GEO::L + GEO::TT - 1;  // window offset of x[q]
        // (window starts and q keep x's absolute parity: xs0 is a multiple of 4)
        window_sums(a.taps, a.K, GEO::L, j % GEO::L, thr, base,
                    [&](int t) { return lds[xpad(base - t)]; }, nf, fin);
      });
    };
    tile_cascade<TS, true, true>(a, mt, lds, y, lane, b, tile, m0, fix);
  } else if constexpr (MODE == 1) {
    tile_cascade<TS>(a, mt, lds, y, lane, b, tile, m0, 0, AggEntry{});
  } else if constexpr (MODE == 2) {
    tile_cascade<TS>(a, mt, lds, y, lane, b, tile, m0, 0, GivenEntry{});
  } else {
    tile_cascade<TS>(a, mt, lds, y, lane, b, tile, m0, 0, early);
  }
}

template <class GEO, bool DLY = false>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4))) void k_chain_tile(
    TileArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[GEO::LDSF + 2 * kD];  // + the early slot
  // grid (B, ntiles): linear ids tile-major (x fastest), no division
  const int64_t tile = blockIdx.y, b = blockIdx.x;
  chain_tile_body<GEO, DLY, false>(a, lds, threadIdx.x, b, tile);
}

// The paired tail tile (chain_tile.h, PairEntry).  A row's last tile often
// fills under half of its wave (config 3/4: 72000 outputs = 23 tiles + 28 of
// 64 sub-chunks), and chain_tile_body has no per-lane exit: the idle lanes run
// the whole tile on zeros.  Here one wave carries the last tiles of channels b
// (lanes 0-31) and b2 (lanes 32-63), launched after k_chain_tile has run the
// other ntiles - 1 tiles of every channel (launch_chain_tile).
//
// x image: half 0's lanes keep chain_tile_body's windows (lane l at image
// float 32 l), read from b's row up to image float kXB = 1088, past lane 31's
// window end 32 * 31 + W = 1064; half 1's windows follow from kXB on (lane
// 32 + j at kXB + 32 j), read from b2's row at the same xs0.  So no lane of a
// half ever sees a sample of the other channel, and every lane's window is
// what it would be in a wave of the channel's own (zeros past the row's end).
template <class GEO>
struct PairGeo {
  // half 0's image, whole 32-float rows of the padding (xpad): 1088 floats
  static constexpr int XB = (kLS * (kWave / 2 - 1) + GEO::W + 31) / 32 * 32;
  static_assert(xpad(XB + kLS) - xpad(XB) == 36, "half 1's lane windows 36 floats apart");
  static constexpr int NWIN = (XB + kLS * (kWave / 2 - 1) + GEO::W + 3) / 4 * 4;
  static constexpr int XF = xpad(NWIN + 4) + 4;
  static constexpr int LDSF0 = XF > GEO::LDSF ? XF : GEO::LDSF;
  static constexpr int LDSF = LDSF0 > kScanFloatsPair ? LDSF0 : kScanFloatsPair;
  static constexpr int SLOT = kWave;  // floats of the two early slots (16 doubles each, 12 used)
};

template <class GEO, bool DLY>
__device__ __forceinline__ void chain_tile_pair_body(const TileArgs& a, float* lds, int lane,
                                                     int64_t b, int64_t b2, bool has2) {
  typedef PairGeo<GEO> PG;
  constexpr int TS = GEO::TSUB;
  const int64_t tile = a.ntiles - 1;
  const int64_t m0 = tile * GEO::TILE;
  const tt_ptr mt = (tt_ptr)a.tt;
  const int hf = lane >> 5;
  const int64_t bx = has2 ? b2 : b;  // (no b2: its addresses are b's, never stored to)

  // Early poll of each half's hand-off flag (chain_tile_body), lanes 0 and 32.
  uint32_t fl = 0;
  if (tile > 0 && (lane & 31) == 0 && (!hf || has2))
    fl = load_flag(a.flags + (hf ? b2 : b) * a.ntiles + tile - 1);

  // ---- the two x windows -> one padded LDS image
  {
    const __amdgpu_buffer_rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + b * a.ld_x, 0, (int)(a.n_in * 4), 0x00020000);
    // (no second channel: an empty resource, every load gives zeros)
    const __amdgpu_buffer_rsrc_t rx1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + bx * a.ld_x, 0, has2 ? (int)(a.n_in * 4) : 0, 0x00020000);
    const int64_t xs0 = m0 * GEO::M / GEO::L + a.cq - (GEO::TT - 1);  // multiple of 4
    constexpr int NF = PG::NWIN / 4, NA = PG::XB / 4;
    const int off0 = (int)(xs0 * 4) + 16 * lane;
    float* const l0 = lds + 4 * lane + 4 * (lane >> 3);
#pragma unroll
    for (int k = 0; k < (NF + kWave - 1) / kWave; ++k) {
      // float4 f = lane + 64 k of the image: b's row below NA, b2's from NA on
      const int f = lane + kWave * k;
      if (k * kWave < NA && ((k + 1) * kWave <= NA || f < NA)) {
        const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx0, off0 + 1024 * k, 0, kStream);
        *reinterpret_cast<f32x4*>(l0 + 288 * k) = v;
      }
      if ((k + 1) * kWave > NA && (k * kWave >= NA || f >= NA) &&
          ((k + 1) * kWave <= NF || f < NF)) {
        const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rx1, off0 + 1024 * k - 4 * PG::XB, 0,
                                                              kStream);
        *reinterpret_cast<f32x4*>(l0 + 288 * k) = v;
      }
    }
  }
  fence();
  PairEntry entry{{false, false}, reinterpret_cast<const double*>(lds + PG::LDSF), b2, has2};
  if (tile > 0) {
    entry.early[0] = __builtin_amdgcn_readlane(fl, 0) == 1u;
    entry.early[1] = __builtin_amdgcn_readlane(fl, 32) == 1u;
    if (entry.early[0] || entry.early[1]) {
      // One LDS-DMA of all 64 lanes (the destination is the slot + 4 lane
      // bytes): lane 32 h + j brings dword j of half h's state, j < 24; the
      // other lanes repeat dwords 0-7 into the slot's unused tail.  A half
      // whose flag was not up yet loads too and ignores what it got.
      const int64_t prev = (hf ? bx : b) * a.ntiles + tile - 1;
      const int j = lane & 31;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(reinterpret_cast<const uint32_t*>(
                                                               a.states + prev * kD) +
                                                           (j < 2 * kD ? j : j - 2 * kD)),
          (__attribute__((address_space(3))) void*)(lds + PG::LDSF), 4, 0, kSc1);
    }
  }

  // ---- 1. SRC (chain_tile_body's): half 1's windows start at image float XB
  float y[TS];
  {
    const float* xw = lds + 36 * lane + hf * (xpad(PG::XB) - 36 * (kWave / 2));
    static_assert(TS == 48, "SRC parts of 48 / 24 outputs");
    if constexpr (DLY) {
      src_part<GEO, 0, 48, true>(xw, mt, y);
      pin(y);
    } else {
      src_part<GEO, 0, 24, false>(xw, mt, y);
      pin(y);
      src_part<GEO, 24, 24, false>(xw, mt, y);
      pin(y);
    }
  }
  tile_cascade<TS>(a, mt, lds, y, lane, b, tile, m0, 0, entry);
}

template <class GEO, bool DLY = false>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4))) void
k_chain_tile_pair(TileArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[PairGeo<GEO>::LDSF + PairGeo<GEO>::SLOT];
  const int64_t b = 2 * (int64_t)blockIdx.x;
  chain_tile_pair_body<GEO, DLY>(a, lds, threadIdx.x, b, b + 1, b + 1 < a.B);
}

// Launches 1 and 3 of the three-launch mode (chain_tile.h, AggEntry).
template <class GEO, bool DLY, int MODE>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(4))) void k_chain_tile3(
    TileArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[GEO::LDSF];
  chain_tile_body<GEO, DLY, false, MODE>(a, lds, threadIdx.x, blockIdx.x, blockIdx.y);
}

template <class GEO, bool DLY = false>
__global__ __launch_bounds__(kWave) void k_chain_tile_repair(TileArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[GEO::LDSF + 2 * kD];  // + the early slot
  repair_channels(a, 0, 1, [&](int64_t b, int64_t tile) {
    chain_tile_body<GEO, DLY, true>(a, lds, (int)threadIdx.x, b, tile);
  });
}

// ---------------------------------------------------------------------------
// Generic single-pass kernel: any L, M with ceil(K/L) <= 8 (config 5's
// L/M = 160/147, K = 1023: 7 taps per branch) and at most 8 phase classes.
// The polyphase branch of a lane's outputs changes from output to output and
// from lane to lane:
//   j = m*M + c, phi = j mod L, q = j div L,
//   y[m] = sum_u h[phi][u] x[q - (T-1) + u],  h[phi][u] = taps[phi + L(T-1-u)],
// summed as k_src_generic does (even u and odd u in two chains, y = even +
// odd), so y is bitwise that kernel's.  Sub-chunks start at outputs m = 32 j,
// and their branch sequences repeat with j mod C, C = L / gcd(32 M mod L, L)
// (5 for 160/147): the host tabulates every class's 32 rows of taps and its
// q-advance bits (TileTables::seq/adv), so a lane's taps for output i sit at a
// compile-time offset of its class row and the SRC does no phase arithmetic.
// A workgroup is kGenWaves waves, one channel each at the same tile index
// (ids stay tile-major for the hand-off); they share the class tables in LDS.
// Each wave owns its x window (and stages its stores through it).  Steps 2-5
// are tile_cascade<32>.
// ---------------------------------------------------------------------------
// The generic kernels' workgroup: kGenWaves waves, wave w takes channel
// g kGenWaves + w of channel group g; the ids are tile-major over groups.
__device__ __forceinline__ int gen_wave() {
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
}

// Tile x window of a generic kernel's wave: x[qa .. qa + a.win) (zeros
// outside [0, n_in)), 8 float4 loads in flight per lane per round.
__device__ __forceinline__ void gen_load_window(const TileArgs& a, float* win, int lane, int64_t b,
                                                int64_t qa) {
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.x) + b * a.ld_x, 0, (int)(a.n_in * 4), 0x00020000);
  const int nf = a.win >> 2;
  for (int f0 = 0; f0 < nf; f0 += 8 * kWave) {
    f32x4 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int f = f0 + r * kWave + lane;  // past the window: harmless reads
      v[r] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)((qa + 4 * f) * 4), 0, kStream);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int f = f0 + r * kWave + lane;
      if (f < nf) *reinterpret_cast<f32x4*>(win + 4 * f) = v[r];
    }
  }
}

// Class tables of k_chain_gen into LDS (class stride kGenClassStride floats:
// the rows that lanes of different classes read together start on distinct
// bank quads), then the advance masks; two float4 loads in flight per thread.
// Ends with a workgroup barrier.
__device__ __forceinline__ void gen_load_classes(const TileArgs& a, float* seq, uint32_t* adv) {
  constexpr int kNT = kWave * kGenWaves;
  constexpr int kF4 = kGenTS * kGenTT / 4;  // float4s per class
  const int C = ((tt_ptr)a.tt)->classes;
  const f32x4* src = reinterpret_cast<const f32x4*>(a.tt->seq);
  f32x4 v[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) v[r] = src[(r * kNT + threadIdx.x) & (kGenClasses * kF4 - 1)];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = r * kNT + threadIdx.x, k = i / kF4, f = i - k * kF4;
    if (k < C) *reinterpret_cast<f32x4*>(seq + k * kGenClassStride + 4 * f) = v[r];
  }
  if (threadIdx.x < kGenClasses) adv[threadIdx.x] = a.tt->adv[threadIdx.x];
  __syncthreads();
}

// The generic kernels' on_nf for the repair rerun: window x[qa ..] unpadded
// in `win`, the lane's outputs m0 + 32 lane + i with j0 = (m0 + 32 lane) M + c.
__device__ __forceinline__ void gen_fix(const TileArgs& a, tt_ptr mt, const float* win, int64_t qa,
                                        int64_t j0, int64_t b, int64_t z0, float (&yy)[kGenTS],
                                        double (&v)[kD]) {
  const float thr = mt->flush_thr;
  fix_outputs(a, mt, b, z0, yy, v, [&](int i, float& nf, float& fin) {
    const int64_t j = j0 + (int64_t)i * a.M, q = j / a.L;
    const int base = (int)(q - qa);
    window_sums(a.taps, a.K, a.L, (int)(j - q * a.L), thr, a.T - 1,
                [&](int t) { return win[base - t]; }, nf, fin);
  });
}

// One tile of k_chain_gen for one wave (REPAIR: the rerun with the
// non-finite path).
template <bool UP, bool REPAIR, class ENTRY = ChainedEntry>
__device__ __forceinline__ void chain_gen_body(const TileArgs& a, const float* seq,
                                               const uint32_t* adv, float* win, int lane,
                                               int64_t b, int64_t tile, ENTRY&& entry = ENTRY{}) {
  const int L = a.L, M = a.M, T = a.T;
  const tt_ptr mt = (tt_ptr)a.tt;
  const int C = mt->classes;
  const int64_t m0 = tile * kGenTile;

  // ---- x window of the tile
  const int64_t qlo = (m0 * M + a.c) / L - (T - 1);
  const int64_t qa = (qlo >> 2) << 2;  // floor to a multiple of 4
  gen_load_window(a, win, lane, b, qa);
  fence();

  // ---- 1. SRC of the lane's 32 outputs, software-pipelined one output deep
  // (output i+1's LDS reads are issued before output i's FMAs).  UP (M < L):
  // q advances by 0 or 1 per output, so the 8-sample window slides in
  // registers and one new sample is read per output; otherwise all 8 are read.
  // (j = m M + c in 32 bits: tile_geometry keeps n_out M + c below 2^31)
  float y[kGenTS];
  const int64_t j0 = (m0 + (int64_t)kGenTS * lane) * M + a.c;
  {
    const int jl = (int)(m0 * M + a.c) + kGenTS * M * lane;
    int qr = jl / L - (T - 1) - (int)qa;  // window offset of the output's first tap
    const int dq = M / L;
    const int cls = ((int)tile * kWave + lane) % C;  // sub-chunk j = m0/32 + lane
    const float* row = seq + cls * kGenClassStride;   // output i's taps at row + 8 i
    const uint32_t am = adv[cls];
    float w[kGenTT];
#pragma unroll
    for (int u = 0; u < kGenTT; ++u) w[u] = win[qr + u];
    float4 h0 = *reinterpret_cast<const float4*>(row);
    float4 h1 = *reinterpret_cast<const float4*>(row + 4);
    float nx = UP ? win[qr + kGenTT] : 0.f;  // enters the window if q advances
#pragma unroll
    for (int i = 0; i < kGenTS; ++i) {
      // operands of output i+1
      const bool carry = (am >> i) & 1u;
      const int qr_n = qr + dq + (carry ? 1 : 0);
      float4 h0n, h1n;
      float nxn = 0.f, wn[kGenTT];
      if (i + 1 < kGenTS) {
        h0n = *reinterpret_cast<const float4*>(row + kGenTT * (i + 1));
        h1n = *reinterpret_cast<const float4*>(row + kGenTT * (i + 1) + 4);
        if constexpr (UP) {
          nxn = win[qr_n + kGenTT];
        } else {
#pragma unroll
          for (int u = 0; u < kGenTT; ++u) wn[u] = win[qr_n + u];
        }
      }
      // (even u, odd u) partial sums in the halves of one v_pk_fma_f32
      // chain: the same two chains, in the same order, as k_src_generic's.
      f32x2 acc = {0.f, 0.f};
      acc = __builtin_elementwise_fma(f32x2{h0.x, h0.y}, f32x2{w[0], w[1]}, acc);
      acc = __builtin_elementwise_fma(f32x2{h0.z, h0.w}, f32x2{w[2], w[3]}, acc);
      acc = __builtin_elementwise_fma(f32x2{h1.x, h1.y}, f32x2{w[4], w[5]}, acc);
      acc = __builtin_elementwise_fma(f32x2{h1.z, h1.w}, f32x2{w[6], w[7]}, acc);
      y[i] = acc.x + acc.y;
      if (i + 1 < kGenTS) {
        if constexpr (UP) {
#pragma unroll
          for (int u = 0; u < kGenTT - 1; ++u) w[u] = carry ? w[u + 1] : w[u];
          w[kGenTT - 1] = carry ? nx : w[kGenTT - 1];
          nx = nxn;
        } else {
#pragma unroll
          for (int u = 0; u < kGenTT; ++u) w[u] = wn[u];
        }
        h0 = h0n;
        h1 = h1n;
        qr = qr_n;
      }
    }
  }
  pin(y);
  if constexpr (REPAIR)
    tile_cascade<kGenTS, true, true>(a, mt, win, y, lane, b, tile, m0,
                                     [&](float (&yy)[kGenTS], double (&v)[kD]) {
                                       gen_fix(a, mt, win, qa, j0, b, m0 + kGenTS * lane, yy, v);
                                     });
  else
    tile_cascade<kGenTS>(a, mt, win, y, lane, b, tile, m0, 0, entry);
}

template <bool UP>
__global__ __launch_bounds__(kWave * kGenWaves) __attribute__((amdgpu_waves_per_eu(4))) void
k_chain_gen(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t tile = blockIdx.y;  // grid (groups, ntiles): tile-major
  const int64_t b = (int64_t)blockIdx.x * kGenWaves + w;
  float* seq = smem;
  uint32_t* adv = reinterpret_cast<uint32_t*>(smem + kGenClasses * kGenClassStride);
  gen_load_classes(a, seq, adv);
  if (b >= a.B) return;
  float* win = smem + kGenClasses * kGenClassStride + kGenClasses + w * a.win;
  chain_gen_body<UP, false>(a, seq, adv, win, lane, b, tile);
}

// Launches 1 and 3 of the three-launch mode (chain_tile.h, AggEntry).
template <bool UP, int MODE>
__global__ __launch_bounds__(kWave * kGenWaves) __attribute__((amdgpu_waves_per_eu(4))) void
k_chain_gen3(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t tile = blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x * kGenWaves + w;
  float* seq = smem;
  uint32_t* adv = reinterpret_cast<uint32_t*>(smem + kGenClasses * kGenClassStride);
  gen_load_classes(a, seq, adv);
  if (b >= a.B) return;
  float* win = smem + kGenClasses * kGenClassStride + kGenClasses + w * a.win;
  if constexpr (MODE == 1) chain_gen_body<UP, false>(a, seq, adv, win, lane, b, tile, AggEntry{});
  else chain_gen_body<UP, false>(a, seq, adv, win, lane, b, tile, GivenEntry{});
}

template <bool UP>
__global__ __launch_bounds__(kWave * kGenWaves) void k_chain_gen_repair(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  float* seq = smem;
  uint32_t* adv = reinterpret_cast<uint32_t*>(smem + kGenClasses * kGenClassStride);
  gen_load_classes(a, seq, adv);
  float* win = smem + kGenClasses * kGenClassStride + kGenClasses + w * a.win;
  repair_channels(a, w, kGenWaves, [&](int64_t b, int64_t tile) {
    chain_gen_body<UP, true>(a, seq, adv, win, lane, b, tile);
  });
}

// ---------------------------------------------------------------------------
// Select-free generic kernel for a compile-time ratio M < L (config 5's
// 160/147).  Output i of a lane reads x[q_i - (T-1) + u], q_i = q_0 + g_i +
// d_i with g_i = i M div L (compile-time) and d_i in {0, 1} (the class's
// phase carry).  The host folds d_i and the parity of g_i into the class rows
// (TileTables::seqs: T taps shifted by 0..2 in 10 slots), so output i sums
// its row against the window pairs from g_i rounded down to even -- registers
// at compile-time indices: no window sliding, no per-lane selects.  A shift
// of 1 swaps which half of the v_pk_fma_f32 holds the even-u and the odd-u
// chain; the extra slots hold zero taps (x * 0 + acc == acc, and +0 stays
// +0), so y = even + odd is bitwise k_chain_gen's and k_src_generic's.
// ---------------------------------------------------------------------------
// T7 (T <= 7 taps per branch, config 5's K = 1023): an output whose g_i is
// even has shift d_i in {0, 1}, so its taps fill slots 0..7 and slots 8, 9 are
// zero: the last tap-pair read and FMA are skipped (bitwise the same y).
constexpr int ct_gcd(int a, int b) { return b ? ct_gcd(b, a % b) : a; }

// Class rows of k_chain_gct into LDS (the C classes in use only).  Ends with
// a workgroup barrier.
__device__ __forceinline__ void ct_load_classes(const TileArgs& a, float* seq) {
  constexpr int kF4 = kGenTS * kCtRow / 4;  // float4s per class
  const int C = ((tt_ptr)a.tt)->classes;
  const f32x4* src = reinterpret_cast<const f32x4*>(&a.tt->seqs[0][0][0]);
  for (int i = threadIdx.x; i < C * kF4; i += kWave * kGenWaves) {
    const int k = i / kF4, f = i - k * kF4;
    *reinterpret_cast<f32x4*>(seq + k * kCtClassStride + 4 * f) = src[i];
  }
  __syncthreads();
}

// x offset (a multiple of 4) of the x window of a generic kernel's tile.
template <int L, int M>
__device__ __forceinline__ int64_t gen_window_start(const TileArgs& a, int64_t tile) {
  const int64_t qlo = (tile * kGenTile * M + a.c) / L - (a.T - 1);
  return (qlo >> 2) << 2;
}

// Steps 1-5 of one tile of k_chain_gct for one wave whose x window x[qa ..]
// is in `win` (REPAIR: the rerun with the non-finite path; entry:
// tile_cascade's).
template <int L, int M, bool T7, bool REPAIR, int G = 2, class ENTRY = ChainedEntry>
__device__ __forceinline__ void gct_tile(const TileArgs& a, const float* seq, float* win,
                                         int lane, int64_t b, int64_t tile, int64_t qa,
                                         ENTRY&& entry = ENTRY{}) {
  static_assert(M < L, "q advances by 0 or 1 per output");
  constexpr int NPW = ((kGenTS - 1) * M / L) / 2 + kCtTaps / 2;  // window pairs per lane
  const int T = a.T;
  // (opaque: in the persistent kernel's tile loop, table loads stay where
  // they are used instead of hoisted out of the loop into live registers)
  tt_ptr mt = (tt_ptr)a.tt;
  asm volatile("" : "+s"(mt));
  // the phase classes of the 32-output sub-chunk starts, known at compile
  // time for the ratio (gen_classes; the host checked the tables hold as many)
  constexpr int C = L / ct_gcd((kGenTS * M) % L, L);
  const int64_t m0 = tile * kGenTile;

  // ---- 1. SRC of the lane's 32 outputs from its register window
  // (j = m M + c in 32 bits: tile_geometry keeps n_out M + c below 2^31)
  float y[kGenTS];
  const int64_t j0 = (m0 + (int64_t)kGenTS * lane) * M + a.c;
  {
    const int jl = (int)(m0 * M + a.c) + kGenTS * M * lane;
    const float* xl = win + (jl / L - (T - 1) - (int)qa);
    const float* row = seq + (((int)tile * kWave + lane) % C) * kCtClassStride;
    f32x2 X[NPW];
#pragma unroll
    for (int m = 0; m < NPW; ++m) X[m] = f32x2{xl[2 * m], xl[2 * m + 1]};
    // Outputs in groups of G, the next group's tap rows read while this one
    // computes and the G FMA chains interleaved (each output's own chain,
    // groups in ascending order, is unchanged: y bitwise the same).  G = 2
    // against one output at a time: 1.128 -> 1.122 ms at config 5
    // (profiles/r04_gct_pairs_ab.txt); groups of 4 spill at 4 waves per SIMD
    // and pay at the persistent kernel's 3 (profiles/r05_gcp_ab.txt).
    static_assert(kGenTS % G == 0, "whole groups");
    struct Row {
      f32x4 t0, t1;
      f32x2 t2;
    };
    auto load_row = [&](int i) {
      Row r;
      r.t0 = *reinterpret_cast<const f32x4*>(row + kCtRow * i);
      r.t1 = *reinterpret_cast<const f32x4*>(row + kCtRow * i + 4);
      if (!(T7 && ((i * M / L) % 2 == 0)))
        r.t2 = *reinterpret_cast<const f32x2*>(row + kCtRow * i + 8);
      else
        r.t2 = f32x2{0.f, 0.f};
      return r;
    };
    Row cur[G];
#pragma unroll
    for (int o = 0; o < G; ++o) cur[o] = load_row(o);
#pragma unroll
    for (int i0 = 0; i0 < kGenTS; i0 += G) {
      Row nxt[G];
      if (i0 + G < kGenTS) {
#pragma unroll
        for (int o = 0; o < G; ++o) nxt[o] = load_row(i0 + G + o);
      }
      f32x2 acc[G];
#pragma unroll
      for (int o = 0; o < G; ++o) acc[o] = f32x2{0.f, 0.f};
#pragma unroll
      for (int pp = 0; pp < 5; ++pp) {
#pragma unroll
        for (int o = 0; o < G; ++o) {
          const int i = i0 + o;
          const int g2 = (i * M / L) / 2;
          const bool last = !(T7 && ((i * M / L) % 2 == 0));
          if (pp == 4 && !last) continue;
          const f32x2 t = pp == 0   ? f32x2{cur[o].t0.x, cur[o].t0.y}
                          : pp == 1 ? f32x2{cur[o].t0.z, cur[o].t0.w}
                          : pp == 2 ? f32x2{cur[o].t1.x, cur[o].t1.y}
                          : pp == 3 ? f32x2{cur[o].t1.z, cur[o].t1.w}
                                    : cur[o].t2;
          acc[o] = __builtin_elementwise_fma(t, X[g2 + pp], acc[o]);
        }
      }
#pragma unroll
      for (int o = 0; o < G; ++o) y[i0 + o] = acc[o].x + acc[o].y;
#pragma unroll
      for (int o = 0; o < G; ++o) cur[o] = nxt[o];
    }
  }
  pin(y);
  if constexpr (REPAIR)
    tile_cascade<kGenTS, true, true>(a, mt, win, y, lane, b, tile, m0,
                                     [&](float (&yy)[kGenTS], double (&v)[kD]) {
                                       gen_fix(a, mt, win, qa, j0, b, m0 + kGenTS * lane, yy, v);
                                     });
  else
    tile_cascade<kGenTS>(a, mt, win, y, lane, b, tile, m0, 0, entry);
}

// One tile of k_chain_gct for one wave: its x window, then gct_tile.
template <int L, int M, bool T7, bool REPAIR, class ENTRY = ChainedEntry>
__device__ __forceinline__ void chain_gct_body(const TileArgs& a, const float* seq, float* win,
                                               int lane, int64_t b, int64_t tile,
                                               ENTRY&& entry = ENTRY{}) {
  const int64_t qa = gen_window_start<L, M>(a, tile);
  gen_load_window(a, win, lane, b, qa);
  fence();
  gct_tile<L, M, T7, REPAIR>(a, seq, win, lane, b, tile, qa, entry);
}

template <int L, int M, bool T7 = false>
__global__ __launch_bounds__(kWave * kGenWaves) __attribute__((amdgpu_waves_per_eu(4))) void
k_chain_gct(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t tile = blockIdx.y;  // grid (groups, ntiles): tile-major
  const int64_t b = (int64_t)blockIdx.x * kGenWaves + w;
  float* seq = smem;
  ct_load_classes(a, seq);
  if (b >= a.B) return;
  float* win = smem + ((tt_ptr)a.tt)->classes * kCtClassStride + w * a.win;
  chain_gct_body<L, M, T7, false>(a, seq, win, lane, b, tile);
}

// Launches 1 and 3 of the three-launch mode (chain_tile.h, AggEntry).
template <int L, int M, bool T7, int MODE>
__global__ __launch_bounds__(kWave * kGenWaves) __attribute__((amdgpu_waves_per_eu(4))) void
k_chain_gct3(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t tile = blockIdx.y;
  const int64_t b = (int64_t)blockIdx.x * kGenWaves + w;
  float* seq = smem;
  ct_load_classes(a, seq);
  if (b >= a.B) return;
  float* win = smem + ((tt_ptr)a.tt)->classes * kCtClassStride + w * a.win;
  if constexpr (MODE == 1) chain_gct_body<L, M, T7, false>(a, seq, win, lane, b, tile, AggEntry{});
  else chain_gct_body<L, M, T7, false>(a, seq, win, lane, b, tile, GivenEntry{});
}

template <int L, int M, bool T7 = false>
__global__ __launch_bounds__(kWave * kGenWaves) void k_chain_gct_repair(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int lane = threadIdx.x & (kWave - 1);
  float* seq = smem;
  ct_load_classes(a, seq);
  float* win = smem + ((tt_ptr)a.tt)->classes * kCtClassStride + w * a.win;
  repair_channels(a, w, kGenWaves, [&](int64_t b, int64_t tile) {
    chain_gct_body<L, M, T7, true>(a, seq, win, lane, b, tile);
  });
}

// Persistent k_chain_gct (round 4), for batches of at least a chip's worth of
// workgroups: a workgroup loads the class rows once and walks channel groups
// (grid-stride); each wave runs its channel's tiles in order, carrying the
// end state in registers (RegCarry: no hand-off, no flags, no tile waiting on
// another workgroup).  Every tile's end state is still published for the
// repair kernel.  Rows are bitwise the chained kernel's: the same tile code on
// the same entry states.  Config 5 (8192 channels): 1.134-1.137 vs
// 1.191-1.200 ms same box (profiles/r04_gcp_ab.txt).
// Round 5: 3 waves per SIMD (up to 168 VGPRs) instead of 4, which buys (a) the
// next tile's x window in flight in registers behind the whole current tile
// -- loaded as soon as this tile's window is in LDS, the next channel's tile 0
// behind a channel's last tile -- and (b) the SRC in groups of 4 outputs:
// 1.116 -> 1.094 ms same box (profiles/r05_gcp_ab.txt; (a) alone 1.098).  At 4
// waves per SIMD half the window in flight measured the same and the whole
// window spilled (round 4); an LDS-DMA into a second window slot does not fit
// the LDS, and stores straight from registers instead of store_tile's LDS
// staging, which would free the slot, ran 1.6x (default cache policy) to 6x
// (nt) slower (16-byte pieces 128 bytes apart).
constexpr int kGcpWin = 8;  // float4 per lane of a tile's x window (a.win <= 4 * 8 * 64)

template <int L, int M, bool T7 = false>
__global__ __launch_bounds__(kWave * kGenWaves) __attribute__((amdgpu_waves_per_eu(3))) void
k_chain_gcp(TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int w = gen_wave();
  const int64_t groups = (a.B + kGenWaves - 1) / kGenWaves;
  float* seq = smem;
  ct_load_classes(a, seq);
  float* win = smem + ((tt_ptr)a.tt)->classes * kCtClassStride + w * a.win;
  const int nf = a.win >> 2;
  f32x4 v[kGcpWin];
  auto load = [&](int64_t bb, int64_t tile) {
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.x) + bb * a.ld_x, 0, (int)(a.n_in * 4), 0x00020000);
    const int64_t qa = gen_window_start<L, M>(a, tile);
    const int ln = lane_id();
#pragma unroll
    for (int r = 0; r < kGcpWin; ++r)  // past the window: harmless reads
      v[r] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)((qa + 4 * (r * kWave + ln)) * 4), 0,
                                                   kStream);
  };
  if ((int64_t)blockIdx.x * kGenWaves + w < a.B) load((int64_t)blockIdx.x * kGenWaves + w, 0);
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t b = g * kGenWaves + w;
    if (b >= a.B) break;  // the last group's missing channels (wave-uniform)
    RegCarry carry{0.0, 0.0};
    for (int64_t tile = 0; tile < a.ntiles; ++tile) {
      const int64_t qa = gen_window_start<L, M>(a, tile);
      {
        const int ln = lane_id();
#pragma unroll
        for (int r = 0; r < kGcpWin; ++r) {
          // (rows r < kGcpWin - 1 are whole: the launcher checks nf; one exec
          // mask instead of eight)
          const int f = r * kWave + ln;
          if (r < kGcpWin - 1 || f < nf) *reinterpret_cast<f32x4*>(win + 4 * f) = v[r];
        }
      }
      fence();
      if (tile + 1 < a.ntiles) {
        load(b, tile + 1);
      } else {
        const int64_t bn = b + (int64_t)gridDim.x * kGenWaves;
        if (bn < a.B) load(bn, 0);
      }
      // (an opaque lane per tile: what the tile derives from it is recomputed
      // instead of hoisted out of the loop and held through it)
      int ln = lane_id();
      asm volatile("" : "+v"(ln));
      gct_tile<L, M, T7, false, 4>(a, seq, win, ln, b, tile, qa, carry);
    }
  }
}

// Launch 2 of the three-launch mode (chain_tile.h, AggEntry): wave k of the
// channel's workgroup owns state block k; lane l of round r holds tile
// t = 64 r + l.  With P = D_k^(64 TS) (a tile) and e_t the aggregates, the
// entry states S_t = sum_(s<t) P^(t-1-s) e_s come from an inclusive
// Kogge-Stone over the lanes, I_l = sum_(s<=l) P^(l-s) e_(64r+s), and the
// carry C of the rounds before: S_(64r+l) = P^l C + I_(l-1), C' = P^64 C +
// I_63.  They replace the aggregates in states[] (launch 3 reads them).
__global__ __launch_bounds__(kWave * kS) void k_tile_carry(TileArgs a) {
  typedef double m2[4];  // row-major 2x2
  auto mul = [](const m2& x, const m2& y, m2& r) {
    const double r0 = fma(x[0], y[0], x[1] * y[2]), r1 = fma(x[0], y[1], x[1] * y[3]);
    const double r2 = fma(x[2], y[0], x[3] * y[2]), r3 = fma(x[2], y[1], x[3] * y[3]);
    r[0] = r0;
    r[1] = r1;
    r[2] = r2;
    r[3] = r3;
  };
  const int k = (int)threadIdx.x / kWave;
  const int lane = (int)threadIdx.x % kWave;
  const int64_t b = blockIdx.x;
  const TileTables* mt = a.tt;
  m2 pw[7];  // P^(2^j)
  {
    const m2 d5 = {mt->Dp[5][k][0], mt->Dp[5][k][1], mt->Dp[5][k][2], mt->Dp[5][k][3]};
    mul(d5, d5, pw[0]);
  }
#pragma unroll
  for (int j = 1; j < 7; ++j) mul(pw[j - 1], pw[j - 1], pw[j]);
  m2 pl = {1.0, 0.0, 0.0, 1.0};  // P^lane
#pragma unroll
  for (int j = 0; j < 6; ++j)
    if ((lane >> j) & 1) mul(pl, pw[j], pl);
  double c0 = 0.0, c1 = 0.0;
  double* st = a.states + b * a.ntiles * kD + 2 * k;
  for (int64_t t0 = 0; t0 < a.ntiles; t0 += kWave) {
    const int64_t t = t0 + lane;
    const bool in = t < a.ntiles;
    double i0 = in ? st[t * kD] : 0.0, i1 = in ? st[t * kD + 1] : 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int d = 1 << j;
      const int src = lane >= d ? lane - d : lane;
      const double x0 = shfl_f64(i0, src), x1 = shfl_f64(i1, src);
      if (lane >= d) {
        i0 = fma(pw[j][0], x0, fma(pw[j][1], x1, i0));
        i1 = fma(pw[j][2], x0, fma(pw[j][3], x1, i1));
      }
    }
    double x0 = shfl_f64(i0, lane > 0 ? lane - 1 : 0), x1 = shfl_f64(i1, lane > 0 ? lane - 1 : 0);
    if (lane == 0) x0 = x1 = 0.0;
    if (in) {
      st[t * kD] = fma(pl[0], c0, fma(pl[1], c1, x0));
      st[t * kD + 1] = fma(pl[2], c0, fma(pl[3], c1, x1));
    }
    const double j0 = shfl_f64(i0, kWave - 1), j1 = shfl_f64(i1, kWave - 1);
    const double n0 = fma(pw[6][0], c0, fma(pw[6][1], c1, j0));
    const double n1 = fma(pw[6][2], c0, fma(pw[6][3], c1, j1));
    c0 = n0;
    c1 = n1;
  }
}

constexpr int64_t kRepairGroups = 1024;  // workgroups of a repair kernel

void launch_tile_carry(const TileArgs& a, hipStream_t s) {
  TraceScope trace("chain_tile_carry", s);
  hipLaunchKernelGGL(k_tile_carry, dim3((unsigned)a.B), dim3(kWave * kS), 0, s, a);
}

}  // namespace

int launch_three(TileKernel agg, TileKernel given, dim3 grid, unsigned block, size_t shm,
                 const TileArgs& a, hipStream_t s) {
  if (int rc = allow_lds(agg, shm)) return rc;
  if (int rc = allow_lds(given, shm)) return rc;
  {
    TraceScope trace("chain_tile_agg", s);
    hipLaunchKernelGGL(agg, grid, dim3(block), shm, s, a);
  }
  launch_tile_carry(a, s);
  TraceScope trace("chain_tile", s);
  hipLaunchKernelGGL(given, grid, dim3(block), shm, s, a);
  return DSP_OK;
}

int launch_repair(TileKernel rep, unsigned rgrid, unsigned block, size_t shm, const TileArgs& a,
                  hipStream_t s) {
  if (int rc = allow_lds(rep, shm)) return rc;
  TraceScope trace("chain_repair", s);
  hipLaunchKernelGGL(rep, dim3(rgrid), dim3(block), shm, s, a);
  return DSP_OK;
}

int launch_chain_tile(const float* x, float* y, float* z, int64_t B, int64_t n_in, int64_t ld_x,
                      int64_t n_out, int64_t ld_y, const float* taps, int K, int L, int M,
                      int64_t c, const double* sos, int S, int clip, const void* tables,
                      uint64_t key, uint32_t max_spins, int variant, void* ws, size_t ws_bytes,
                      hipStream_t s) {
  TilePlan tp;
  if (!tables || !tile_geometry(n_in, n_out, K, L, M, c, S, &tp)) return kNotFused;
  DSP_REQUIRE(taps, "null taps");  // the non-finite path reads the caller's taps
  // Tables built for another geometry or cascade: the two-launch chain.  The
  // key also says whether the tables' taps make branch 0 a pure delay.
  const uint64_t key0 = tables_key(tp, n_in, n_out, K, L, M, c, sos, S);
  const bool dly = key == dly_key(key0);
  if (key != key0 && !dly) return kNotFused;
  // (one row: its pitch addresses nothing)
  auto aligned = [B](const void* p, int64_t ld) {
    return (B == 1 || (ld & 3) == 0) && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  };
  if (!aligned(x, ld_x) || (y && !aligned(y, ld_y)) || !aligned(z, ld_y)) return kNotFused;
  SosParams p;
  if (!realize(sos, S, &p)) return kNotFused;
  const TileWs w = tile_ws(B, tp.ntiles);
  DSP_REQUIRE(ws && ws_bytes >= w.total, "chain workspace too small: %zu < %zu bytes", ws_bytes,
              w.total);
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "chain workspace not 256-B aligned");
  DSP_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 255) == 0, "chain tables not 256-B aligned");
  DSP_REQUIRE(B * tp.ntiles < ((int64_t)1 << 31), "batch too large for one launch");
  char* base = static_cast<char*>(ws);
  TileArgs a;
  a.x = x;
  a.y = y;
  a.z = z;
  a.tt = static_cast<const TileTables*>(tables);
  a.states = reinterpret_cast<double*>(base + w.st_off);
  a.flags = reinterpret_cast<uint32_t*>(base + w.fl_off);
  a.err = reinterpret_cast<uint32_t*>(base + w.err_off);
  a.B = B;
  a.n_in = n_in;
  a.ld_x = ld_x;
  a.n_out = n_out;
  a.ld_y = ld_y;
  a.ntiles = tp.ntiles;
  a.cq = c / L;
  a.clip = clip;
  a.max_spins = max_spins;
  a.taps = taps;
  a.c = c;
  a.K = K;
  a.L = L;
  a.M = M;
  a.T = (K + L - 1) / L;
  a.win = tp.win;
  // Workgroups of one wave (kinds 1 and 4) or of kGenWaves waves, a channel
  // each.  The repair kernel after the single-pass one (k_chain_*_repair): 64
  // channels per wave, at most kRepairGroups workgroups.
  const int64_t waves = tp.kind == 1 || tp.kind == 4 ? 1 : kGenWaves;
  const int64_t groups = ceil_div(B, waves);  // (<= B: groups * ntiles < 2^31 too)
  const unsigned block = (unsigned)(kWave * waves);
  const unsigned rgrid = (unsigned)std::min<int64_t>(ceil_div(B, block), kRepairGroups);
  // The mode.  dsp_chain_path (variant) 4 forces the three-launch mode and 2
  // the chained tiles; 0 follows the planner (chain_mode's promise); 3 asks for
  // the persistent kernel, which only kind 3 has -- that kind never takes three
  // launches under it (below), the others stay automatic.
  const bool three = variant == 4 || ((variant == 0 || (variant == 3 && tp.kind != 3)) &&
                                      plan_three_launches(tp, B));
  if (tp.kind == 4) {
    // the per-phase kernels (chain_pp_<n>.hip): tile 0's window starts at xa0
    // (a multiple of 4; the alignment A is in the tap rows)
    a.cq = pp_need(K, L, M, c).xa0;
    const PpEntry& e = kPpEntries[tp.pp];
    int rc = launch_chain_pp_0(e, a, rgrid, three, s);
    if (rc == kNotFused) rc = launch_chain_pp_1(e, a, rgrid, three, s);
    if (rc == kNotFused) rc = launch_chain_pp_2(e, a, rgrid, three, s);
    if (rc == kNotFused) rc = launch_chain_pp_3(e, a, rgrid, three, s);
    if (rc == kNotFused) return set_error(DSP_EINVAL, "no per-phase kernel for entry %d", tp.pp);
    return rc;
  }
  // Each kind picks its kernels -- k1 and k3 are launches 1 and 3 of the
  // three-launch mode -- and what is its own of the chained launch: kind 1's
  // paired tail tiles, kind 3's persistent kernel.
  const dim3 grid((unsigned)groups, (unsigned)tp.ntiles);
  dim3 cgrid = grid;  // of the chained (or persistent) launch
  size_t shm = 0;
  TileKernel k1, k3, kern, rep, pair = nullptr;
  if (tp.kind == 1) {
    // (No persistent variant: one measured 9 % slower at config 4 and 5 % at
    // config 3 than these chained tiles, profiles/r04_tilep_ab.txt.)
    k1 = dly ? k_chain_tile3<Geo3241, true, 1> : k_chain_tile3<Geo3241, false, 1>;
    k3 = dly ? k_chain_tile3<Geo3241, true, 2> : k_chain_tile3<Geo3241, false, 2>;
    kern = dly ? k_chain_tile<Geo3241, true> : k_chain_tile<Geo3241, false>;
    // A last tile of at most 32 sub-chunks (half a wave): the last tiles of
    // two channels share a wave (k_chain_tile_pair), after the other tiles
    // of every channel.  a.ntiles stays: tile ntiles - 2 raises its flag.
    const int64_t tail = n_out - (tp.ntiles - 1) * Geo3241::TILE;
    if (B >= 2 && ceil_div(tail, (int64_t)Geo3241::TSUB) <= kWave / 2) {
      pair = dly ? k_chain_tile_pair<Geo3241, true> : k_chain_tile_pair<Geo3241, false>;
      cgrid.y = (unsigned)(tp.ntiles - 1);
    }
    rep = dly ? k_chain_tile_repair<Geo3241, true> : k_chain_tile_repair<Geo3241, false>;
  } else if (tp.kind == 3) {
    shm = ct_lds_bytes(gen_classes(L, M), tp.win);
    const bool t7 = a.T <= 7;
    kern = t7 ? k_chain_gct<160, 147, true> : k_chain_gct<160, 147, false>;
    rep = t7 ? k_chain_gct_repair<160, 147, true> : k_chain_gct_repair<160, 147, false>;
    const TileKernel pers = t7 ? k_chain_gcp<160, 147, true> : k_chain_gcp<160, 147, false>;
    // Persistent kernel when the batch fills the chip with whole rounds of
    // channel groups (a smaller batch runs the chained kernel, whose tiles of
    // one channel overlap everything but their carry; the three-launch mode is
    // for batches far below these).  Variant 3: whenever its window fits.
    const int res = t7 ? resident_groups<k_chain_gcp<160, 147, true>>(kWave * kGenWaves, shm)
                       : resident_groups<k_chain_gcp<160, 147, false>>(kWave * kGenWaves, shm);
    const int64_t rounds = res > 0 ? ceil_div(groups, res) : 0;
    const bool fits = tp.win <= 4 * kGcpWin * kWave && tp.win > 4 * (kGcpWin - 1) * kWave;
    if (!three && variant != 2 && fits &&
        (variant == 3 || (res > 0 && groups >= res && groups * 8 >= rounds * res * 7))) {
      kern = pers;
      cgrid = dim3((unsigned)std::min<int64_t>(groups, std::max(res, 1)));
    }
    k1 = t7 ? k_chain_gct3<160, 147, true, 1> : k_chain_gct3<160, 147, false, 1>;
    k3 = t7 ? k_chain_gct3<160, 147, true, 2> : k_chain_gct3<160, 147, false, 2>;
  } else {
    shm = gen_lds_bytes(tp.win);
    kern = M < L ? k_chain_gen<true> : k_chain_gen<false>;
    rep = M < L ? k_chain_gen_repair<true> : k_chain_gen_repair<false>;
    k1 = M < L ? k_chain_gen3<true, 1> : k_chain_gen3<false, 1>;
    k3 = M < L ? k_chain_gen3<true, 2> : k_chain_gen3<false, 2>;
  }
  if (three) {
    if (int rc = launch_three(k1, k3, grid, block, shm, a, s)) return rc;
  } else {
    if (int rc = allow_lds(kern, shm)) return rc;
    TraceScope trace("chain_tile", s);
    if (cgrid.y > 0) hipLaunchKernelGGL(kern, cgrid, dim3(block), shm, s, a);
    if (pair) hipLaunchKernelGGL(pair, dim3((unsigned)ceil_div(B, 2)), dim3(block), 0, s, a);
  }
  if (int rc = launch_repair(rep, rgrid, block, shm, a, s)) return rc;
  DSP_LAUNCHED("k_chain_tile");
  return DSP_OK;
}

}  // namespace dsp
