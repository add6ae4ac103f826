// Host planner of the single-pass chain kernels (chain_plan.hip): what the
// launcher (chain_tile.hip, launch_chain_tile) needs of it.
#pragma once
#include "chain_pp.h"
#include "chain_tile.h"

namespace dsp {

// Instantiated geometries: (L, M, ceil(K/L), c mod L).  (3, 2, 41, 0) is the
// benchmark's L3/M2 with the default K = 121 (configs 3 and 4).
typedef TileGeo<3, 2, 41, 0> Geo3241;

struct TilePlan {
  int kind;  // 1: k_chain_tile<Geo3241>, 2: k_chain_gen, 3: k_chain_gct<160, 147>,
             // 4: k_chain_pp<PpGeo<...>> (chain_pp.h)
  int64_t tsub, tile, ntiles;
  int win;   // kind 2: floats of a wave's x window
  int pp;    // kind 4: the entry of chain_pp_list.h
};

// The kernel and tiling that serve a call; false: the two-launch chain.
bool tile_geometry(int64_t n_in, int64_t n_out, int K, int L, int M, int64_t c, int S,
                   TilePlan* tp);

// Whether the default (dsp_chain_path 0) takes the three-launch mode for a
// batch of B rows of this plan.
bool plan_three_launches(const TilePlan& tp, int64_t B);

uint64_t tables_key(const TilePlan& tp, int64_t n_in, int64_t n_out, int K, int L, int M,
                    int64_t c, const double* sos, int S);
uint64_t dly_key(uint64_t base);

struct TileWs {
  size_t err_off, st_off, fl_off, total;
};
TileWs tile_ws(int64_t B, int64_t ntiles);

// The per-phase kernels' instantiations (chain_pp_list.h, tools/gen_chain_pp.py).
extern const PpEntry kPpEntries[];

// What a call's geometry needs of a per-phase kernel (chain_pp.h, file
// comment): the reduced ratio, the window alignment A and the first window
// sample xa0 of tile 0, r0 and rho, the slot count P, the tap pairs NP of the
// widest slot row and the delay branch's centre offset UC (-1: no delay
// branch, downsampling).
struct PpNeed {
  int g, LR, MR, T, A, r0, rho, P, npmin, UC;
  int64_t xa0;
};
PpNeed pp_need(int K, int L, int M, int64_t c);

// Dynamic LDS of the generic kernels (k_chain_gen; k_chain_gct and its phase
// classes).
size_t gen_lds_bytes(int win);
int gen_classes(int L, int M);
size_t ct_lds_bytes(int classes, int win);

}  // namespace dsp
