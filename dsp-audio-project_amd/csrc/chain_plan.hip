// Host planner of the single-pass chain (chain_tile.hip, chain_pp.h): which
// kernel and tiling serve a call (tile_geometry), whether its default takes
// the three-launch mode (plan_three_launches), the workspace layout (tile_ws)
// and the kernels' tables, built in float64 (chain_tile_tables; the algebra
// is in chain_tile.hip's file comment).  No device code and no launch: the
// launcher is chain_tile.hip's launch_chain_tile.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cascade.h"
#include "chain_plan.h"
#include "chain_pp.h"
#include "chain_tile.h"

namespace dsp {

const PpEntry kPpEntries[] = {
#define PP_GEO(IDX, LR, MR, TS, NP, UC, NH, PB) {LR, MR, TS, NP, UC, NH, PB},
#include PP_LIST
#undef PP_GEO
};

namespace {

int64_t floor_mod(int64_t a, int64_t m) { return ((a % m) + m) % m; }

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The entry of chain_pp_list.h that serves the geometry, or -1.
int pp_entry(int K, int L, int M, int64_t c) {
  const PpNeed n = pp_need(K, L, M, c);
  if (n.LR > 8 || n.MR > 8) return -1;
  for (int i = 0; i < (int)std::size(kPpEntries); ++i) {
    const PpEntry& e = kPpEntries[i];
    // (an entry far wider than the call's taps would spend its FMAs on zero
    // taps: fewer taps take k_chain_gen or the two-launch chain)
    if (e.LR != n.LR || e.MR != n.MR || e.NP < n.npmin || e.NP > n.npmin + 4) continue;
    if (e.UC >= 0 ? (n.LR < n.MR || e.UC != n.UC || n.A != 0) : n.LR >= n.MR) continue;
    return i;
  }
  return -1;
}

// Floats of the generic kernel's x window for one tile: the tile's input span
// ((kGenTile-1) M / L + T), up to 3 of alignment, and taps past T reading up
// to kGenTT - T samples beyond; at least the store staging.
int gen_window(int L, int M, int T) {
  const int64_t w = ((int64_t)(kGenTile - 1) * M) / L + T + 4 + (kGenTT - T) + 2;
  const int64_t r = (w + 3) / 4 * 4;
  return (int)std::max<int64_t>(r, std::max(staging_floats(kGenTS), kScanFloats));
}

constexpr size_t kGenLdsMax = 64 * 1024;  // two workgroups (8 waves) per CU at least

// The single-pass kernels' grids are (channels or channel groups, tiles): at
// most 65535 tiles per row (201 M outputs of the L3/M2 kernel, 134 M of the
// generic ones); longer rows take the two-launch chain.
constexpr int64_t kMaxTiles = 65535;

}  // namespace

PpNeed pp_need(int K, int L, int M, int64_t c) {
  PpNeed n;
  n.g = (int)gcd64(L, M);
  n.LR = L / n.g;
  n.MR = M / n.g;
  n.T = (K + L - 1) / L;
  n.rho = (int)(c % n.g);
  const int64_t c1 = c / n.g;
  n.r0 = (int)(c1 % n.LR);
  const int64_t w0 = c1 / n.LR - (n.T - 1);  // tile 0's first window sample, unaligned
  n.A = (int)floor_mod(w0, 4);
  n.xa0 = w0 - n.A;
  n.P = (n.MR % 2) ? 2 * n.LR : n.LR;
  int smax = 0;
  for (int t = 0; t < n.P; ++t) {
    const int qc = t * n.MR / n.LR;
    const int delta = (n.r0 + t * n.MR) / n.LR - qc;
    smax = std::max(smax, n.A + (qc & 1) + delta);
  }
  n.npmin = (n.T + smax + 1) / 2;
  n.UC = n.LR >= n.MR ? (int)(n.T - 1 - c / L) : -1;
  return n;
}

size_t gen_lds_bytes(int win) {
  return ((size_t)kGenClasses * kGenClassStride + kGenClasses + (size_t)kGenWaves * win) *
         sizeof(float);
}

// Phase classes of the generic kernel's sub-chunk starts (outputs 32 j):
// L / gcd(32 M mod L, L).
int gen_classes(int L, int M) {
  return (int)(L / gcd64(((int64_t)kGenTS * M) % L, L));
}

size_t ct_lds_bytes(int classes, int win) {
  return ((size_t)classes * kCtClassStride + (size_t)kGenWaves * win) * sizeof(float);
}

bool tile_geometry(int64_t n_in, int64_t n_out, int K, int L, int M, int64_t c, int S,
                   TilePlan* tp) {
  // S = 0 (the EQ bypassed, or a clip-only EQ): no single-pass kernel.  z is y
  // (or its clip) there, and the two-launch chain's copy pass is cheaper than
  // the kernel's identity cascade; it also keeps the bypass's non-finite
  // semantics (an inf or NaN stays within the SRC's window; the single-pass
  // repair would carry it into every later state of the padding stages).
  if (S < 1 || S > kS || n_in < 1 || n_out < 1 || L < 1 || M < 1 || K < 1) return false;
  // n_in a multiple of 4 (the rows' float4 windows), but for the one-tap SRC
  // bypass: its x loads stop at the row's end by the buffer range check, per
  // dword (tools/probe_buffer_oob.hip), so any length runs -- one row, or
  // rows whose pitch is a multiple of 4 (launch_chain_tile checks)
  const bool one_tap = L == 1 && M == 1 && K == 1 && c == 0;
  if (n_in % 4 && !one_tap) return false;
  // SRC bypass (L = M = 1): only as the one-tap SRC (K = 1, c = 0; the
  // caller passes the tap 1.0), which the per-phase entry of the cascade alone
  // serves (chain_pp.h); any other L = M = 1 call takes the two-launch chain.
  if (L == 1 && M == 1 && (K != 1 || c != 0)) return false;
  if (n_in * 4 + 16 >= ((int64_t)1 << 31) || n_out * 4 + 16 >= ((int64_t)1 << 31)) return false;
  // The plan of a kind whose lanes own tsub outputs, if its tiles fit a grid.
  auto plan = [&](int kind, int64_t tsub, int win, int pp) {
    *tp = TilePlan{kind, tsub, kWave * tsub, ceil_div(n_out, kWave * tsub), win, pp};
    return tp->ntiles <= kMaxTiles;
  };
  const int TT = (K + L - 1) / L;
  // Specialised kernel: lane windows on 16-byte boundaries, i.e. the x offset
  // of tile t's window, t*2048 + c/L - (TT-1), a multiple of 4.
  if (L == 3 && M == 2 && TT == 41 && c % L == 0 && n_out % 4 == 0 &&
      ((c / L) - (TT - 1)) % 4 == 0)
    return plan(1, Geo3241::TSUB, 0, -1);
  // Per-phase kernels (chain_pp.h): every ratio of the app's sliders at the
  // default tap rule (and config 1's 2/1 at K = 127).
  if (L <= 64 && M <= 64) {
    const int e = pp_entry(K, L, M, c);
    if (e >= 0) return plan(4, kPpEntries[e].TS, 0, e);
  }
  if (TT > kGenTT || gen_classes(L, M) > kGenClasses ||
      (n_out + kGenTile) * M + c >= ((int64_t)1 << 31))
    return false;
  if (L == 160 && M == 147) {
    // Window pairs up to (31 M div L) rounded to even + 10 past the lane's
    // start: at most 1 float beyond gen_window's span; +4 keeps the rounding.
    const int win = gen_window(L, M, TT) + 4;
    if (ct_lds_bytes(gen_classes(L, M), win) <= kGenLdsMax) return plan(3, kGenTS, win, -1);
  }
  const int win = gen_window(L, M, TT);
  return gen_lds_bytes(win) <= kGenLdsMax && plan(2, kGenTS, win, -1);
}

// Fingerprint of everything the tables depend on that a call can state on the
// host: the kernel kind and geometry, the cascade (sos bits) and the table
// layout version.  FNV-1a, 64 bit.
uint64_t tables_key(const TilePlan& tp, int64_t n_in, int64_t n_out, int K, int L, int M,
                    int64_t c, const double* sos, int S) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
      h ^= b[i];
      h *= 1099511628211ull;
    }
  };
  const int64_t v[] = {5 /* table layout version */, tp.kind, tp.tsub, tp.kind == 4 ? tp.pp : -1,
                       n_in, n_out, K, L, M, c, S,
                       (int64_t)sizeof(TileTables)};
  mix(v, sizeof(v));
  if (S > 0 && sos) mix(sos, sizeof(double) * 5 * (size_t)S);
  return h ? h : 1;  // 0 never names a table
}

// Key of tables whose taps take the DLY kernel (never 0, never the plain key).
uint64_t dly_key(uint64_t base) {
  const uint64_t k = base ^ 0x9e3779b97f4a7c15ull;
  return k ? k : 2;
}

namespace {

size_t align256(size_t v) { return v > SIZE_MAX - 255 ? SIZE_MAX : (v + 255) & ~(size_t)255; }

// Solves the 4x4 system M z = r in place (partial pivoting); false if singular
// to working precision.
bool solve4(double M[4][4], double r[4]) {
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int i = c + 1; i < 4; ++i)
      if (std::fabs(M[i][c]) > std::fabs(M[piv][c])) piv = i;
    if (!(std::fabs(M[piv][c]) > 1e-13)) return false;
    if (piv != c) {
      for (int j = 0; j < 4; ++j) std::swap(M[c][j], M[piv][j]);
      std::swap(r[c], r[piv]);
    }
    for (int i = c + 1; i < 4; ++i) {
      const double f = M[i][c] / M[c][c];
      for (int j = c; j < 4; ++j) M[i][j] -= f * M[c][j];
      r[i] -= f * r[c];
    }
  }
  for (int c = 3; c >= 0; --c) {
    double s = r[c];
    for (int j = c + 1; j < 4; ++j) s -= M[c][j] * r[j];
    r[c] = s / M[c][c];
  }
  return true;
}

// Pass-1 tables in input-normal coordinates (file comment, step 2): the state
// covariance of the first n states under unit white noise, X = sum_k A^k B B^T
// A^kT (doubling: X <- X + P X P^T, P <- P^2), its Cholesky factor P (X = P
// P^T), Gc[i] = P^-1 A^(tsub-1-i) B in float32 and Q = T^-1 P.  Any
// invertible P gives the exact E' in float64 arithmetic; input-normal
// coordinates keep the float32 sums well scaled.  false when X is not
// numerically positive definite (an uncontrollable mode, e.g. a band cancelled
// by its inverse) or P is ill-conditioned: the two-launch chain serves those.
bool input_normal_tables(const std::vector<double>& A, const double* Bv,
                         const std::vector<double>& Ti, int n, int tsub, TileTables* tt) {
  auto at = [&](const std::vector<double>& M, int r, int c) -> double { return M[(size_t)r * kD + c]; };
  std::vector<double> X((size_t)kD * kD, 0.0), Pw(A), tmp((size_t)kD * kD);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) X[(size_t)r * kD + c] = Bv[r] * Bv[c];
  for (int it = 0; it < 40; ++it) {
    // X += Pw X Pw^T
    double pmax = 0.0;
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += at(Pw, r, k) * at(X, k, c);
        tmp[(size_t)r * kD + c] = acc;
      }
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += at(tmp, r, k) * at(Pw, c, k);
        X[(size_t)r * kD + c] += acc;
      }
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += at(Pw, r, k) * at(Pw, k, c);
        tmp[(size_t)r * kD + c] = acc;
        pmax = std::max(pmax, std::fabs(acc));
      }
    Pw.swap(tmp);
    if (pmax < 1e-30) break;
  }
  // Cholesky X = P P^T (lower).
  std::vector<double> P((size_t)kD * kD, 0.0), Pi((size_t)kD * kD, 0.0);
  for (int j = 0; j < n; ++j) {
    double d = at(X, j, j);
    for (int k = 0; k < j; ++k) d -= at(P, j, k) * at(P, j, k);
    if (!(d > 1e-24 * at(X, j, j)) || !(d > 0.0)) return false;
    const double pj = std::sqrt(d);
    P[(size_t)j * kD + j] = pj;
    for (int i = j + 1; i < n; ++i) {
      double v = at(X, i, j);
      for (int k = 0; k < j; ++k) v -= at(P, i, k) * at(P, j, k);
      P[(size_t)i * kD + j] = v / pj;
    }
  }
  // P^-1 (lower triangular, forward substitution per column).
  for (int c = 0; c < n; ++c)
    for (int r = c; r < n; ++r) {
      double v = (r == c) ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) v -= at(P, r, k) * at(Pi, k, c);
      Pi[(size_t)r * kD + c] = v / at(P, r, r);
    }
  double nP = 0.0, nPi = 0.0;
  for (int r = 0; r < n; ++r) {
    double a = 0.0, b = 0.0;
    for (int c = 0; c < n; ++c) {
      a += std::fabs(at(P, r, c));
      b += std::fabs(at(Pi, r, c));
    }
    nP = std::max(nP, a);
    nPi = std::max(nPi, b);
  }
  if (!(nP * nPi < 1e8)) return false;
  // Gc[i] = P^-1 A^(tsub-1-i) B, i = tsub-1 down to 0.
  std::vector<double> g(Bv, Bv + kD), gn(kD);
  for (int i = tsub - 1; i >= 0; --i) {
    for (int r = 0; r < kD; ++r) {
      double v = 0.0;
      for (int c = 0; c < n && r < n; ++c) v += at(Pi, r, c) * g[c];
      tt->Gc[i / 2][r][i % 2] = (float)v;
    }
    for (int r = 0; r < n; ++r) {
      double v = 0.0;
      for (int c = 0; c < n; ++c) v += at(A, r, c) * g[c];
      gn[r] = v;
    }
    for (int r = 0; r < n; ++r) g[r] = gn[r];
  }
  // Q = T^-1 P (both lower triangular).
  for (int r = 0; r < kD; ++r)
    for (int c = 0; c < kD; ++c) {
      double v = 0.0;
      if (r < n && c < n)
        for (int k = c; k <= r; ++k) v += at(Ti, r, k) * at(P, k, c);
      tt->Q[r][c] = v;
    }
  return true;
}

// Block-diagonal form of the first 2*Sr states (the real stages): T block
// unit lower triangular with A T = T D, D = diag(A_kk).  Fills the carry part
// of the tables (G' = D^(tsub-1-i) B' with B' = T^-1 B, the powers of D, T);
// false when two stages share a pole pair or T is ill-conditioned.
bool modal_tables(const SosParams& p, int Sr, int tsub, TileTables* tt) {
  const int n = 2 * Sr;
  const std::vector<double> A = state_matrix(p, kS);  // 12 x 12
  auto Aat = [&](int r, int c) { return A[(size_t)r * kD + c]; };
  std::vector<double> T((size_t)kD * kD, 0.0);
  for (int i = 0; i < n; ++i) T[(size_t)i * kD + i] = 1.0;
  for (int j = 0; j < Sr; ++j) {
    for (int i = j + 1; i < Sr; ++i) {
      // A_ii X - X A_jj = -sum_{l=j}^{i-1} A_il T_lj
      double C[2][2] = {{0, 0}, {0, 0}};
      for (int l = j; l < i; ++l)
        for (int r = 0; r < 2; ++r)
          for (int c = 0; c < 2; ++c)
            for (int q = 0; q < 2; ++q)
              C[r][c] -= Aat(2 * i + r, 2 * l + q) * T[(size_t)(2 * l + q) * kD + 2 * j + c];
      // vec (column-major): (I (x) A_ii - A_jj^T (x) I) vec(X) = vec(C)
      double M[4][4], rhs[4];
      for (int cc = 0; cc < 2; ++cc)
        for (int rr = 0; rr < 2; ++rr) {
          const int row = cc * 2 + rr;
          rhs[row] = C[rr][cc];
          for (int c2 = 0; c2 < 2; ++c2)
            for (int r2 = 0; r2 < 2; ++r2) {
              const int col = c2 * 2 + r2;
              double v = 0.0;
              if (c2 == cc) v += Aat(2 * i + rr, 2 * i + r2);
              if (r2 == rr) v -= Aat(2 * j + c2, 2 * j + cc);
              M[row][col] = v;
            }
        }
      if (!solve4(M, rhs)) return false;
      for (int cc = 0; cc < 2; ++cc)
        for (int rr = 0; rr < 2; ++rr) T[(size_t)(2 * i + rr) * kD + 2 * j + cc] = rhs[cc * 2 + rr];
    }
  }
  // T^-1 (unit lower triangular: forward substitution per column).
  std::vector<double> Ti((size_t)kD * kD, 0.0);
  for (int c = 0; c < n; ++c)
    for (int r = 0; r < n; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int q = 0; q < r; ++q) s -= T[(size_t)r * kD + q] * Ti[(size_t)q * kD + c];
      Ti[(size_t)r * kD + c] = s;
    }
  double nT = 0.0, nTi = 0.0;
  for (int r = 0; r < n; ++r) {
    double a = 0.0, b2 = 0.0;
    for (int c = 0; c < n; ++c) {
      a += std::fabs(T[(size_t)r * kD + c]);
      b2 += std::fabs(Ti[(size_t)r * kD + c]);
    }
    nT = std::max(nT, a);
    nTi = std::max(nTi, b2);
  }
  if (!(nT * nTi < 1e8)) return false;
  // B of the realisation (includes the input gain), then B' = T^-1 B.
  double Bv[kD] = {0}, Bp[kD];
  cascade_state_step(p, kS, true, Bv, 1.0);
  for (int r = 0; r < kD; ++r) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += Ti[(size_t)r * kD + c] * Bv[c];
    Bp[r] = r < n ? s : 0.0;
  }
  auto mul = [](const double* X, const double* Y, double* Z) {
    const double z0 = X[0] * Y[0] + X[1] * Y[2], z1 = X[0] * Y[1] + X[1] * Y[3];
    const double z2 = X[2] * Y[0] + X[3] * Y[2], z3 = X[2] * Y[1] + X[3] * Y[3];
    Z[0] = z0;
    Z[1] = z1;
    Z[2] = z2;
    Z[3] = z3;
  };
  for (int k = 0; k < kS; ++k) {
    double Dk[4] = {0, 0, 0, 0};
    if (k < Sr)
      for (int q = 0; q < 4; ++q) Dk[q] = Aat(2 * k + q / 2, 2 * k + q % 2);
    // G'[i] block k = D_k^(tsub-1-i) B'_k, from i = tsub-1 down.
    double g0 = Bp[2 * k], g1 = Bp[2 * k + 1];
    for (int i = tsub - 1; i >= 0; --i) {
      tt->G[i][2 * k] = g0;
      tt->G[i][2 * k + 1] = g1;
      const double n0 = Dk[0] * g0 + Dk[1] * g1, n1 = Dk[2] * g0 + Dk[3] * g1;
      g0 = n0;
      g1 = n1;
    }
    // D_k^tsub by square-and-multiply, then repeated squaring per level.
    double R[4] = {1, 0, 0, 1}, Bq[4] = {Dk[0], Dk[1], Dk[2], Dk[3]};
    for (int e = tsub; e > 0; e >>= 1) {
      if (e & 1) mul(R, Bq, R);
      if (e > 1) mul(Bq, Bq, Bq);
    }
    for (int d = 0; d < 6; ++d) {
      for (int q = 0; q < 4; ++q) tt->Dp[d][k][q] = k < Sr ? R[q] : 0.0;
      mul(R, R, R);
    }
  }
  for (int r = 0; r < kD; ++r)
    for (int c = 0; c < kD; ++c) tt->T[r][c] = (r < n && c < n) ? T[(size_t)r * kD + c] : 0.0;
  return input_normal_tables(A, Bv, Ti, n, tsub, tt);
}

// Tap pairs of the packed SRC: branch ph, pair p = (h[2p - a], h[2p + 1 - a])
// with h[u] = taps[ph + L (TT - 1 - u)] (0 outside [0, TT) or past K) and a the
// branch's window parity.
template <class GEO>
void tap_pairs(const float* taps, int K, TileTables* tt) {
  for (int p = 0; p < kNPMax; ++p)
    for (int ph = 0; ph < 4; ++ph)
      for (int e = 0; e < 2; ++e) {
        float v = 0.f;
        const int a = ph < GEO::L ? branch_parity<GEO>(ph) : -1;
        if (a >= 0 && p < GEO::NP) {
          const int u = 2 * p + e - a;
          const int k = ph + GEO::L * (GEO::TT - 1 - u);
          if (u >= 0 && u < GEO::TT && k < K) v = taps[k];
        }
        tt->TP[p][ph][e] = v;
      }
}

// Class tables of the generic kernel (TileTables::seq / adv).
void gen_sequences(const float* taps, int K, int L, int M, int64_t c, TileTables* tt) {
  const int T = (K + L - 1) / L, C = gen_classes(L, M);
  const int64_t step = ((int64_t)kGenTS * M) % L, dphi = M % L;
  for (int k = 0; k < C; ++k) {
    int64_t phi = (c % L + k * step) % L;  // branch of the class's first output
    uint32_t bits = 0;
    for (int i = 0; i < kGenTS; ++i) {
      for (int u = 0; u < kGenTT; ++u) {
        const int64_t idx = phi + (int64_t)L * (T - 1 - u);
        tt->seq[k][i][u] = (u < T && idx < K) ? taps[idx] : 0.f;
      }
      if (phi + dphi >= L) bits |= 1u << i;
      phi = (phi + dphi) % L;
    }
    tt->adv[k] = bits;
  }
  tt->classes = C;
}

// Shifted class rows of k_chain_gct (TileTables::seqs).
void ct_sequences(const float* taps, int K, int L, int M, int64_t c, TileTables* tt) {
  const int T = (K + L - 1) / L, C = gen_classes(L, M);
  const int64_t step = ((int64_t)kGenTS * M) % L;
  for (int k = 0; k < C; ++k) {
    const int64_t phi0 = (c % L + k * step) % L;  // branch of the class's first output
    for (int i = 0; i < kGenTS; ++i) {
      const int64_t g = (int64_t)i * M / L;
      const int64_t d = (phi0 + (int64_t)i * M) / L - g;  // 0 or 1
      const int64_t phi = (phi0 + (int64_t)i * M) % L;
      const int sh = (int)((g & 1) + d);
      for (int v = 0; v < kCtRow; ++v) {
        const int u = v - sh;
        const int64_t idx = phi + (int64_t)L * (T - 1 - u);
        tt->seqs[k][i][v] = (v < kCtTaps && u >= 0 && u < T && idx < K) ? taps[idx] : 0.f;
      }
    }
  }
}

// Branch 0 of the L3/M2 tile a pure delay (src_part's DLY): its tap pairs are
// zero except the centre tap's slot, which is finite and non-zero.
template <class GEO>
bool delay_branch(const TileTables* tt) {
  if (branch_parity<GEO>(0) < 0) return false;
  constexpr int sl = dly_slot<GEO>();
  for (int p = 0; p < GEO::NP; ++p)
    for (int e = 0; e < 2; ++e) {
      const float v = tt->TP[p][0][e];
      const bool centre = 2 * p + e == sl;
      if (centre ? !(std::isfinite(v) && v != 0.f) : v != 0.f) return false;
    }
  // the pairs the DLY kernel skips (void_pair) hold zero taps
  for (int p = 0; p < GEO::NP; ++p)
    for (int ph = 1; ph < GEO::L; ++ph)
      if (void_pair<GEO>(p, ph) && (tt->TP[p][ph][0] != 0.f || tt->TP[p][ph][1] != 0.f))
        return false;
  return true;
}

// Tap rows of the per-phase kernel entry e (TileTables::tpw, chain_pp.h):
// slot t's row p, e = h[2 p + e - s(t)] of its branch phi(t), h[u] = taps[phi
// + L (T - 1 - u)] (0 outside [0, T) or past K).  With a delay branch (e.UC >=
// 0) its slots' rows must hold the centre tap alone (finite, non-zero) at 2 p
// + e = UC + s(t); false otherwise (the two-launch chain serves the call).
bool pp_rows(const float* taps, int K, int L, int M, int64_t c, const PpEntry& e,
             TileTables* tt) {
  const PpNeed n = pp_need(K, L, M, c);
  if (n.P * e.NP * 2 > kPpTapFloats) return false;
  float td = 0.f;
  for (int t = 0; t < n.P; ++t) {
    const int qc = t * n.MR / n.LR;
    const int delta = (n.r0 + t * n.MR) / n.LR - qc;
    const int phi = n.g * ((n.r0 + t * n.MR) % n.LR) + n.rho;
    const int sh = n.A + (qc & 1) + delta;
    const bool dly = e.UC >= 0 && t % n.LR == 0;
    for (int v = 0; v < 2 * e.NP; ++v) {
      const int u = v - sh;
      const int64_t idx = phi + (int64_t)L * (n.T - 1 - u);
      const float h = (u >= 0 && u < n.T && idx < K) ? taps[idx] : 0.f;
      tt->tpw[t * e.NP * 2 + v] = h;
      if (dly) {
        if (v == e.UC + sh) {
          if (!(std::isfinite(h) && h != 0.f) || (td != 0.f && h != td)) return false;
          td = h;
        } else if (h != 0.f) {
          return false;
        }
      }
    }
  }
  tt->pp_td = td;
  tt->pp_np = e.NP;
  return true;
}

// Whether a single-pass launch takes the three-launch mode: when the chained
// hand-off (~2.2 us a tile: one 441000-sample channel, 144 tiles, 0.31 ms)
// would bound it.  With t the tile's throughput cost at a full chip, chained
// ~ 2.2 us ntiles + 0.8 t B ntiles and three launches ~ 15 us + 1.4 t B
// ntiles (launch 1 redoes each tile's x, SRC, pass 1 and scan: ~0.4 t; two
// more launches).  Fitted on the cascade alone (t = 6 ns; both modes forced
// on one box at 1..4096 channels of 48000 and 441000 samples,
// profiles/r06_eq_alone_modes.txt) and checked on the SRC kernels (t = 7 ns,
// profiles/r06_three_launch_modes.txt).
bool three_launch(int64_t B, int64_t ntiles, double t_tile) {
  const double tiles = (double)B * (double)ntiles;
  return 15e-6 + 1.4 * t_tile * tiles < 2.2e-6 * (double)ntiles + 0.8 * t_tile * tiles;
}
constexpr double kTileCostIdent = 6e-9, kTileCostSrc = 7e-9;

}  // namespace

// The one mode decision behind chain_mode and launch_chain_tile.  The tile
// cost is the cascade's alone for the one-tap per-phase entry, an SRC's
// otherwise.
bool plan_three_launches(const TilePlan& tp, int64_t B) {
  bool ident = false;
  if (tp.kind == 4) {
    const PpEntry& e = kPpEntries[tp.pp];
    ident = e.LR == 1 && e.MR == 1 && e.NP == 1 && e.UC == 0;
  }
  return three_launch(B, tp.ntiles, ident ? kTileCostIdent : kTileCostSrc);
}

TileWs tile_ws(int64_t B, int64_t ntiles) {
  TileWs w;
  w.err_off = 0;  // include/dspcore.h: the workspace's first word
  w.st_off = 256;
  const size_t st = mul_sat((size_t)B, (size_t)ntiles, kD, sizeof(double));
  const size_t fl = mul_sat((size_t)B, (size_t)ntiles, sizeof(uint32_t));
  w.fl_off = st == SIZE_MAX ? SIZE_MAX : add_sat(w.st_off, align256(st));
  w.total = (fl == SIZE_MAX || w.fl_off == SIZE_MAX) ? SIZE_MAX : add_sat(w.fl_off, align256(fl));
  return w;
}

int64_t chain_tile_sub(int64_t n_in, int64_t n_out, int K, int L, int M, int64_t c, int S) {
  TilePlan tp;
  return tile_geometry(n_in, n_out, K, L, M, c, S, &tp) ? tp.tsub : 0;
}

int chain_mode(int64_t B, int64_t n_in, int64_t n_out, int K, int L, int M, int64_t c, int S) {
  TilePlan tp;
  if (B < 1 || !tile_geometry(n_in, n_out, K, L, M, c, S, &tp)) return 0;
  return plan_three_launches(tp, B) ? 3 : 1;
}

size_t chain_tile_workspace_bytes(int64_t B, int64_t n_in, int64_t n_out, int K, int L, int M,
                                  int64_t c, int S) {
  // The status header (256 B, word 0: hand-off status) always exists.
  TilePlan tp;
  if (B <= 0 || !tile_geometry(n_in, n_out, K, L, M, c, S, &tp)) return 256;
  return tile_ws(B, tp.ntiles).total;
}

size_t chain_tile_tables_bytes() { return sizeof(TileTables); }

int chain_tile_tables(void* out, size_t out_bytes, int64_t n_in, int64_t n_out, const float* taps,
                      int K, int L, int M, int64_t c, const double* sos, int S, uint64_t* key) {
  if (key) *key = 0;
  TilePlan tp;
  if (!tile_geometry(n_in, n_out, K, L, M, c, S, &tp)) return kNotFused;
  DSP_REQUIRE(out && out_bytes >= sizeof(TileTables), "tables buffer too small: %zu < %zu bytes",
              out_bytes, sizeof(TileTables));
  DSP_REQUIRE(taps && sos, "null pointer");
  SosParams p;
  if (!realize(sos, S, &p)) return kNotFused;  // a b0 == 0 band: no NORM form
  TileTables* tt = static_cast<TileTables*>(out);
  std::memset(tt, 0, sizeof(TileTables));
  if (!modal_tables(p, S, (int)tp.tsub, tt)) return kNotFused;  // shared poles: two-launch
  // The kernels' finite arithmetic uses the flushed taps (common.h,
  // kTapFlushRel); the caller's own taps go to the kernels' non-finite path.
  std::vector<float> ft(taps, taps + K);
  const float thr = tap_flush_threshold(taps, K, L);
  for (float& t : ft) t = flush_tap(t, thr);
  tt->flush_thr = thr;
  bool dly = false;
  if (tp.kind == 1) {
    tap_pairs<Geo3241>(ft.data(), K, tt);
    dly = delay_branch<Geo3241>(tt);
  } else if (tp.kind == 4) {
    // every entry with a delay branch needs it (no plain instantiation)
    if (!pp_rows(ft.data(), K, L, M, c, kPpEntries[tp.pp], tt)) return kNotFused;
    tt->pp_geo = tp.pp;
  } else {
    gen_sequences(ft.data(), K, L, M, c, tt);
  }
  if (tp.kind == 3) ct_sequences(ft.data(), K, L, M, c, tt);
  for (int k = 0; k < kS; ++k) {
    // NORM form (realize() above refused b0 == 0): g = 1, {c1, c2, a1, a2}
    for (int q = 0; q < 4; ++q) tt->cf[k][q] = p.c[k][q + 1];
  }
  tt->gain = p.G;
  // pass 2 applies the gain at the output (pass2_cascade): states in 1 / gain
  // (Q for the float32 pass 1, G for the float64 one of the per-phase kernels)
  for (int r = 0; r < kD; ++r)
    for (int c = 0; c < kD; ++c) tt->Q[r][c] /= p.G;
  for (int i = 0; i < 64; ++i)
    for (int c = 0; c < kD; ++c) tt->G[i][c] /= p.G;
  tt->tsub = (int32_t)tp.tsub;
  tt->np = tp.kind == 1 ? Geo3241::NP : 0;
  tt->L = L;
  tt->M = M;
  tt->K = K;
  tt->S = S;
  tt->key = dly ? dly_key(tables_key(tp, n_in, n_out, K, L, M, c, sos, S))
                : tables_key(tp, n_in, n_out, K, L, M, c, sos, S);
  if (key) *key = tt->key;
  return DSP_OK;
}

}  // namespace dsp
