"""Every per-phase single-pass chain kernel (csrc/chain_pp.h: k_chain_pp<G>,
k_chain_pp3<G, 1>, k_chain_pp3<G, 2> and k_chain_pp_repair<G> of each of the
geometries of csrc/chain_pp_list.h) in all three modes at its row and tile
edges, and the rows and ratios that reach a geometry at window alignments no
long slider row has.

The geometries are parsed from chain_pp_list.h (test_pp_model._entries), one
parametrised case per entry; an entry's representative (L, M, K) is the first
ratio of its line's comment, so an entry added later is picked up.  Entry 0 is
the cascade alone (the SRC bypass, L = M = 1, as the one-tap SRC).

1. test_entry_every_mode_at_length_edges: with TILE = 64 TS, rows (multiples
   of 4 samples) of the smallest length with n_in L >= K (one ragged tile, most
   of the window outside the row), the largest with n_out <= TILE, the smallest
   with n_out > TILE, and two full tiles with about a third of a third one,
   n_out off every multiple of 4 and of TS.  Integer upsampling (M' = 1: n_out
   = n_in L / M, a multiple of 4) cannot be off a multiple of 4: entries 0, 1,
   9, 10, 14, 20, 24, 31, 34 and 41 of the list as it stands (the test derives
   it from M').  B = 5: two rows of noise, one of noise times 8 into the clip,
   one silent in its first half, one all zeros.  dsp_chain_path 2 (chained
   tiles), 4 (three launches) and 1 (two-launch chain) on one Chain: the
   kernels by their trace names, y of 2 and 4 equal to 1's, z within 2e-6 and
   |X| within 1e-5 of the peak (test_gpu_pp.py's limits), every row against the
   float64 oracle (y 2e-6 max(1, max|y|), z 1e-5, |X| 1e-5 of its peak), the
   zero row exactly zero.
2. test_entry_repair_kernel: the two-tiles-and-a-third length on paths 2 and
   4 with one inf or NaN per row at the places the repair kernel's own window
   indexing matters (the row's first and last samples, the first sample of
   tile 1's window, the last sample tile 0's lane 63 reads, both signs in one
   window) and one clean row: masks equal to path 1's and to the oracle's,
   finite y equal to path 1's, finite z within 2e-6, the clean row bitwise
   what it is in a batch without bad values.
3. test_short_rows_and_reduced_ratios: every slider ratio at 4 samples and at
   the largest multiple of 4 with n_in L < K (c = (n_in L - 1) // 2, n_out =
   ceil(K / M)), and ratios outside the sliders that reduce to a listed
   geometry (gcd up to 32, K up to 2561) at those two lengths and the ragged
   three-tile one.  The trace must agree with the host's answer
   (dsp_chain_tile_len, dsp_chain_tile_tables); whatever runs is checked
   against the oracle, and where a per-phase kernel serves the case paths 2
   and 4 against path 1.  MUST_SERVE names the cases a per-phase kernel has to
   serve, so that this cannot turn into a test of the two-launch chain.

Every case prints the lengths, the kernels its traces showed and its worst
y, z and |X| errors next to their limits.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from test_gpu_nonfinite import _same
from test_gpu_pp import EQ_ATOL, MAG_RTOL, SRC_ATOL, _chain_path, _traced
from test_gpu_wide_batch import _fin_err, _nfft_for, _pool_map
from test_pp_model import (NON_SLIDER, SLIDER, _entries, _entry_ratios, _gains, _host_answer,
                           _n_out, _ragged_length, _short_lengths, _xa0)

pytestmark = pytest.mark.gpu

FS = 48000
B = 5
PATH_Z_ATOL = 2e-6           # z of paths 2 and 4 against path 1 (test_gpu_pp.py)
ENTRIES = _entries()
RATIOS = _entry_ratios()
ENTRY_IDS = [f"e{e[0]}-{L}/{M}K{K}" for e, (L, M, K) in zip(ENTRIES, RATIOS)]
NAN, INF = float("nan"), float("inf")


# --------------------------------------------------------------------------- helpers
def _plan(n_in, L, M, K):
    from dspcore import design
    if L == 1 and M == 1:     # the SRC bypass as the one-tap SRC (dspcore.chain.Chain)
        return design.SrcPlan(1, 1, 1, np.ones(1), 0, n_in, n_in, FS)
    return design.src_plan(n_in, FS, M, L, K)


def _chain(gpu, L, M, K, n_in, n_fft, batch=B):
    from dspcore.chain import Chain, ChainConfig
    return Chain(ChainConfig(n_in, FS, L, M, K, _gains(), n_fft=n_fft), batch, gpu)


def _pp_entry(ch):
    """The per-phase entry the chain's tables were built for, or -1."""
    from test_abi import _tables_dtype
    if ch.tile_len <= 0 or ch.tile_tables is None:
        return -1
    tb = ch.tile_tables.cpu().numpy().view(_tables_dtype())[0]
    return int(tb["pp_geo"]) if int(tb["pp_np"]) > 0 else -1


def _rows(n_in, seed):
    """[5, n_in]: two rows of noise, one times 8 (into the clip), one silent
    in its first half, one all zeros."""
    x = np.random.default_rng(seed).uniform(-1, 1, (B, n_in)).astype(np.float32)
    x[2] *= 8.0
    x[3, : n_in // 2] = 0.0
    x[4] = 0.0
    x.setflags(write=False)
    return x


_REF = {}


def _oracle(key, x, L, M, K, n_fft):
    """The oracle's (y, z, |X|) of every row of x, once per key, read-only."""
    if key not in _REF:
        from oracle import dsp_ref_cpu as orc

        def one(row):
            y, z, _, mag, _ = orc.chain(row.astype(np.float64), FS, L, M, _gains(),
                                        None if L == M == 1 else K, n_fft)
            return y, z, mag
        out = _pool_map(one, list(x))
        for item in out:
            for a in item:
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _run(ch, xd, path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with _chain_path(path):
            (y, z, m), names = _traced(lambda: ch.run(xd))
    return y.cpu().numpy(), z.cpu().numpy(), m.cpu().numpy(), names


def _y_tol(ry):
    fin = np.isfinite(ry)
    return SRC_ATOL * max(1.0, float(np.max(np.abs(ry[fin]))) if fin.any() else 1.0)


def _against_oracle(tag, out, ref, worst):
    """Rows of (y, z, |X|) against the oracle's within the project's
    tolerances, non-finite masks exactly; folds the worst errors (y as a
    multiple of its limit's scale) into `worst`."""
    y, z, mag = out[:3]
    assert y.shape[1] == ref[0][0].size, (tag, y.shape, ref[0][0].size)
    for b, (ry, rz, rm) in enumerate(ref):
        worst[0] = max(worst[0], _fin_err(y[b], ry) / (_y_tol(ry) / SRC_ATOL))
        worst[1] = max(worst[1], _fin_err(z[b], rz))
        worst[2] = max(worst[2], _fin_err(mag[b], rm, rel=True))
        _same(y[b], ry, _y_tol(ry), f"{tag} row {b} y against the oracle")
        _same(z[b], rz, EQ_ATOL, f"{tag} row {b} z against the oracle", masks=("nan",))
        _same(mag[b], rm, MAG_RTOL, f"{tag} row {b} |X| against the oracle", rel=True)


def _assert_names(tag, path, names):
    if path == 2:
        assert "chain_tile" in names and "chain_tile_agg" not in names, (tag, names)
        assert "src_poly" not in names, (tag, names)
    elif path == 4:
        assert "chain_tile_agg" in names and "chain_tile_carry" in names, (tag, names)
        assert "chain_tile" in names and "src_poly" not in names, (tag, names)
    else:
        assert "chain_tile" not in names and "chain_tile_agg" not in names, (tag, names)


def _check_modes(tag, ch, x, ref):
    """Paths 2, 4 and 1 of one Chain on the finite batch x (part 1's checks).
    Returns (kernels seen, worst errors [y / scale, z, |X| rel, z path, |X|
    path])."""
    xd = torch.tensor(x, device=ch.device)
    outs ={p: _run(ch, xd, p) for p in (1, 2, 4)}
    assert ch.handoff_ok(), tag
    worst = [0.0] * 5
    seen = set()
    y1, z1, m1, _ = outs[1]
    for p in (2, 4, 1):
        y, z, m, names = outs[p]
        _assert_names(f"{tag} path {p}", p, names)
        if p != 1:
            seen |= set(names)
            assert np.array_equal(y, y1), (tag, p, float(np.max(np.abs(y - y1))))
            ez = float(np.max(np.abs(z - z1)))
            em = float(np.max(np.abs(m - m1)))
            peak = float(np.max(np.abs(m1)))
            worst[3] = max(worst[3], ez)
            worst[4] = max(worst[4], em / max(peak, 1e-30))
            assert ez <= PATH_Z_ATOL, f"{tag} path {p}: z is {ez:.3g} from path 1's"
            assert em <= MAG_RTOL * peak, f"{tag} path {p}: |X| is {em:.3g} from path 1's ({peak:.3g})"
        _against_oracle(f"{tag} path {p}", (y, z, m), ref, worst)
        for what, a in (("y", y), ("z", z), ("|X|", m)):
            assert not a[B - 1].any(), f"{tag} path {p}: the all-zero row's {what} is not zero"
    return seen, worst


def _report(tag, worst):
    print(f"{tag}: y {worst[0]:.2e} max(1, max|y|) (limit {SRC_ATOL:.0e} max(1, max|y|)), "
          f"z {worst[1]:.2e} (limit {EQ_ATOL:.0e}), |X| {worst[2]:.2e} (limit {MAG_RTOL:.0e} of the "
          f"peak); against path 1: z {worst[3]:.2e} (limit {PATH_Z_ATOL:.0e}), |X| {worst[4]:.2e} "
          f"(limit {MAG_RTOL:.0e} of the peak)")


def _edge_lengths(L, M, K, TS):
    """[(what, n_in)] of part 1 for a geometry with tiles of 64 TS outputs."""
    tile = 64 * TS
    smallest = -(-K // L)
    smallest += -smallest % 4
    full = (tile * M // L) // 4 * 4
    while _n_out(full, L, M, K) > tile:
        full -= 4
    while _n_out(full + 4, L, M, K) <= tile:
        full += 4
    return [("smallest", smallest), ("full tile", full), ("tile + a little", full + 4),
            ("two tiles + ragged", _ragged_length(L, M, K, TS))]


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("idx", range(len(ENTRIES)), ids=ENTRY_IDS)
def test_entry_every_mode_at_length_edges(gpu, idx):
    L, M, K = RATIOS[idx]
    _, LR, MR, TS = ENTRIES[idx][:4]
    g = math.gcd(L, M)
    assert (L // g, M // g) == (LR, MR), "the comment's first ratio reduces to the entry's"
    tile = 64 * TS
    lens = _edge_lengths(L, M, K, TS)
    n_outs = [_n_out(n, L, M, K) for _, n in lens]
    assert lens[0][1] * L >= K > (lens[0][1] - 4) * L and n_outs[0] <= tile
    assert n_outs[1] <= tile < n_outs[2] and lens[2][1] == lens[1][1] + 4
    assert 2 * tile < n_outs[3] < 3 * tile
    # off every multiple of 4 and of TS, but for integer upsampling (M' = 1)
    assert (n_outs[3] % 4 and n_outs[3] % TS) or MR == 1, (n_outs[3], TS)
    total, seen_all = [0.0] * 5, set()
    for (what, n_in), n_out in zip(lens, n_outs):
        assert n_in % 4 == 0
        n_fft = _nfft_for(n_out)
        ch = _chain(gpu, L, M, K, n_in, n_fft)
        assert ch.n_out == n_out and ch.tile_len == TS and _pp_entry(ch) == idx, \
            (what, n_in, ch.n_out, ch.tile_len, _pp_entry(ch))
        x = _rows(n_in, 1000 * idx + n_in)
        ref = _oracle(("edge", idx, n_in), x[:B - 1], L, M, K, n_fft)
        tag = f"entry {idx} {L}/{M} K{K} {what} n_in {n_in} n_out {n_out}"
        seen, worst = _check_modes(tag, ch, x, ref)
        _report(tag, worst)
        seen_all |= seen
        total = [max(a, b) for a, b in zip(total, worst)]
    print(f"entry {idx} {L}/{M} K{K}: n_in {[n for _, n in lens]} n_out {n_outs} kernels "
          f"{sorted(seen_all)}")
    assert {"chain_tile", "chain_tile_agg", "chain_tile_carry", "chain_repair"} <= seen_all


# --------------------------------------------------------------------------- 2
def _bad_rows(n_in, plan, entry, seed):
    """[6, n_in] with one bad value (or pair) per row, the last row clean, and
    the (position, value) lists."""
    _, LR, MR, TS, NP = entry[:5]
    LS = TS * MR // LR
    xa0 = _xa0(plan)
    W = (((TS - 1) * MR // LR) & ~1) + 2 * NP      # a lane's window (chain_pp.h, PpGeo::W)
    xa1 = xa0 + 64 * LS                            # first sample of tile 1's window
    last63 = xa0 + 63 * LS + W - 1                 # last sample tile 0's lane 63 reads
    assert 0 < xa1 < n_in and 0 <= last63 < n_in, (xa0, xa1, last63, n_in)
    specs = [[(0, NAN)], [(n_in - 1, -INF)], [(xa1, INF)], [(last63, NAN)],
             [(n_in // 2, INF), (n_in // 2 + 3, -INF)], []]
    x = np.random.default_rng(seed).uniform(-1, 1, (len(specs), n_in)).astype(np.float32)
    clean = x.copy()
    for r, sp in enumerate(specs):
        for pos, val in sp:
            x[r, pos] = val
    x.setflags(write=False)
    clean.setflags(write=False)
    return x, clean, specs


@pytest.mark.parametrize("idx", range(len(ENTRIES)), ids=ENTRY_IDS)
def test_entry_repair_kernel(gpu, idx):
    L, M, K = RATIOS[idx]
    entry = ENTRIES[idx]
    TS = entry[3]
    n_in = _ragged_length(L, M, K, TS)
    n_out = _n_out(n_in, L, M, K)
    n_fft = _nfft_for(n_out)
    x, clean, specs = _bad_rows(n_in, _plan(n_in, L, M, K), entry, 77 + idx)
    R = x.shape[0]
    ch = _chain(gpu, L, M, K, n_in, n_fft, batch=R)
    assert ch.tile_len == TS and _pp_entry(ch) == idx
    ref = _oracle(("bad", idx, n_in), x, L, M, K, n_fft)
    xd, cd = torch.tensor(x, device=gpu), torch.tensor(clean, device=gpu)
    y1, z1, m1, names1 = _run(ch, xd, 1)
    _assert_names("path 1", 1, names1)
    worst = [0.0] * 5
    seen = set()
    for p in (2, 4):
        tag = f"entry {idx} {L}/{M} K{K} n_in {n_in} path {p}"
        y, z, m, names = _run(ch, xd, p)
        yc, zc, mc, _ = _run(ch, cd, p)
        assert ch.handoff_ok(), tag
        _assert_names(tag, p, names)
        assert "chain_repair" in names, (tag, names)
        seen |= set(names)
        for r in range(R):
            rt = f"{tag} row {r} {specs[r]}"
            _same(y[r], y1[r], 0.0, rt + " y against path 1")
            _same(z[r], z1[r], PATH_Z_ATOL, rt + " z against path 1", masks=("nan",))
            worst[3] = max(worst[3], _fin_err(z[r], z1[r]))
            assert np.array_equal(np.isnan(m[r]), np.isnan(m1[r])), rt + " |X| NaN mask"
        _against_oracle(tag, (y, z, m), ref, worst)
        # the clean row: bitwise what it is without the bad rows beside it
        for what, a, c in (("y", y, yc), ("z", z, zc), ("|X|", m, mc)):
            assert np.array_equal(a[R - 1].view(np.int32), c[R - 1].view(np.int32)), \
                f"{tag}: the clean row's {what} depends on the other rows"
    print(f"entry {idx} {L}/{M} K{K}: n_in {n_in} n_out {n_out} bad values {specs[:-1]} kernels "
          f"{sorted(seen)}")
    _report(f"entry {idx} non-finite", worst)
    assert {"chain_tile", "chain_tile_agg", "chain_repair"} <= seen


# --------------------------------------------------------------------------- 3
# (L, M, n_in; None: the ragged three-tile length) a per-phase kernel must serve
MUST_SERVE = {(2, 4, 4), (3, 5, 4), (16, 24, 4), (56, 64, 4)} | {(L, M, None) for L, M in NON_SLIDER}
RATIO3 = SLIDER + NON_SLIDER


@pytest.mark.parametrize("L,M", RATIO3, ids=[f"{L}/{M}" for L, M in RATIO3])
def test_short_rows_and_reduced_ratios(gpu, L, M):
    from dspcore import _lib, design
    lib = _lib.load()
    K = design.default_num_taps(L, M)
    cases = [(n, n) for n in _short_lengths(L, K)]
    if (L, M) in NON_SLIDER:
        ts, _, pe = _host_answer(lib, design.src_plan(4096, FS, M, L, K), 4096)
        assert pe >= 0, f"{L}/{M}: no per-phase kernel at a long row (tile_len {ts})"
        cases.append((None, _ragged_length(L, M, K, ts)))
    served = []
    for key, n_in in cases:
        n_out = _n_out(n_in, L, M, K)
        if key is not None:
            assert n_in * L < K and n_out == -(-K // M)
        n_fft = 2048 if n_out <= 2048 else _nfft_for(n_out)
        tag = f"{L}/{M} K{K} n_in {n_in} n_out {n_out}"
        ch = _chain(gpu, L, M, K, n_in, n_fft)
        host_ts, _, host_pe = _host_answer(lib, ch.src, n_in)
        pe = _pp_entry(ch)
        assert (ch.tile_len, pe) == (host_ts, host_pe), (tag, ch.tile_len, pe, host_ts, host_pe)
        if (L, M, key) in MUST_SERVE:
            assert pe >= 0, f"{tag}: no per-phase kernel serves it (tile_len {ch.tile_len})"
        x = _rows(n_in, 7 * n_in + 64 * L + M)
        ref = _oracle(("short", L, M, n_in), x[:B - 1], L, M, K, n_fft)
        out = _run(ch, torch.tensor(x, device=gpu), 0)
        names = out[3]
        if ch.tile_len > 0:      # a single-pass kernel serves the call
            assert "chain_tile" in names and "src_poly" not in names, (tag, names)
        else:
            assert "src_poly" in names and "chain_tile_agg" not in names, (tag, names)
        assert ch.handoff_ok(), tag
        worst = [0.0] * 5
        _against_oracle(tag + " default path", out, ref, worst)
        for what, a in (("y", out[0]), ("z", out[1]), ("|X|", out[2])):
            assert not a[B - 1].any(), f"{tag}: the all-zero row's {what} is not zero"
        if pe >= 0:
            g = math.gcd(L, M)
            assert ENTRIES[pe][1:3] == (L // g, M // g)
            seen, w = _check_modes(tag, ch, x, ref)
            assert {"chain_tile", "chain_tile_agg", "chain_repair"} <= seen
            worst = [max(a, b) for a, b in zip(worst, w)]
            served.append((n_in, pe))
        _report(tag + (f" entry {pe}" if pe >= 0 else f" (tile_len {ch.tile_len}: "
                                                      f"{sorted(set(names))})"), worst)
    print(f"{L}/{M}: served by a per-phase kernel (n_in, entry): {served}")
