"""Wide batches of short rows through every kernel that maps channels (or
transforms) to workgroups, waves and lanes by more than `b = blockIdx.x`.

Every kernel here derives its channel from its ids: the persistent config-5
kernel walks channel groups grid-stride with the next channel's window in
flight (csrc/chain_tile.hip, k_chain_gcp), the repair kernels take 64 channels
per wave on a grid capped at 1024 workgroups (csrc/chain_tile.h,
repair_channels), the spectrum / STFT kernel is a persistent grid of two
transforms per workgroup (csrc/fft_spec.hip, k_spec_stream), the SRC launches in
parts of 65535 rows (csrc/src_poly.hip, launch_src), the FFT's non-finite
repair takes 256 transforms per workgroup (csrc/fft_nf.hip, k_nf_small), the
general cascade flattens B * C lanes over blocks of 256 (csrc/iir.hip), and
the paired tail tile, the generic kernels' groups of four waves and the
per-phase kernels all have a partial last wave or group.  All of that can go
wrong at short rows as long as the batch is wide, so the rows here are 96 to
about 5000 samples and the batches up to 262405 channels.

Method (families A-E, G): R = 61 base rows -- 49 finite ones (uniform noise,
three scaled by 40 into the clip, three silent in their first half) and 12
with NaN, +inf or -inf at the places tests/test_gpu_nonfinite.py uses (a delay
output's window edges, a tile boundary, a sub-chunk boundary, the first and
last samples, both signs in one window), placed for the geometry under test.
The 61-row batch runs once per case and path with the wide batch's plan
(Chain(..., plan_batch=B): its single-pass mode and chunking) and is checked
row by row against the float64 oracle (oracle/dsp_ref_cpu.py) within the
project's tolerances (y 2e-6 max(1, max|y|), z 1e-5, |X| 1e-5 max|X|), the
non-finite masks exactly.  Then x_wide = base[arange(B) % 61] runs, and EVERY
row of y, z and |X| must equal its base row bitwise (NaN masks equal, the rest
compared as bits): rows are bitwise independent of the batch within a mode,
and the persistent kernel is bitwise the chained one.
61 is prime, so b % 61 visits every residue of 2, 4, 64 and 256: every base
row lands in every wave slot and lane, and a wrong channel index anywhere
shows as a mismatched row.  Families that take finite input only (E2, G) use
the 49 finite rows.

Family F (the spectrum / STFT kernel) needs no periodic trick: one channel
with many overlapping frames, every frame against numpy's float64 rfft of the
Hann-windowed frame.

Each test asserts the condition its shape is there for (the kernel that ran by
its trace names, tile counts, pairing, grid arithmetic against the device's CU
count) and prints its wall time and the worst base-row error next to the
tolerance.
"""
import os
import time
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from test_gpu_nonfinite import (EQ_ATOL, INF, MAG_RTOL, NAN, SRC_ATOL, _quiet, _same,
                                _same_complex, orc_fft)
from test_gpu_parity import _chain_path

pytestmark = pytest.mark.gpu

R = 61            # base rows; prime: b % 61 visits every residue of 2, 4, 64, 256
N_BAD = 12
BAD_AT = tuple(5 * i + 3 for i in range(N_BAD))          # base rows that carry inf / NaN
SCALED = (1, 17, 32)                                     # finite rows driven into the clip
HALF_SILENT = (2, 19, 36)                                # finite rows silent in their first half
FS48, FS44 = 48000, 44100
WAVE = 64
REPAIR_GROUPS = 1024     # csrc/chain_tile.hip kRepairGroups
GRID_Y = 65535           # csrc/src_poly.hip kMaxGridY
B_Y = GRID_Y + 1 + 64 + 3          # 65603: past the SRC's grid-y limit and 1024 repair waves
B_GEN = 262144 + 256 + 5           # past 1024 generic repair groups of 256 channels


def _gains():
    from oracle import dsp_ref_cpu as orc
    return orc.CONFIG3_GAINS


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _ceil(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- rows
def _bad_specs(plan, n, tile, sub):
    """The (position, value) lists of test_gpu_nonfinite._rows for a row of n
    inputs of the SRC `plan`, whose single-pass kernel has tiles of `tile` and
    sub-chunks of `sub` outputs; positions clamped into the row.  A row shorter
    than a tile puts the tile-boundary entries on a sub-chunk boundary."""
    L, M, c, n_out = plan.L, plan.M, plan.c_offset, plan.n_out
    T = -(-plan.K // L)

    def q(m):                                  # last input sample output m reads
        return (m * M + c) // L

    m_d = next((m for m in range(n_out // 3, n_out) if (m * M + c) % L == 0), n_out // 2)
    qd = q(m_d)
    if n_out > tile:
        m_t = 2 * tile if 2 * tile < n_out - tile else tile
    else:
        m_t = max(sub, (n_out // 2) // sub * sub)
    m_s = m_t + 5 * sub if m_t + 5 * sub < n_out else m_t + sub
    if m_s >= n_out:
        m_s = m_t
    specs = [
        [(qd - (T - 1), NAN)],                  # the delay output's window edge
        [(qd, INF)],                            # its other edge
        [(qd - (T - 1) // 2 - 1, -INF)],        # off its centre
        [(q(m_t), INF), (q(m_t) + 3, -INF)],    # both signs, one window: NaN
        [(q(m_t - 1), NAN)],                    # last sample of the tile before
        [(q(m_t) - (T - 1), -INF)],             # first sample of the tile's first window
        [(q(m_s), INF), (q(m_s) - 1, INF)],     # sub-chunk boundary, one sign
        [(0, NAN)],
        [(n - 1, -INF)],
        [(n - 1, NAN)],
        [(n - 5, INF), (n - 3, INF)],
        [(n // 2, NAN), (n // 2 + 7, INF)],
    ]
    assert len(specs) == N_BAD
    return [[(min(max(int(p), 0), n - 1), v) for p, v in sp] for sp in specs]


def _base_rows(n, seed, specs=None):
    """[61, n] float32 (specs: the 12 bad rows' lists) or [49, n] (finite
    only), and the list of every row's (position, value) entries."""
    rows = R if specs is not None else R - N_BAD
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.9, 0.9, (rows, n)).astype(np.float32)
    for r in SCALED:
        x[r] *= 40.0
    for r in HALF_SILENT:
        x[r, : n // 2] = 0.0
    placed = [[] for _ in range(rows)]
    if specs is not None:
        assert not set(BAD_AT) & (set(SCALED) | set(HALF_SILENT))
        for r, sp in zip(BAD_AT, specs):
            for pos, val in sp:
                x[r, pos] = val
            placed[r] = sp
    x.setflags(write=False)
    return x, placed


def _pool_map(fn, rows):
    """fn over the rows on a few threads (numpy's convolve and scipy's lfilter
    release the GIL), numpy's warnings off in every worker."""
    def quiet(row):
        with np.errstate(all="ignore"):
            return fn(row)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            return list(pool.map(quiet, rows))


_ORACLE = {}


def _oracle(key, fn, x):
    """fn(row as float64) for every base row, computed once per key and shared
    (the arrays read-only)."""
    if key not in _ORACLE:
        out = _pool_map(lambda row: fn(row.astype(np.float64)), list(x))
        for item in out:
            for a in (item if isinstance(item, tuple) else (item,)):
                a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


# --------------------------------------------------------------------------- checks
def _fin_err(got, want, rel=False):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    fin = np.isfinite(got) & np.isfinite(want)
    if not fin.any():
        return 0.0
    err = float(np.max(np.abs(got[fin] - want[fin])))
    return err / max(float(np.max(np.abs(want[fin]))), 1e-30) if rel else err


def _y_tol(want):
    fin = np.isfinite(want)
    return SRC_ATOL * max(1.0, float(np.max(np.abs(want[fin]))) if fin.any() else 1.0)


def _check_base(label, placed, ref, y=None, z=None, mag=None):
    """Base rows against the oracle's (y, z, mag) row by row: non-finite masks
    exactly, finite values within the project's tolerances.  Returns the
    worst (y error / its tolerance scale, z error, |X| relative error)."""
    worst = [0.0, 0.0, 0.0]
    for r, (ry, rz, rm) in enumerate(ref):
        tag = f"{label} base row {r} {placed[r]}"
        if y is not None:
            worst[0] = max(worst[0], _fin_err(y[r], ry) / (_y_tol(ry) / SRC_ATOL))
            _same(y[r], ry, _y_tol(ry), tag + " y")
        if z is not None:
            worst[1] = max(worst[1], _fin_err(z[r], rz))
            _same(z[r], rz, EQ_ATOL, tag + " z", masks=("nan",))
        if mag is not None:
            worst[2] = max(worst[2], _fin_err(mag[r], rm, rel=True))
            _same(mag[r], rm, MAG_RTOL, tag + " |X|", masks=("nan", "+inf", "-inf"), rel=True)
    return worst


def _assert_rows_periodic(wide, base, what, rows=R):
    """Every row b of `wide` is bitwise row b % rows of `base` (device
    tensors): NaN masks equal, everything else compared as bits."""
    assert wide.shape[1:] == base.shape[1:] and base.shape[0] == rows, (what, wide.shape, base.shape)
    B = wide.shape[0]
    step = max(1, (64 << 20) // max(1, 4 * wide[0].numel()))     # <= 64 MiB per piece
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        got = wide[b0:b1]
        want = base[torch.arange(b0, b1, device=wide.device) % rows]
        if got.is_complex():
            got, want = torch.view_as_real(got), torch.view_as_real(want)
        gn, wn = torch.isnan(got), torch.isnan(want)
        zero = torch.zeros((), dtype=got.dtype, device=got.device)
        same = (gn == wn) & (torch.where(gn, zero, got).contiguous().view(torch.int32)
                             == torch.where(wn, zero, want).contiguous().view(torch.int32))
        if not bool(same.all()):
            bad = (~same.reshape(b1 - b0, -1)).any(dim=1).nonzero().flatten() + b0
            first = int(bad[0])
            col = int((~same[first - b0].reshape(-1)).nonzero().flatten()[0])
            raise AssertionError(
                f"{what}: {bad.numel()} of rows {b0}..{b1 - 1} differ from their base rows; first "
                f"row {first} (base row {first % rows}) at flat element {col}; rows "
                f"{bad[:12].tolist()}")


def _collapse(names):
    """Trace names with immediate repeats folded (a launch in parts)."""
    return [n for i, n in enumerate(names) if i == 0 or n != names[i - 1]]


def _trace(fn):
    """(fn(), kernel names the library launched)."""
    from dspcore import _lib
    _lib.trace_enable(True)
    _lib.trace_read()
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [n for n, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    return out, names


def _free():
    torch.cuda.empty_cache()


def _widen(base_d, B):
    return base_d[torch.arange(B, device=base_d.device) % base_d.shape[0]]


# --------------------------------------------------------------------------- chain cases
def _nfft_for(n_out):
    """The largest power of two <= 2048 the spectrum's centre segment holds."""
    room = n_out - n_out // 2
    return min(2048, 1 << (room.bit_length() - 1))


# name: (fs, L, M, K, n_in, n_fft (None: _nfft_for), B (callable of the CU count), tile_len)
CHAIN_CASES = {
    # A: L3/M2 at the default K = 121 -- k_chain_tile, k_chain_tile_pair, k_chain_tile_repair
    "A1": (FS48, 3, 2, None, 2104, None, lambda cu: 131, 48),
    "A2": (FS48, 3, 2, None, 4096, None, lambda cu: 131, 48),
    "A3": (FS48, 3, 2, None, 96, 64, lambda cu: B_Y, 48),
    # B: the generic kernel k_chain_gen and its repair, four waves per group
    "B1-5/4": (FS48, 5, 4, 31, 3200, None, lambda cu: 256 + 5, 32),
    "B1-2/3": (FS48, 2, 3, 15, 3200, None, lambda cu: 256 + 5, 32),
    # (104 inputs, not 96: the 64-point centre segment needs n_out - n_out // 2 >= 64)
    "B2": (FS48, 5, 4, 31, 104, 64, lambda cu: B_GEN, 32),
    # C: config 5's ratio -- k_chain_gct / k_chain_gcp (three rounds at least of the
    # persistent grid, whose residency amdgpu_waves_per_eu(3) bounds at 3 * CUs groups)
    "C": (FS44, 160, 147, 1023, 4800, None, lambda cu: 4 * (7 * cu + 37) + 1, 32),
    # D: the per-phase kernels at the default tap rule
    "D-2/1": (FS48, 2, 1, None, 3000, None, lambda cu: 131, None),
    "D-4/3": (FS48, 4, 3, None, 3000, None, lambda cu: 131, None),
    "D-1/2": (FS48, 1, 2, None, 3000, None, lambda cu: 131, None),
    "D-8/7": (FS48, 8, 7, None, 3000, None, lambda cu: 131, None),
    "D-2/1-wide": (FS48, 2, 1, None, 96, 64, lambda cu: B_Y, None),
}
CHAIN_RUNS = ([(c, p) for c in ("A1", "A2", "A3") for p in (0, 1)]
              + [(c, 0) for c in ("B1-5/4", "B1-2/3", "B2")]
              + [("C", p) for p in (3, 2, 0, 1)]
              + [(c, 0) for c in CHAIN_CASES if c.startswith("D-")])


def _chain_cfg(name):
    from dspcore.chain import ChainConfig
    from dspcore.design import src_plan
    fs, L, M, K, n_in, n_fft, _, _ = CHAIN_CASES[name]
    plan = src_plan(n_in, fs, M, L, K)
    n_fft = _nfft_for(plan.n_out) if n_fft is None else n_fft
    return ChainConfig(n_in, fs, L, M, K, _gains(), n_fft=n_fft), plan


_CHAIN_INPUT = {}


def _chain_input(name, tile_len):
    """Base rows and the oracle's (y, z, |X|) of a chain case, once."""
    if name not in _CHAIN_INPUT:
        from oracle import dsp_ref_cpu as orc
        cfg, plan = _chain_cfg(name)
        x, placed = _base_rows(cfg.n_in, 1000 + len(_CHAIN_INPUT),
                               _bad_specs(plan, cfg.n_in, WAVE * tile_len, tile_len))

        def one(row):
            y, z, _, mag, _ = orc.chain(row, cfg.fs, cfg.L, cfg.M, cfg.gains, cfg.num_taps,
                                        cfg.n_fft)
            return y, z, mag
        _CHAIN_INPUT[name] = (x, placed, _oracle(("chain", name), one, x))
    return _CHAIN_INPUT[name]


def _last_tile_states(ch):
    """Published end state of every channel's last tile (csrc/chain_plan.hip
    tile_ws(): 256-byte header, then [B][ntiles][12] float64)."""
    ntiles = _ceil(ch.n_out, WAVE * ch.tile_len)
    st = ch.workspace[256:256 + ch.B * ntiles * 96].view(torch.float64).reshape(ch.B, ntiles, 12)
    return st[:, -1].cpu().numpy()


def _shape_conditions(name, path, ch, B, names, xb):
    """What the case's shape is there for (the issue's conditions)."""
    from dspcore import _lib
    from dspcore.chain import Chain
    _, L, M, _, n_in, _, _, _ = CHAIN_CASES[name]
    cfg = ch.cfg
    lib = _lib.load()
    S = ch.sos.shape[0]
    ntiles = _ceil(ch.n_out, WAVE * ch.tile_len)
    if path == 1:
        assert "src_poly" in names and "chain_tile" not in names, names
        if B > GRID_Y:
            assert names.count("src_poly") == _ceil(B, GRID_Y) == 2, names
        return
    assert "chain_tile" in names and "chain_repair" in names and "src_poly" not in names, names
    if path == 0:     # every wide case here runs the chained (or persistent) tiles
        assert lib.dsp_chain_mode(B, n_in, ch.n_out, ch.src.K, L, M, ch.src.c_offset, S) == 1
        assert "chain_tile_agg" not in names, names
    if name.startswith("A"):
        assert ch.n_out % 4 == 0
        tail_subs = _ceil(ch.n_out - (ntiles - 1) * WAVE * 48, 48)
        want_pair = {"A1": True, "A2": False, "A3": True}[name]
        assert (tail_subs <= WAVE // 2) == want_pair, (ch.n_out, tail_subs)
        assert ntiles == {"A1": 2, "A2": 2, "A3": 1}[name]
        assert _ceil(B, WAVE) >= 3 and B % 2 == 1      # three repair waves, a lone last half
        if name == "A3":
            assert _ceil(B, WAVE) > REPAIR_GROUPS       # the repair's second sweep
            assert any(b % R in BAD_AT for b in range(REPAIR_GROUPS * WAVE, B))
        # the paired tile publishes its half's end state after 32 sub-chunks,
        # the unpaired after 64 (tests/test_gpu_tail_pair.py): channel 0's last
        # published state differs from its B = 1 run's exactly when paired
        if path == 0:
            wide_state = _last_tile_states(ch)[0]
            one = Chain(cfg, 1, ch.device)
            with _chain_path(2):
                one.run(xb[0:1].contiguous())
            torch.cuda.synchronize()
            paired = not np.array_equal(_last_tile_states(one)[0], wide_state)
            assert paired == want_pair, (name, paired)
    elif name.startswith("B"):
        groups = _ceil(B, 4)
        assert B % 4 == 1 and _ceil(B, 4 * WAVE) >= 2   # one live wave last, a second repair group
        if name == "B2":
            assert _ceil(B, 4 * WAVE) > REPAIR_GROUPS
            assert any(b % R in BAD_AT for b in range(REPAIR_GROUPS * 4 * WAVE, B))
        assert groups * ntiles < 2 ** 31
    elif name == "C":
        groups = _ceil(B, 4)
        # at most 3 waves per SIMD and four-wave groups: <= 3 * CUs resident
        # groups, so the persistent grid walks three rounds at least, the last
        # one partial, and the last group holds one live channel
        assert groups > 2 * 3 * _cus() and B % 4 == 1 and ntiles == 3
        assert _ceil(B, 4 * WAVE) >= 20                 # the repair follows across many groups


_BASE_RUN = {}


@pytest.mark.parametrize("name,path", CHAIN_RUNS, ids=[f"{c}-path{p}" for c, p in CHAIN_RUNS])
def test_chain_wide_batch_rows_are_the_base_rows(gpu, name, path):
    """Families A-D through Chain.run: the 61 base rows (planned for the wide
    batch) against the float64 oracle, then every row of the wide batch
    bitwise its base row, on the default path and the forced ones."""
    from dspcore.chain import Chain
    t0 = time.perf_counter()
    batch, tile_len = CHAIN_CASES[name][6:]
    B = batch(_cus())
    cfg, _ = _chain_cfg(name)
    probe = Chain(cfg, 1, gpu)
    assert probe.tile_len > 0 and (tile_len is None or probe.tile_len == tile_len), probe.tile_len
    x, placed, ref = _chain_input(name, probe.tile_len)
    del probe
    xb = torch.from_numpy(np.array(x)).to(gpu)

    base = Chain(cfg, R, gpu, plan_batch=B)
    with _chain_path(path):
        (yb, zb, mb), names_b = _trace(lambda: base.run(xb))
    assert base.handoff_ok()
    worst = _check_base(f"{name} path {path}", placed, ref, yb.cpu().numpy(), zb.cpu().numpy(),
                        mb.cpu().numpy())
    for r in SCALED:
        assert float(zb[r].abs().max()) == 1.0, "the scaled rows must reach the clip"
    t1 = time.perf_counter()

    xw = _widen(xb, B)
    wide = Chain(cfg, B, gpu)
    assert wide.chunk_len == base.chunk_len and wide.tile_len == base.tile_len
    with _chain_path(path):
        (yw, zw, mw), names_w = _trace(lambda: wide.run(xw))
    assert wide.handoff_ok()
    assert _collapse(names_w) == _collapse(names_b), (names_w, names_b)
    _shape_conditions(name, path, wide, B, names_w, xb)
    _assert_rows_periodic(yw, yb, f"{name} path {path} y")
    _assert_rows_periodic(zw, zb, f"{name} path {path} z")
    _assert_rows_periodic(mw, mb, f"{name} path {path} |X|")
    if name == "C":
        # all four paths give the same base rows: the persistent kernel is
        # bitwise the chained one, y bitwise the SRC kernel's on every path
        keep = _BASE_RUN.setdefault("C", {})
        keep[path] = tuple(t.cpu().numpy() for t in (yb, zb, mb))
        if 2 in keep and 3 in keep:
            for a, b in zip(keep[2], keep[3]):
                np.testing.assert_array_equal(a, b)
        if 1 in keep and 2 in keep:
            fin = np.isfinite(keep[1][0])
            np.testing.assert_array_equal(keep[1][0][fin], keep[2][0][fin])
    print(f"{name} path {path} B={B}: base rows y {worst[0]:.3g} (tol {SRC_ATOL:g} "
          f"max(1,|y|)), z {worst[1]:.3g} (tol {EQ_ATOL:g}), |X| {worst[2]:.3g} (tol {MAG_RTOL:g} "
          f"max|X|); base {t1 - t0:.2f} s, wide {time.perf_counter() - t1:.2f} s")
    del yw, zw, mw, xw, wide, base
    _free()


# --------------------------------------------------------------------------- D: the EQ alone
def test_eq_single_pass_wide_batch(gpu):
    """L = M = 1 through ops.eq_single_pass (the cascade alone as the one-tap
    single-pass kernel): n = 3072, B = 131."""
    from dspcore import _lib, design, ops
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    n, B, fs = 3072, 131, 72000
    sos = design.eq_plan(fs, _gains()).sos
    tsub = int(_lib.load().dsp_chain_tile_len(n, n, 1, 1, 1, 0, sos.shape[0]))
    assert tsub > 0
    ident = design.SrcPlan(1, 1, 1, np.ones(1), 0, n, n, fs)
    x, placed = _base_rows(n, 77, _bad_specs(ident, n, WAVE * tsub, tsub))
    ref = _oracle(("eq1", n), lambda row: orc.equaliser(row, fs, _gains()), x)
    xb = torch.from_numpy(np.array(x)).to(gpu)
    zb, names_b = _trace(lambda: ops.eq_single_pass(xb, sos, plan_batch=B))
    assert zb is not None and "chain_tile" in names_b, names_b
    worst = _check_base("EQ alone", placed, [(None, rz, None) for rz in ref], z=zb.cpu().numpy())
    zw, names_w = _trace(lambda: ops.eq_single_pass(_widen(xb, B), sos))
    assert zw is not None and _collapse(names_w) == _collapse(names_b), (names_w, names_b)
    _assert_rows_periodic(zw, zb, "EQ alone z")
    print(f"EQ alone B={B}: base rows z {worst[1]:.3g} (tol {EQ_ATOL:g}); "
          f"{time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- E: two-launch cascade
# chunk_len -> waves per channel of k_iir_wave (csrc/iir.hip run_fused: one wave up to
# 64 chunks, two up to 128, four up to 256); 4200 samples, since 600 samples are
# at most 19 chunks of the 32-sample granule and could only ever take one wave
E1_N = 4200
E1_CHUNKS = {128: 1, 64: 2, 32: 4}


@pytest.mark.parametrize("chunk_len", sorted(E1_CHUNKS))
def test_cascade_wave_variants_wide_batch(gpu, chunk_len):
    """E1: ops.biquad_cascade with the config-3 cascade, the one-, two- and
    four-wave k_iir_wave (grid of B), B = 1031, bad rows included."""
    from dspcore import design, ops
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    n, B, fs = E1_N, 1031, 72000
    C = _ceil(n, chunk_len)
    assert (1 if C <= 64 else 2 if C <= 128 else 4) == E1_CHUNKS[chunk_len] and C <= 256
    sos = design.eq_plan(fs, _gains()).sos
    ident = design.SrcPlan(1, 1, 1, np.ones(1), 0, n, n, fs)
    x, placed = _base_rows(n, 78, _bad_specs(ident, n, 16 * chunk_len, chunk_len))
    ref = _oracle(("eq1", n, chunk_len), lambda row: orc.equaliser(row, fs, _gains()), x)
    xb = torch.from_numpy(np.array(x)).to(gpu)
    zb, names_b = _trace(lambda: ops.biquad_cascade(xb, sos, True, chunk_len=chunk_len))
    assert names_b == ["iir_fused"], names_b
    worst = _check_base(f"E1 chunk {chunk_len}", placed, [(None, rz, None) for rz in ref],
                        z=zb.cpu().numpy())
    zw, names_w = _trace(lambda: ops.biquad_cascade(_widen(xb, B), sos, True, chunk_len=chunk_len))
    assert names_w == names_b, names_w
    _assert_rows_periodic(zw, zb, f"E1 chunk {chunk_len} z")
    print(f"E1 chunk_len {chunk_len} ({E1_CHUNKS[chunk_len]} waves) B={B}: base rows z "
          f"{worst[1]:.3g} (tol {EQ_ATOL:g}); {time.perf_counter() - t0:.2f} s")


def test_cascade_general_path_wide_batch(gpu):
    """E2: a 9-stage cascade (the general path: k_iir_pass lanes = B * C over
    blocks of 256 spanning channels, k_iir_carry blocks of 256 channels),
    chunk_len = 256, n = 600, B = 1031; finite rows."""
    from dspcore import design, ops
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    n, B, fs, chunk_len = 600, 1031, 72000, 256
    gains = {f"b{i}": (-1) ** i * (3 + i) for i in range(9)}
    sos = design.eq_plan(fs, gains).sos
    assert sos.shape[0] == 9
    x, placed = _base_rows(n, 79)
    rows = x.shape[0]
    ref = _oracle(("eq9", n), lambda row: orc.equaliser(row, fs, gains), x)
    xb = torch.from_numpy(np.array(x)).to(gpu)
    zb, names_b = _trace(lambda: ops.biquad_cascade(xb, sos, True, chunk_len=chunk_len))
    assert names_b == ["iir_prep", "iir_state", "iir_carry", "iir_apply"], names_b
    C = _ceil(n, chunk_len)
    assert _ceil(B, 256) > 1 and (B * C) % 256 and 256 % C      # blocks that span channels
    worst = _check_base("E2", placed, [(None, rz, None) for rz in ref], z=zb.cpu().numpy())
    zw, names_w = _trace(lambda: ops.biquad_cascade(_widen(xb, B), sos, True, chunk_len=chunk_len))
    assert names_w == names_b, names_w
    _assert_rows_periodic(zw, zb, "E2 z", rows=rows)
    print(f"E2 S=9 B={B}: base rows z {worst[1]:.3g} (tol {EQ_ATOL:g}); "
          f"{time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- G: SRC alone
# (L, M, K): the four register-blocked instantiations of launch_src_rows
# (L3/M2 T = 41 and 85, L2/M1 T = 64 and 41) and the generic kernel
SRC_CASES = [(3, 2, 121), (3, 2, 255), (2, 1, 127), (2, 1, 81), (7, 5, 289)]


@pytest.mark.parametrize("L,M,K", SRC_CASES, ids=[f"{l}-{m}-K{k}" for l, m, k in SRC_CASES])
def test_src_second_grid_part_rows_are_the_base_rows(gpu, L, M, K):
    """ops.src_polyphase past 65535 rows (the grid's y extent): the second
    launch's rows are their base rows too; base rows against orc.resample."""
    from dspcore import design, ops
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    n, B = 96, B_Y
    plan = design.src_plan(n, FS48, M, L, K)
    assert plan.K == K and -(-K // L) == {121: 41, 255: 85, 127: 64, 81: 41, 289: 42}[K]
    x, placed = _base_rows(n, 80 + K)
    rows = x.shape[0]
    ref = _oracle(("src", L, M, K), lambda row: orc.resample(row, FS48, M, L, K)[0], x)
    xb = torch.from_numpy(np.array(x)).to(gpu)
    yb, names_b = _trace(lambda: ops.src_polyphase(xb, plan))
    assert names_b == ["src_poly"], names_b
    worst = _check_base(f"SRC {L}/{M} K={K}", placed, [(ry, None, None) for ry in ref],
                        y=yb.cpu().numpy())
    xw = _widen(xb, B)
    yw, names_w = _trace(lambda: ops.src_polyphase(xw, plan))
    assert names_w == ["src_poly"] * _ceil(B, GRID_Y) and len(names_w) == 2, names_w
    _assert_rows_periodic(yw, yb, f"SRC {L}/{M} K={K} y", rows=rows)
    print(f"G SRC {L}/{M} K={K} B={B}: base rows y {worst[0]:.3g} (tol {SRC_ATOL:g} "
          f"max(1,|y|)); {time.perf_counter() - t0:.2f} s")
    del yw, xw
    _free()


# --------------------------------------------------------------------------- F: spectrum / STFT
# n_fft: (threads of a k_spec_stream workgroup = kSpecTpbx * Plan<log2(n_fft) - 1>::TPT with
# kSpecTpbx = 2 and TPT = (n_fft / 2) / 16 (csrc/fft_spec.hip, csrc/fft_pass.h), hop)
SPEC_CASES = {64: (4, 1), 256: (16, 4), 2048: (128, 8), 16384: (1024, 64)}
NF_GROUP = 256           # transforms per k_nf_small workgroup (csrc/fft_nf.hip kNfThreads)


def _frames_for(n_fft):
    """Frames of one channel so that ceil(frames / 2) units exceed twice the
    largest possible residency (32 wave slots per CU), plus 3: a second loop
    iteration in every workgroup and a last unit of one transform."""
    threads, _ = SPEC_CASES[n_fft]
    assert threads == 2 * max(1, (n_fft // 2) // 16)
    res_max = _cus() * 32 // _ceil(threads, WAVE)
    frames = 2 * (2 * res_max) + 3
    assert _ceil(frames, 2) > 2 * res_max and frames % 2 == 1
    return frames


@pytest.mark.parametrize("n_fft", sorted(SPEC_CASES))
def test_stft_past_one_round_of_resident_workgroups(gpu, n_fft):
    """ops.stft_magnitude with more units than two rounds of the persistent
    grid: EVERY frame against numpy's float64 rfft of the Hann-windowed frame
    (1e-5 max|X| per frame); then one NaN in the middle: every frame that
    covers it all NaN (across two k_nf_small workgroups), every other frame
    bitwise the finite run's."""
    from numpy.lib.stride_tricks import sliding_window_view
    from dspcore import design, ops
    t0 = time.perf_counter()
    _, hop = SPEC_CASES[n_fft]
    frames = _frames_for(n_fft)
    n = n_fft + hop * (frames - 1)
    assert n < 400_000
    half = n_fft // 2 + 1
    x = np.random.default_rng(n_fft).uniform(-1, 1, n).astype(np.float32)
    xd = torch.from_numpy(x[None, :]).to(gpu)
    mag, names = _trace(lambda: ops.stft_magnitude(xd, n_fft, hop, frames))
    assert "stft" in names, names
    got = mag[0].cpu().numpy()
    assert got.shape == (frames, half)
    win = design.hann(n_fft)
    view = sliding_window_view(x.astype(np.float64), n_fft)[::hop]
    assert view.shape[0] == frames
    worst = 0.0
    block = max(1, (256 << 20) // (16 * n_fft))         # host temporaries under ~600 MB
    for f0 in range(0, frames, block):
        ref = np.abs(np.fft.rfft(view[f0:f0 + block] * win, axis=1))
        err = np.max(np.abs(got[f0:f0 + block] - ref), axis=1) / np.max(ref, axis=1)
        worst = max(worst, float(err.max()))
        bad = np.nonzero(err > MAG_RTOL)[0]
        assert bad.size == 0, (f"n_fft {n_fft}: {bad.size} frames of {f0}.. beyond 1e-5 max|X|, "
                               f"first {f0 + int(bad[0])} ({err[bad[0]]:.3g})")
    t1 = time.perf_counter()
    # one NaN whose frames straddle a multiple of 256 transforms
    f_edge = (frames // 2) // NF_GROUP * NF_GROUP
    pos = f_edge * hop + n_fft // 2
    xn = xd.clone()
    xn[0, pos] = NAN
    mag_n = ops.stft_magnitude(xn, n_fft, hop, frames)[0]
    f = np.arange(frames)
    covers = (f * hop <= pos) & (pos < f * hop + n_fft)
    assert len(set(f[covers] // NF_GROUP)) >= 2 and covers.sum() == n_fft // hop
    cov = torch.from_numpy(covers).to(gpu)
    assert bool(torch.isnan(mag_n[cov]).all()), "a frame that covers the NaN is not all NaN"
    assert torch.equal(mag_n[~cov].view(torch.int32), mag[0][~cov].view(torch.int32)), \
        "a frame that does not cover the NaN changed"
    print(f"F n_fft {n_fft} hop {hop} frames {frames}: worst frame |X| {worst:.3g} (tol "
          f"{MAG_RTOL:g} max|X|); finite {t1 - t0:.2f} s, NaN pass {time.perf_counter() - t1:.2f} s")
    del mag, mag_n, xn
    _free()


def test_fft_16_points_777_rows(gpu):
    """ops.fft on 777 rows of 16 points (four k_nf_small workgroups, the last
    one of 9 rows) with inf / NaN in rows 300, 511 and 776: their masks are
    orc.fft_dit's, the finite rows bitwise the same rows in batches of 8."""
    from dspcore import ops
    t0 = time.perf_counter()
    B, N = 777, 16
    x = np.random.default_rng(16).uniform(-1, 1, (B, N)).astype(np.float32)
    bad = {300: [(0, INF)], 511: [(7, NAN), (8, -INF)], 776: [(15, -INF)]}
    for r, sp in bad.items():
        for pos, val in sp:
            x[r, pos] = val
    # a group's first rows, a group's last row, the batch's last row in a partial group
    assert {r // NF_GROUP for r in bad} == {1, 3} and 511 % NF_GROUP == NF_GROUP - 1
    assert _ceil(B, NF_GROUP) == 4 and B % NF_GROUP
    xd = torch.from_numpy(x).to(gpu)
    X = ops.fft(xd)
    Xh = X.cpu().numpy()
    with _quiet():
        for r in bad:
            _same_complex(Xh[r], np.asarray(orc_fft(x[r]), dtype=np.complex128), f"row {r}")
    fin = np.ones(B, dtype=bool)
    fin[list(bad)] = False
    assert np.isfinite(Xh[fin].view(np.float32)).all()
    small = torch.cat([ops.fft(xd[b0:b0 + 8].contiguous()) for b0 in range(0, B, 8)])
    keep = torch.from_numpy(fin).to(gpu)
    assert torch.equal(torch.view_as_real(X[keep]).view(torch.int32),
                       torch.view_as_real(small[keep]).view(torch.int32))
    ref = np.fft.fft(x[fin].astype(np.float64), axis=1)
    err = float(np.max(np.abs(Xh[fin] - ref)) / np.max(np.abs(ref)))
    assert err <= MAG_RTOL
    print(f"F fft 16 x {B}: finite rows {err:.3g} (tol {MAG_RTOL:g} max|X|); "
          f"{time.perf_counter() - t0:.2f} s")
