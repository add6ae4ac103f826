"""The streaming kernels (csrc/iir_stream.hip, dspcore/stream.py) at their
chunk, stage, history and batch edges -- what tests/test_gpu_stream.py, with
B = 3 and blocks of 1..5000 samples, never executes.

1. k_iir_stream<S, NORM> for every S = 1..8 (7 runs as 8) with NORM and with a
   b0 == 0 stage, over consecutive blocks whose lengths realise every chunk
   geometry edge: T = 32 ceil(n / 2048), C = ceil(n / T), cap = n - (C - 1) T
   with C = 1, 2, 63, 64 (lane 63 live), the step 2048 -> 2049 (T 32 -> 64),
   cap = T > 32, cap = 1; every block once through views of the row (mostly
   unaligned: guarded scalar loads and stores) and once through 16-byte
   aligned staging (float4), bitwise the same.  Then blocks of 131 072,
   131 073 and 70 001 samples (T = 2048, 2080, 1120: 64, 65 and 35 tiles per
   lane), and x / out at different alignments (vec_x != vec_y) with the bytes
   around `out` guarded by a sentinel.
2. k_stream_roll at hist = 1 .. 4096 (all 16 register slots), n_block below,
   at and above hist, bitwise against a clone, every other column untouched.
3. StreamChain at hist = 0 (K <= L: flush() has a branch of its own), 1, 1536
   and 4096 against the one-shot SRC (bitwise), the two-launch chain and the
   oracle.
4. Streams shorter than the filter (N L < K), an empty flush, an empty push.
5. inf / NaN through the StreamChain: in the SRC history, across the roll.
6. Wide batches (65 537 channels; the SRC's second 65 535-row launch through
   the staging pitch), every row bitwise its base row (the method of
   tests/test_gpu_wide_batch.py), and a non-default stream.

Bounds are tests/test_gpu_stream.py's: Z_ULP2 against the one-shot cascade,
EQ_ATOL / SRC_ATOL against the float64 oracle, CROSS_PATH against the
two-launch chain, and the exit state within 1e-9 of the largest state
component of a float64 model of design.state_space's recursion.  The model
here is that recursion vectorised (_state_trace: per stage w = lfilter([1],
[1, a1, a2], u), delay lines w[n - 1], w[n - 2], stage output g w + c1 w[-1]
+ c2 w[-2] with design.df2_realization's g, c, G); it is checked against the
per-sample loop _state_model on a short row (they agree to 3e-12), and on
the 332 146-sample rows of the long-block test it deviates from the same
recursion in np.longdouble by at most 7.6e-13 of the largest state component
(S = 6; 6.9e-13 with the b0 == 0 cascade, host measurement), so float64
rounding of the model is three orders below the bound and the 1e-9 stands for
the long rows as well.

Every case asserts the condition its shape is there for (T, C, cap, the vec
flags, hist, trace names and launch counts) and prints its wall time and worst
errors."""
import time

import numpy as np
import pytest
import torch

from test_gpu_stream import (CROSS_PATH, EQ_ATOL, FORBIDDEN, FS_EQ, FS_IN, PARTS, SRC_ATOL, Z_ULP2,
                             _gains, _state_model)
from test_gpu_wide_batch import R, _assert_rows_periodic, _free, _widen

pytestmark = pytest.mark.gpu

STATE_RTOL = 1e-9
NAN, INF = float("nan"), float("inf")
GRID_Y = 65535            # csrc/src_poly.hip kMaxGridY
B_WIDE = GRID_Y + 2       # 65537: past one SRC launch, an odd batch
MAX_HIST = 4096           # include/dspcore_stream.h DSP_STREAM_MAX_HIST
ROLL_NT = 256             # csrc/iir_stream.hip kRollNT


def _ceil(a, b):
    return -(-a // b)


def _chunks(n):
    """(T, C, cap) of a block of n samples (csrc/iir_stream.hip run_stream)."""
    T = 32 * _ceil(n, 2048)
    C = _ceil(n, T)
    return T, C, n - (C - 1) * T


def _vec(t):
    """The kernels' float4 condition for the rows of a [B, n] view."""
    return int(t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0)


def _traced(fn):
    """(fn(), trace names of the library's launches)."""
    from dspcore import _lib
    _lib.trace_enable(True)
    _lib.trace_read()
    try:
        out = fn()
        names = [k for k, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    return out, names


def _bits(t):
    """float32 / float64 array or tensor as integers: NaNs and signs count."""
    if isinstance(t, torch.Tensor):
        return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    a = np.ascontiguousarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _assert_states_periodic(wide, base, what):
    """Every row b of the float64 states `wide` is bit for bit row b % R of
    `base` (an all-NaN state is the kernel's own NaN in both)."""
    assert base.shape[0] == R and wide.shape[1:] == base.shape[1:], (what, wide.shape, base.shape)
    want = _bits(base)[torch.arange(wide.shape[0], device=wide.device) % R]
    same = (_bits(wide) == want).all(dim=1)
    bad = (~same).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} rows differ from their base rows: "
                              f"{bad[:12].tolist()}")


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return bool(torch.equal(a, b)) if isinstance(a, torch.Tensor) else bool(np.array_equal(a, b))


# --------------------------------------------------------------------------- 1: the cascade
# block lengths and the (T, C, cap) each realises
GEOMETRY = [(1, (32, 1, 1)), (32, (32, 1, 32)), (33, (32, 2, 1)), (2016, (32, 63, 32)),
            (2017, (32, 64, 1)), (2047, (32, 64, 31)), (2048, (32, 64, 32)), (2049, (64, 33, 1)),
            (4096, (64, 64, 64)), (4097, (96, 43, 65)), (31, (32, 1, 31)), (1, (32, 1, 1))]
BLOCKS = [n for n, _ in GEOMETRY]
LONG_GEOMETRY = [(131072, (2048, 64, 2048)), (131073, (2080, 64, 33)), (70001, (1120, 63, 561))]
B0_STAGE = [0.0, 0.7, 0.2, -0.5, 0.25]


def _cascade(S, norm):
    """S stages of design.eq_plan(72000, .) from subsets / supersets of
    CONFIG3_GAINS; norm=False: the last one replaced by a b0 == 0 stage."""
    from dspcore import design
    g = dict(_gains())
    if S == 1:
        g = {"Bass": -4}
    elif S < 6:
        g = dict(list(g.items())[:S])
    if S >= 7:
        g["Air"] = 2.5
    if S == 8:
        g["Body"] = -1.5
    sos = np.ascontiguousarray(design.eq_plan(FS_EQ, g).sos)
    assert sos.shape == (S, 5) and bool(np.all(sos[:, 0] != 0))
    if not norm:
        sos = sos.copy()
        sos[-1] = B0_STAGE
    assert design.df2_realization(sos)[2] == norm
    return sos


def _state_trace(sos, x, ends):
    """design.state_space's recursion over the rows of x in float64,
    vectorised: the states [len(ends), B, 2S] after ends[i] samples and the
    unclipped output."""
    from scipy.signal import lfilter
    from dspcore import design
    rows, gain, norm = design.df2_realization(sos)
    S = rows.shape[0]
    ends = np.asarray(ends)
    u = x.astype(np.float64) * (gain if norm else 1.0)
    st = np.zeros((ends.size, x.shape[0], 2 * S))
    for k in range(S):
        g, c1, c2, a1, a2 = rows[k]
        w = lfilter([1.0], [1.0, a1, a2], u, axis=1)
        wp = np.concatenate([np.zeros((x.shape[0], 2)), w], axis=1)    # wp[:, i + 2] = w[:, i]
        st[:, :, 2 * k] = wp[:, ends + 1].T
        st[:, :, 2 * k + 1] = wp[:, ends].T
        u = g * w + c1 * wp[:, 1:-1] + c2 * wp[:, :-2]
    return st, u


def _sosfilt_clip(sos, x):
    from scipy.signal import sosfilt
    sos6 = np.column_stack([sos[:, :3], np.ones(sos.shape[0]), sos[:, 3:]])
    return np.clip(sosfilt(sos6, x.astype(np.float64), axis=1), -1.0, 1.0)


def _state_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def test_state_trace_is_the_state_model():
    """The vectorised model against tests/test_gpu_stream.py's per-sample loop."""
    x = np.random.default_rng(20).uniform(-1, 1, (3, 700)).astype(np.float32)
    x[1] *= 8
    worst = 0.0
    for S in range(1, 9):
        for norm in (True, False):
            sos = _cascade(S, norm)
            st, _ = _state_trace(sos, x, [1, 33, 700])
            for i, n in enumerate((1, 33, 700)):
                worst = max(worst, _state_err(st[i], _state_model(sos, x[:, :n])))
    print(f"vectorised state model vs the per-sample loop: {worst:.3g}")
    assert worst <= 1e-11


_ROWS = {}


def _rows(n, seed, B=3):
    key = (n, seed, B)
    if key not in _ROWS:
        x = np.random.default_rng(seed).uniform(-1, 1, (B, n)).astype(np.float32)
        x[1] *= 8
        x.setflags(write=False)
        _ROWS[key] = x
    return _ROWS[key]


def _run_blocks(xd, zd, sos, lengths, staged=None):
    """xd's rows through the cascade in consecutive blocks, the state threaded
    in place (zi is zf); returns the state after every block [blocks, B, 2S].
    staged=(xs, os): every block is copied to the front of the 16-byte aligned
    rows of xs, filtered into os and copied to zd (float4 loads and stores);
    otherwise views of xd and zd at the block's own column."""
    from dspcore import ops
    B = xd.shape[0]
    state = torch.zeros((B, 2 * sos.shape[0]), dtype=torch.float64, device=xd.device)
    states, at = [], 0
    for n in lengths:
        if staged is None:
            xin, out = xd[:, at:at + n], zd[:, at:at + n]
        else:
            xin, out = staged[0][:, :n], staged[1][:, :n]
            xin.copy_(xd[:, at:at + n])
            assert _vec(xin) == 1 and _vec(out) == 1
        (_, zf), names = _traced(lambda: ops.biquad_cascade_state(xin, sos, True, zi=state, out=out,
                                                                  zf=state))
        assert zf is state and names == ["iir_stream"], names
        if staged is not None:
            zd[:, at:at + n].copy_(out)
        states.append(state.clone())
        at += n
    assert at == xd.shape[1]
    return torch.stack(states)


def _check_cascade(label, x, xd, zd, states, sos, lengths, one):
    """z against the one-shot cascade and float64 sosfilt + clip, the state
    after every block against the float64 model."""
    z = zd.cpu().numpy()
    err = float(np.max(np.abs(z - one)))
    eo = float(np.max(np.abs(z - _sosfilt_clip(sos, x))))
    want, _ = _state_trace(sos, x, np.cumsum(lengths))
    got = states.cpu().numpy()
    assert got.shape == want.shape
    es = [_state_err(g, w) for g, w in zip(got, want)]
    print(f"{label}: z vs one-shot {err:.3g} (tol {Z_ULP2:g}), vs sosfilt {eo:.3g} (tol "
          f"{EQ_ATOL:g}), state after each block {max(es):.3g} (tol {STATE_RTOL:g})")
    assert err <= Z_ULP2
    assert eo <= EQ_ATOL
    for n, e in zip(lengths, es):
        assert e <= STATE_RTOL, (label, n, e)
    # row 1 (x8) clips hard, and its state is the unclipped recursion's
    assert float(np.max(np.abs(one[1]))) == 1.0 and float(np.max(np.abs(want[-1][1]))) > 1.0


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "b0"])
@pytest.mark.parametrize("S", range(1, 9))
def test_cascade_every_instantiation_at_every_chunk_edge(gpu, S, norm):
    from dspcore import ops
    t0 = time.perf_counter()
    for n, geo in GEOMETRY:
        assert _chunks(n) == geo, (n, _chunks(n), geo)
    assert {c for _, (_, c, _) in GEOMETRY} >= {1, 2, 63, 64}
    sos = _cascade(S, norm)
    x = _rows(sum(BLOCKS), 31)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    one = ops.biquad_cascade(xd, sos, True).cpu().numpy()
    zd = torch.empty_like(xd)
    states = _run_blocks(xd, zd, sos, BLOCKS)
    _check_cascade(f"S={S} {'NORM' if norm else 'b0'}", x, xd, zd, states, sos, BLOCKS, one)
    # the same blocks through aligned staging rows: float4 loads and stores
    pitch = 4100
    xs = torch.zeros((3, pitch), dtype=torch.float32, device=gpu)
    os_ = torch.zeros((3, pitch), dtype=torch.float32, device=gpu)
    z2 = torch.empty_like(xd)
    states2 = _run_blocks(xd, z2, sos, BLOCKS, staged=(xs, os_))
    assert _same_bits(z2, zd) and _same_bits(states2, states)
    print(f"S={S} {'NORM' if norm else 'b0'}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("S,norm", [(6, True), (3, False)], ids=["S6-norm", "S3-b0"])
def test_cascade_long_blocks(gpu, S, norm):
    """Blocks past 131 072 samples: T > 2048, 65 tiles per lane."""
    from dspcore import ops
    t0 = time.perf_counter()
    lengths = [n for n, _ in LONG_GEOMETRY]
    for n, geo in LONG_GEOMETRY:
        assert _chunks(n) == geo, (n, _chunks(n), geo)
    assert [g[0] // 32 for _, g in LONG_GEOMETRY] == [64, 65, 35]
    n = sum(lengths)
    sos = _cascade(S, norm)
    x = _rows(n, 32, B=2)
    ld = _ceil(n, 4) * 4
    xb = torch.zeros((2, ld), dtype=torch.float32, device=gpu)
    zb = torch.zeros((2, ld), dtype=torch.float32, device=gpu)
    xd, zd = xb[:, :n], zb[:, :n]
    xd.copy_(torch.from_numpy(np.array(x)))
    # blocks 1 and 2 start 16-byte aligned (float4), block 3 does not
    starts = np.cumsum([0] + lengths[:-1])
    assert [_vec(xd[:, a:a + 1]) for a in starts] == [1, 1, 0]
    one = ops.biquad_cascade(xd, sos, True).cpu().numpy()
    states = _run_blocks(xd, zd, sos, lengths)
    _check_cascade(f"long S={S}", x, xd, zd, states, sos, lengths, one)
    print(f"long S={S}: {time.perf_counter() - t0:.2f} s")


MIXED_BLOCKS = [33, 2050, 4099, 131, 1]
# name: (x column, out column, x pitch pad, out pitch pad) -> (vec_x, vec_y)
MIXED = {"x4-y1": ((4, 1, 0, 0), (1, 0)), "x1-y4": ((1, 4, 0, 0), (0, 1)),
         "x1-y1": ((1, 1, 0, 0), (0, 0)), "xpitch-y4": ((0, 4, 3, 0), (0, 1)),
         "x4-ypitch": ((4, 0, 0, 1), (1, 0))}
SENTINEL = 12345.0


def _run_mixed(gpu, xd, sos, cfg, want_vec):
    from dspcore import ops
    xo, yo, xpad, ypad = cfg
    pitch = 4112
    assert all(n % 4 for n in MIXED_BLOCKS)
    assert max(xo, yo) + _ceil(max(MIXED_BLOCKS), 4) * 4 <= pitch
    xs = torch.zeros((2, pitch + xpad), dtype=torch.float32, device=gpu)
    os_ = torch.empty((2, pitch + ypad), dtype=torch.float32, device=gpu)
    state = torch.zeros((2, 2 * sos.shape[0]), dtype=torch.float64, device=gpu)
    zd = torch.empty_like(xd)
    states, at = [], 0
    for n in MIXED_BLOCKS:
        xin, out = xs[:, xo:xo + n], os_[:, yo:yo + n]
        assert (_vec(xin), _vec(out)) == want_vec
        xin.copy_(xd[:, at:at + n])
        os_.fill_(SENTINEL)
        _, names = _traced(lambda: ops.biquad_cascade_state(xin, sos, True, zi=state, out=out,
                                                            zf=state))
        assert names == ["iir_stream"], names
        # nothing outside the block's columns is written, at either end of a row
        assert bool((os_[:, :yo] == SENTINEL).all()) and bool((os_[:, yo + n:] == SENTINEL).all())
        assert bool((out != SENTINEL).all())
        zd[:, at:at + n].copy_(out)
        states.append(state.clone())
        at += n
    return zd, torch.stack(states)


@pytest.mark.parametrize("S,norm", [(6, True), (3, False)], ids=["S6-norm", "S3-b0"])
def test_cascade_mixed_alignment(gpu, S, norm):
    """vec_x != vec_y, by the pointer and by the pitch: bitwise the run with
    both aligned; the float4 stores stay inside the block's columns."""
    from dspcore import ops
    t0 = time.perf_counter()
    assert {_chunks(n)[1] > 1 for n in MIXED_BLOCKS} == {True, False}
    sos = _cascade(S, norm)
    x = _rows(sum(MIXED_BLOCKS), 33, B=2)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    one = ops.biquad_cascade(xd, sos, True).cpu().numpy()
    z0, st0 = _run_mixed(gpu, xd, sos, (4, 4, 0, 0), (1, 1))
    _check_cascade(f"aligned S={S}", x, xd, z0, st0, sos, MIXED_BLOCKS, one)
    for name, (cfg, want_vec) in MIXED.items():
        z, st = _run_mixed(gpu, xd, sos, cfg, want_vec)
        assert _same_bits(z, z0), name
        assert _same_bits(st, st0), name
    print(f"mixed alignment S={S}: {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 2: the roll
def _roll(buf, hist, n_block):
    from dspcore import _lib
    lib = _lib.load()
    with torch.cuda.device(buf.device):
        rc = lib.dsp_stream_roll_f32(buf.data_ptr(), buf.shape[0], buf.stride(0), hist, n_block,
                                     torch.cuda.current_stream(buf.device).cuda_stream)
    _lib.check(rc, "dsp_stream_roll_f32")


@pytest.mark.parametrize("hist", [1, 255, 256, 257, 1536, 4095, 4096])
def test_roll_bitwise_at_every_history_length(gpu, hist):
    t0 = time.perf_counter()
    assert hist <= MAX_HIST and MAX_HIST == 16 * ROLL_NT
    slots = _ceil(hist, ROLL_NT)          # register slots of a thread that carry data
    assert slots == {1: 1, 255: 1, 256: 1, 257: 2, 1536: 6, 4095: 16, 4096: 16}[hist]
    blocks = sorted({n for n in (1, hist - 1, hist, hist + 1, 3 * hist) if n >= 1})
    gen = torch.Generator(device="cpu").manual_seed(hist)
    runs = 0
    for n_block in blocks:
        for B in (1, 5):
            for pad in (0, 13):
                ld = hist + n_block + pad
                buf = torch.rand((B, ld), generator=gen, dtype=torch.float32).to(gpu)
                want = buf.clone()
                want[:, :hist] = buf[:, n_block:n_block + hist].clone()
                _, names = _traced(lambda: _roll(buf, hist, n_block))
                assert names == ["stream_roll"], names
                # the history moved, every other column as it was
                assert _same_bits(buf, want), (hist, n_block, B, ld)
                runs += 1
    print(f"roll hist={hist}: {runs} calls, n_block {blocks}; {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 3-5: StreamChain
N_LONG = 12000
HIST_CASES = {(8, 3, 7): 0, (8, 5, 5): 0, (8, 1, 9): 1, (1, 2, 4097): 4096, (1, 3, 1537): 1536}
FLUSH_OUT = {(8, 3, 7): 1, (8, 5, 5): 0, (8, 1, 9): 4, (1, 2, 4097): 1024, (1, 3, 1537): 256}
LONG_PARTS = {"blocks": [1, 100, 4096, 3000, 4803], "ones": [1] * 50 + [N_LONG - 50]}
_REF = {}


def _signal(n, seed):
    key = ("x", n, seed)
    if key not in _REF:
        x = np.random.default_rng(seed).uniform(-1, 1, (3, n)).astype(np.float32)
        x.setflags(write=False)
        _REF[key] = x
    return _REF[key]


def _one_shot(gpu, key, x, L, M, K, oracle=True):
    """One-shot references of x [3, n], once per key: the SRC kernel's y, the
    two-launch Chain's z (dsp_chain_path(1)), the oracle's y and z."""
    if key not in _REF:
        from dspcore import _lib, design, ops
        from dspcore.chain import Chain, ChainConfig
        from oracle import dsp_ref_cpu as orc
        n = x.shape[1]
        xd = torch.from_numpy(np.array(x)).to(gpu)
        y = ops.src_polyphase(xd, design.src_plan(n, FS_IN, M, L, K)).cpu().numpy()
        prev = _lib.chain_path(1)
        try:
            ch = Chain(ChainConfig(n, FS_IN, L, M, K, _gains(), n_fft=256), 3, gpu)
            z = ch.run(xd)[1].cpu().numpy().copy()
        finally:
            _lib.chain_path(prev)
        oy, oz = [], []
        if oracle:
            with np.errstate(all="ignore"):
                for r in x:
                    ry, fs_out = orc.resample(r.astype(np.float64), FS_IN, M, L, K)
                    oy.append(ry)
                    oz.append(orc.equaliser(ry, fs_out, _gains()))
        _REF[key] = (y, z, np.stack(oy) if oracle else None, np.stack(oz) if oracle else None)
    return _REF[key]


def _drive(sc, xd, parts):
    """Pushes xd through sc in `parts`, then flushes.  Returns (y, z, per-call
    output counts, per-call trace names), the flush last."""
    ys, zs, counts, names = [], [], [], []
    at = 0
    for n in list(parts) + [None]:
        if n is None:
            (y, z), got = _traced(sc.flush)
        else:
            (y, z), got = _traced(lambda: sc.push(xd[:, at:at + n]))
            at += n
        assert z.shape[0] == xd.shape[0] and y.shape == z.shape
        ys.append(y.clone())
        zs.append(z.clone())
        counts.append(z.shape[1])
        names.append(got)
    assert at == xd.shape[1]
    return torch.cat(ys, dim=1), torch.cat(zs, dim=1), counts, names


def _check_counts_and_launches(sc, plan, parts, counts, names, src_launches=1):
    """Per-call counts are the plan's; a call that produces output launches
    the SRC and the stateful cascade once (the SRC once per 65535 rows), a
    push with a history the roll, and never the one-shot cascade's kernels."""
    consumed = produced = 0
    for n, got in zip(parts, counts):
        assert got == plan.block(consumed, produced, n)[2]
        consumed += n
        produced += got
    assert counts[-1] == plan.flush(consumed, produced)[2]
    assert sum(counts) == _ceil(consumed * plan.L, plan.M)
    for n, got, call in zip(list(parts) + [0], counts, names):
        assert not FORBIDDEN & set(call), call
        want = ["src_poly"] * src_launches + ["iir_stream"] if got else []
        if n and plan.hist:
            want = want + ["stream_roll"]
        assert call == want, (n, got, call)


# every ratio in blocks; the sample-by-sample start for hist = 0 and 1
HIST_RUNS = ([(k, "blocks") for k in HIST_CASES]
             + [(k, "ones") for k, h in HIST_CASES.items() if h <= 1])


@pytest.mark.parametrize("ratio,parts", HIST_RUNS,
                         ids=[f"{l}-{m}-K{k}-{p}" for (l, m, k), p in HIST_RUNS])
def test_stream_chain_at_the_history_extremes(gpu, ratio, parts):
    from dspcore import design
    from dspcore.stream import StreamChain
    L, M, K = ratio
    hist = HIST_CASES[ratio]
    t0 = time.perf_counter()
    x = _signal(N_LONG, 41)
    plan = design.stream_src_plan(FS_IN, M, L, K)
    assert plan.K == K and plan.hist == hist and (hist == 0) == (K <= L) and N_LONG * L >= K
    ref_y, ref_z, orc_y, orc_z = _one_shot(gpu, ("long", L, M, K), x, L, M, K)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    part = LONG_PARTS[parts]
    assert sum(part) == N_LONG
    sc = StreamChain(FS_IN, L, M, K, _gains(), 3, max(part), gpu)
    assert sc.hist == hist and sc.latency_in == plan.c / L
    y, z, counts, names = _drive(sc, xd, part)
    total = _ceil(N_LONG * L, M)
    assert y.shape == z.shape == (3, total)
    _check_counts_and_launches(sc, plan, part, counts, names)
    assert counts[-1] == FLUSH_OUT[(L, M, K)]      # hist == 0 with output: flush's own branch
    assert counts[0] == plan.ready(1)
    y, z = y.cpu().numpy(), z.cpu().numpy()
    assert _same_bits(y, ref_y), float(np.max(np.abs(y - ref_y)))
    ez = float(np.max(np.abs(z - ref_z)))
    ey = float(np.max(np.abs(y - orc_y)) / max(1.0, np.max(np.abs(orc_y))))
    eo = float(np.max(np.abs(z - orc_z)))
    print(f"{L}/{M} K={K} hist={hist} {parts}: z vs chain {ez:.3g}, y vs oracle {ey:.3g}, z vs "
          f"oracle {eo:.3g}; {time.perf_counter() - t0:.2f} s")
    assert ez <= CROSS_PATH
    assert ey <= SRC_ATOL
    assert eo <= EQ_ATOL


# (L, M, K, N): N L < K
SHORT = [(3, 2, None, 10), (1, 8, None, 7), (8, 7, None, 1), (160, 147, 1023, 3), (1, 2, 4097, 100)]


@pytest.mark.parametrize("L,M,K,N", SHORT, ids=[f"{l}-{m}-N{n}" for l, m, _, n in SHORT])
def test_streams_shorter_than_the_filter(gpu, L, M, K, N):
    """ceil(N L / M) outputs centred at (K - 1) / 2: the first outputs of the
    oracle's chain on the signal zero-padded by 3 K samples."""
    from dspcore import design
    from dspcore.stream import StreamChain
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    plan = design.stream_src_plan(FS_IN, M, L, K)
    assert N * L < plan.K
    total = _ceil(N * L, M)
    x = _signal(N, 42 + N)
    oy, oz = [], []
    for r in x:
        padded = np.concatenate([r.astype(np.float64), np.zeros(3 * plan.K)])
        ry, fs_out = orc.resample(padded, FS_IN, M, L, K)
        oy.append(ry[:total])
        oz.append(orc.equaliser(ry, fs_out, _gains())[:total])
    oy, oz = np.stack(oy), np.stack(oz)
    xd = torch.from_numpy(np.array(x)).to(gpu)
    got = {}
    for name, part in (("one block", [N]), ("by sample", [1] * N)):
        sc = StreamChain(FS_IN, L, M, K, _gains(), 3, N, gpu)
        y, z, counts, names = _drive(sc, xd, part)
        assert y.shape == z.shape == (3, total) and sum(counts) == total
        _check_counts_and_launches(sc, plan, part, counts, names)
        y, z = y.cpu().numpy(), z.cpu().numpy()
        ey = float(np.max(np.abs(y - oy)) / max(1.0, np.max(np.abs(oy))))
        ez = float(np.max(np.abs(z - oz)))
        print(f"{L}/{M} N={N} {name}: {total} outputs ({counts[-1]} at the flush), y vs oracle "
              f"{ey:.3g}, z vs oracle {ez:.3g}")
        assert ey <= SRC_ATOL
        assert ez <= EQ_ATOL
        got[name] = (y, z)
    # the same kernel sums every output in the same order wherever the cuts fall
    assert _same_bits(got["one block"][0], got["by sample"][0])
    assert float(np.max(np.abs(got["one block"][1] - got["by sample"][1]))) <= Z_ULP2
    print(f"{L}/{M} N={N}: {time.perf_counter() - t0:.2f} s")


def test_empty_flush_and_empty_push(gpu):
    from dspcore.stream import StreamChain
    xd = torch.from_numpy(np.array(_signal(3000, 43))).to(gpu)
    sc = StreamChain(FS_IN, 3, 2, None, _gains(), 3, 1000, gpu)
    (y, z), names = _traced(sc.flush)                  # nothing pushed
    assert y.shape == z.shape == (3, 0) and names == []
    parts = [1000, 500, 1, 999, 500]
    sc.reset()
    y0, z0, counts0, _ = _drive(sc, xd, parts)
    # the same stream with an empty block pushed between every two blocks
    sc.reset()
    ys, zs, at = [], [], 0
    for n in parts:
        (ye, ze), names = _traced(lambda: sc.push(xd[:, at:at]))
        assert ye.shape == ze.shape == (3, 0) and names == [], names
        y, z = sc.push(xd[:, at:at + n])
        ys.append(y.clone())
        zs.append(z.clone())
        at += n
    (ye, ze), names = _traced(lambda: sc.push(xd[:, :0]))
    assert ze.shape == (3, 0) and names == []
    y, z = sc.flush()
    y1, z1 = torch.cat(ys + [y], dim=1), torch.cat(zs + [z], dim=1)
    assert y1.shape[1] == sum(counts0)
    assert _same_bits(y1, y0) and _same_bits(z1, z0)


NF_RATIOS = [(3, 2, None), (160, 147, 1023)]
NF_N = 6000
NF_NAN, NF_PINF, NF_NINF = 2500, 1500, 1501


@pytest.mark.parametrize("L,M,K", NF_RATIOS, ids=["3-2-reg", "160-147-generic"])
def test_nonfinite_input_through_the_chain(gpu, L, M, K):
    """A NaN inside a block (channel 0), a +inf as a block's last sample and a
    -inf as the next block's first (channel 1), a clean channel 2."""
    from dspcore import design
    from dspcore.stream import StreamChain
    t0 = time.perf_counter()
    parts = PARTS["ragged"]
    cuts = list(np.cumsum(parts))
    assert sum(parts) == NF_N and NF_NINF in cuts and NF_PINF + 1 == NF_NINF
    assert not any(c in (NF_NAN, NF_NAN + 1) for c in cuts)       # the NaN inside a block
    plan = design.stream_src_plan(FS_IN, M, L, K)
    # csrc/src_poly.hip launch_src_rows: L3/M2 with 41 taps a phase is register-blocked
    assert ((L, M, _ceil(plan.K, L)) == (3, 2, 41)) == (K is None)
    clean = _signal(NF_N, 44)
    x = np.array(clean)
    x[0, NF_NAN] = NAN
    x[1, NF_PINF] = INF
    x[1, NF_NINF] = -INF
    ref_y, ref_z, orc_y, _ = _one_shot(gpu, ("nf", L, M, K), x, L, M, K)
    sc = StreamChain(FS_IN, L, M, K, _gains(), 3, max(parts), gpu)
    y, z, counts, names = _drive(sc, torch.from_numpy(x).to(gpu), parts)
    _check_counts_and_launches(sc, plan, parts, counts, names)
    eq_state = sc.state_dict()["eq_state"].numpy()
    sc.reset()
    yc, zc, _, _ = _drive(sc, torch.from_numpy(np.array(clean)).to(gpu), parts)
    clean_state = sc.state_dict()["eq_state"].numpy()
    y, z, yc, zc = y.cpu().numpy(), z.cpu().numpy(), yc.cpu().numpy(), zc.cpu().numpy()
    # y: bitwise the one-shot kernel's, NaNs and the signs of inf included
    assert _same_bits(y, ref_y), np.nonzero(_bits(y) != _bits(ref_y))
    for mask in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(mask(y), mask(orc_y)), mask.__name__
    fin = np.isfinite(orc_y)
    ey = float(np.max(np.abs(y[fin] - orc_y[fin])))
    assert ey <= SRC_ATOL * max(1.0, float(np.max(np.abs(orc_y[fin]))))
    # finite again once the sample has left every window: hist inputs later
    m = np.arange(y.shape[1])
    q = (m * M + plan.c) // L                  # the last input output m reads
    for ch, last in ((0, NF_NAN), (1, NF_NINF)):
        bad = ~np.isfinite(y[ch])
        assert bad.any() and not bad[q > last + plan.hist].any() and not bad[q < last - 1].any()
    assert np.isfinite(y[2]).all()
    # z: NaN from the first non-finite y on, in every later block and the flush
    assert np.array_equal(np.isnan(z), np.isnan(ref_z))
    assert not np.isinf(z).any()
    fz = ~np.isnan(ref_z)
    ez = float(np.max(np.abs(z[fz] - ref_z[fz])))
    assert ez <= CROSS_PATH
    ends = np.cumsum(counts)
    for ch in (0, 1):
        first = int(np.nonzero(~np.isfinite(y[ch]))[0][0])
        assert np.isfinite(z[ch, :first]).all() and np.isnan(z[ch, first + 1:]).all()
        assert sum(e > first + 1 for e in ends) >= 3            # later blocks and the flush
    # the clean channel is bitwise the clean stream's; the states follow
    assert _same_bits(y[2], yc[2]) and _same_bits(z[2], zc[2])
    assert np.isnan(eq_state[:2]).all() and np.isfinite(eq_state[2]).all()
    assert _same_bits(eq_state[2], clean_state[2])
    print(f"non-finite {L}/{M}: y vs oracle {ey:.3g}, z vs chain {ez:.3g}; "
          f"{time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 6: wide batches
WIDE_BLOCKS = [96, 33]
# base row: [(column, value)]
WIDE_BAD = {3: [(50, NAN)], 8: [(95, INF), (96, -INF)], 13: [(0, -INF)], 18: [(128, NAN)],
            23: [(40, INF)]}
WIDE_SCALED = (1, 17, 32)


def _wide_rows(n, seed, bad):
    x = np.random.default_rng(seed).uniform(-0.9, 0.9, (R, n)).astype(np.float32)
    for r in WIDE_SCALED:
        x[r] *= 40.0
    for r, spec in bad.items():
        assert r not in WIDE_SCALED
        for col, val in spec:
            x[r, min(col, n - 1)] = val
    x.setflags(write=False)
    return x


def _check_z_rows(label, z, ref, x_or_y, tol):
    """Rows of z against the float64 reference: finite rows within tol; a row
    whose input first turns non-finite at p is finite and within tol before p
    and all NaN after it."""
    worst = 0.0
    for r in range(z.shape[0]):
        bad = np.nonzero(~np.isfinite(x_or_y[r]))[0]
        p = int(bad[0]) if bad.size else z.shape[1]
        assert np.isfinite(z[r, :p]).all(), (label, r)
        assert np.isnan(z[r, p + 1:]).all(), (label, r)
        if p:
            worst = max(worst, float(np.max(np.abs(z[r, :p] - ref[r][:p]))))
    assert worst <= tol, (label, worst)
    return worst


def _two_blocks(xd, sos, clip=True):
    from dspcore import ops
    B, n = xd.shape
    assert n == sum(WIDE_BLOCKS)
    z = torch.empty_like(xd)
    state = torch.zeros((B, max(2 * sos.shape[0], 1)), dtype=torch.float64, device=xd.device)
    at = 0
    for nb in WIDE_BLOCKS:
        _, names = _traced(lambda: ops.biquad_cascade_state(xd[:, at:at + nb], sos, clip, zi=state,
                                                            out=z[:, at:at + nb], zf=state))
        assert names == ["iir_stream"], names
        at += nb
    return z, state


@pytest.mark.parametrize("S", [6, 0])
def test_cascade_state_wide_batch(gpu, S):
    """One workgroup per channel (S = 6) and blockIdx.x / per_row (S = 0, the
    clip kernel) at 65 537 channels over two blocks: every row of z and zf
    bitwise its base row."""
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    n = sum(WIDE_BLOCKS)
    x = _wide_rows(n, 61, WIDE_BAD)
    assert any(c == WIDE_BLOCKS[0] - 1 for c, _ in WIDE_BAD[8])     # an inf across the block cut
    sos = _cascade(6, True) if S else np.zeros((0, 5))
    xb = torch.from_numpy(np.array(x)).to(gpu)
    zb, sb = _two_blocks(xb, sos)
    z = zb.cpu().numpy()
    if S:
        with np.errstate(all="ignore"):
            ref = [orc.equaliser(r.astype(np.float64), FS_EQ, _gains()) for r in x]
        worst = _check_z_rows("cascade base rows", z, ref, x, EQ_ATOL)
        fin = np.array([r not in WIDE_BAD for r in range(R)])
        want, _ = _state_trace(sos, x[fin], [n])
        got = sb.cpu().numpy()
        es = _state_err(got[fin], want[0])
        assert es <= STATE_RTOL and np.isnan(got[~fin]).all()
        for r in WIDE_SCALED:
            assert float(np.max(np.abs(z[r]))) == 1.0
        print(f"wide cascade base rows: z {worst:.3g} (tol {EQ_ATOL:g}), state {es:.3g}")
    else:
        assert all(_ceil(nb, 256) == 1 for nb in WIDE_BLOCKS)
        with np.errstate(all="ignore"):
            want = np.clip(x, -1.0, 1.0)
        assert np.array_equal(np.isnan(z), np.isnan(want))
        assert np.array_equal(z[~np.isnan(want)], want[~np.isnan(want)])
        assert not bool(sb.any())                                    # no state is written
    xw = _widen(xb, B_WIDE)
    zw, sw = _two_blocks(xw, sos)
    _assert_rows_periodic(zw, zb, f"S={S} z")
    _assert_states_periodic(sw, sb, f"S={S} zf")
    print(f"wide cascade S={S} B={B_WIDE}: {time.perf_counter() - t0:.2f} s")
    del xw, zw, sw
    _free()


def test_clip_kernel_two_groups_per_row_wide_batch(gpu):
    """k_stream_clip at n = 300: per_row = 2, a workgroup's row is
    blockIdx.x / 2; 1031 channels, clip on and off."""
    from dspcore import ops
    n, B = 300, 1031
    assert _ceil(n, 256) == 2 and B % 2 == 1
    x = _wide_rows(n, 62, {3: [(255, NAN)], 8: [(256, INF)], 13: [(299, -INF)]})
    xb = torch.from_numpy(np.array(x)).to(gpu)
    xw = _widen(xb, B)
    none = np.zeros((0, 5))
    for clip in (True, False):
        (zb, _), names = _traced(lambda: ops.biquad_cascade_state(xb, none, clip))
        assert names == ["iir_stream"], names
        z = zb.cpu().numpy()
        with np.errstate(all="ignore"):
            want = np.clip(x, -1.0, 1.0) if clip else np.array(x)
        assert np.array_equal(np.isnan(z), np.isnan(want))
        assert np.array_equal(z[~np.isnan(want)], want[~np.isnan(want)])
        assert bool(np.isinf(z).any()) != clip
        zw, _ = ops.biquad_cascade_state(xw, none, clip)
        _assert_rows_periodic(zw, zb, f"clip={clip} z")


@pytest.mark.parametrize("hist", [40, 300])
def test_roll_wide_batch(gpu, hist):
    n_block = 64
    gen = torch.Generator(device="cpu").manual_seed(hist)
    base = torch.rand((R, hist + n_block + 4), generator=gen, dtype=torch.float32).to(gpu)
    wide = _widen(base, B_WIDE)
    want = base.clone()
    want[:, :hist] = base[:, n_block:n_block + hist].clone()
    _roll(base, hist, n_block)
    assert _same_bits(base, want)
    _, names = _traced(lambda: _roll(wide, hist, n_block))
    assert names == ["stream_roll"], names
    _assert_rows_periodic(wide, base, f"roll hist={hist}")
    del wide
    _free()


WIDE_PUSHES = [64, 1, 50]
CHAIN_BAD = {3: [(30, NAN)], 8: [(63, INF), (64, -INF)], 13: [(0, -INF)], 18: [(114, NAN)]}


def _drive_rows(sc, xd, parts):
    """_drive, and the history and EQ state rows the stream ends with."""
    y, z, counts, names = _drive(sc, xd, parts)
    sd = sc.state_dict()
    assert tuple(sd["history"].shape) == (sc.B, sc.hist)
    return y, z, counts, names, sd["history"].to(xd.device), sd["eq_state"].to(xd.device)


def test_stream_chain_wide_batch(gpu):
    """StreamChain at 65 537 channels: the SRC's second launch through the
    staging pitch, one cascade workgroup and one roll workgroup per channel."""
    from dspcore import design
    from dspcore.stream import StreamChain
    from oracle import dsp_ref_cpu as orc
    t0 = time.perf_counter()
    L, M = 3, 2
    n = sum(WIDE_PUSHES)
    plan = design.stream_src_plan(FS_IN, M, L, None)
    assert n * L >= plan.K and max(WIDE_PUSHES) == 64 and _ceil(B_WIDE, GRID_Y) == 2
    x = _wide_rows(n, 63, CHAIN_BAD)
    assert any(c == WIDE_PUSHES[0] - 1 for c, _ in CHAIN_BAD[8])    # an inf across the roll
    xb = torch.from_numpy(np.array(x)).to(gpu)
    base = StreamChain(FS_IN, L, M, None, _gains(), R, 64, gpu)
    yb, zb, counts, names, hb, sb = _drive_rows(base, xb, WIDE_PUSHES)
    _check_counts_and_launches(base, plan, WIDE_PUSHES, counts, names)
    assert all(counts) and sum(counts) == _ceil(n * L, M)
    y, z = yb.cpu().numpy(), zb.cpu().numpy()
    wy = wz = 0.0
    with np.errstate(all="ignore"):
        for r in range(R):
            ry, fs_out = orc.resample(x[r].astype(np.float64), FS_IN, M, L, None)
            for mask in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(mask(y[r]), mask(ry)), (r, mask.__name__)
            fin = np.isfinite(ry)
            scale = max(1.0, float(np.max(np.abs(ry[fin]))))
            wy = max(wy, float(np.max(np.abs(y[r][fin] - ry[fin]))) / scale)
            rz = orc.equaliser(ry, fs_out, _gains())
            wz = max(wz, _check_z_rows(f"row {r}", z[r:r + 1], [rz], y[r:r + 1], EQ_ATOL))
    assert wy <= SRC_ATOL
    state = sb.cpu().numpy()
    for r in range(R):
        assert np.isnan(state[r]).all() == (r in CHAIN_BAD), r
    wide = StreamChain(FS_IN, L, M, None, _gains(), B_WIDE, 64, gpu)
    yw, zw, counts_w, names_w, hw, sw = _drive_rows(wide, _widen(xb, B_WIDE), WIDE_PUSHES)
    assert counts_w == counts
    _check_counts_and_launches(wide, plan, WIDE_PUSHES, counts_w, names_w, src_launches=2)
    assert all(call.count("src_poly") == 2 for call in names_w)
    _assert_rows_periodic(yw, yb, "StreamChain y")
    _assert_rows_periodic(zw, zb, "StreamChain z")
    _assert_rows_periodic(hw, hb, "StreamChain history")
    _assert_states_periodic(sw, sb, "StreamChain EQ state")
    print(f"wide StreamChain B={B_WIDE}: base rows y {wy:.3g} (tol {SRC_ATOL:g} max(1,|y|)), z "
          f"{wz:.3g} (tol {EQ_ATOL:g}); {time.perf_counter() - t0:.2f} s")
    del yw, zw, hw, sw, wide
    _free()


def test_stream_chain_on_a_side_stream(gpu):
    """Every launch of a push goes to the current stream: a StreamChain driven
    on a non-default stream is bitwise the default-stream run."""
    from dspcore.stream import StreamChain
    parts = PARTS["ragged"]
    xd = torch.from_numpy(np.array(_signal(sum(parts), 45))).to(gpu)
    sc = StreamChain(FS_IN, 3, 2, None, _gains(), 3, max(parts), gpu)
    y0, z0, counts0, _ = _drive(sc, xd, parts)
    state0 = sc.state_dict()["eq_state"]
    torch.cuda.synchronize()
    sc.reset()
    side = torch.cuda.Stream(device=gpu)
    assert side.cuda_stream != torch.cuda.default_stream(gpu).cuda_stream
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(gpu).cuda_stream == side.cuda_stream
        y1, z1, counts1, _ = _drive(sc, xd, parts)
        state1 = sc.state_dict()["eq_state"]
    side.synchronize()
    torch.cuda.current_stream(gpu).wait_stream(side)
    assert counts1 == counts0
    assert _same_bits(y1, y0) and _same_bits(z1, z0) and _same_bits(state1, state0)
