"""The paired tail tile of the L3/M2 single-pass kernel (csrc/chain_tile.hip,
k_chain_tile_pair): where a row's last tile fills at most half a wave (32 of 64
sub-chunks of 48 outputs), one wave carries the last tiles of two channels,
channel 2c in lanes 0-31 and 2c+1 in lanes 32-63.  No row may change by it:

  * every row of y and z of a batch is bitwise the row of a B = 1 call on that
    channel alone (B = 1 never pairs: the parent's path), whichever half the
    channel rides in and whatever its partner holds -- reversed batches, odd
    batches (the last channel alone in its wave), a partner with an inf or NaN;
  * keep_y=False (y = NULL) gives the same z;
  * the oracle (oracle/dsp_ref_cpu.py; reference dsp_core.py:133-254) within the
    project's SRC and EQ tolerances, a clipped row included;
  * the hand-off flags and the status word read zero after every call, calls
    back to back on one workspace agree, and a captured graph replays bitwise.

Shapes (a tile is 2048 inputs, 3072 outputs; a sub-chunk 32 inputs):
  n_in 2944: two tiles, tail of 28 sub-chunks (config 3/4's)       paired
       3072: tail of exactly 32                                      paired
       3104: tail of 33                                              unpaired
       2948: n_out = 4422 ends inside a sub-chunk, but is no multiple of 4:
             k_chain_tile does not serve it (the rows must agree all the same)
       2952: n_out = 4428 ends inside sub-chunk 29                   paired
        896: one tile, which is the tail; entry state zero           paired
       6304: three full tiles before a 5-lane tail                   paired
Which path ran shows in the workspace: the paired tile publishes its half's
end state after 32 sub-chunks, the unpaired tile after 64 (chain_tile.h,
PairEntry), so the last tile's published state differs from the B = 1 call's
exactly when the tail was paired.

All calls force the chained mode (dsp_chain_path(2)); small batches would
otherwise take the three-launch mode.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SRC_ATOL = 2e-6
EQ_ATOL = 1e-5
FS = 48000
ROWS = 5
# n_in -> whether k_chain_tile_pair serves the tail (None: another kernel's geometry)
SHAPES = {2944: True, 3072: True, 3104: False, 2948: None, 2952: True, 896: True,
          2048 * 3 + 32 * 5: True}
BATCHES = (1, 2, 3, 5)


@contextlib.contextmanager
def _chained():
    from dspcore import _lib
    prev = _lib.chain_path(2)
    try:
        yield
    finally:
        _lib.chain_path(prev)


def _chain(gpu, n_in, B, keep_y=True):
    from dspcore.chain import Chain, ChainConfig
    from oracle import dsp_ref_cpu as orc
    ch = Chain(ChainConfig(n_in, FS, 3, 2, None, orc.CONFIG3_GAINS, n_fft=256), B, gpu,
               keep_y=keep_y)
    assert ch.tile_len == 48, "the geometry must take a single-pass kernel of 48-output sub-chunks"
    return ch


def _layout(ch):
    """(ntiles, offset of the flag array, its bytes): csrc/chain_plan.hip
    tile_ws(), read as tests/test_gpu_graph.py does."""
    ntiles = -(-ch.n_out // (64 * ch.tile_len))
    off = 256 + ((ch.B * ntiles * 12 * 8 + 255) & ~255)
    return ntiles, off, ch.B * ntiles * 4


def _clean(ch):
    """Status word 0 and every hand-off flag 0."""
    _, off, nbytes = _layout(ch)
    assert off + nbytes <= ch.workspace.numel()
    return (ch.handoff_ok() and int(ch.workspace[:4].view(torch.int32).item()) == 0
            and int(torch.count_nonzero(ch.workspace[off:off + nbytes]).item()) == 0)


def _last_states(ch):
    ntiles, _, _ = _layout(ch)
    st = ch.workspace[256:256 + ch.B * ntiles * 96].view(torch.float64).reshape(ch.B, ntiles, 12)
    return st[:, -1].cpu().numpy()


def _run(gpu, x, keep_y=True, ch=None):
    """y, z (numpy) of one traced call on the rows of x, chained mode; the
    trace must show the single-pass launch and no three-launch mode."""
    from dspcore import _lib
    ch = ch or _chain(gpu, x.shape[1], x.shape[0], keep_y)
    with _chained():
        _lib.trace_enable(True)
        _lib.trace_read()
        try:
            y, z, _ = ch.run(torch.from_numpy(np.array(x, dtype=np.float32, order="C")).to(gpu))
            torch.cuda.synchronize(gpu)
            names = [n for n, _ in _lib.trace_read()]
        finally:
            _lib.trace_enable(False)
    assert "chain_tile" in names and "chain_tile_agg" not in names, names
    assert _clean(ch)
    return (None if y is None else y.cpu().numpy()), z.cpu().numpy(), ch


def _same(a, b):
    """Bitwise equality (NaNs by their bits)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _input(n_in):
    x = np.random.default_rng(n_in).uniform(-1, 1, (ROWS, n_in)).astype(np.float32)
    x[1] *= 40.0  # driven into the clip
    return x


_REF = {}


def _ref(gpu, n_in):
    """The rows' B = 1 results (the unpaired path), computed once per shape:
    x, y, z, and the last tile's published end state of each row."""
    if n_in not in _REF:
        x = _input(n_in)
        ch = _chain(gpu, n_in, 1)
        ys, zs, st = [], [], []
        for r in range(ROWS):
            y, z, _ = _run(gpu, x[r:r + 1], ch=ch)
            ys.append(y[0])
            zs.append(z[0])
            st.append(_last_states(ch)[0])
        for a in (x, *ys, *zs):
            a.setflags(write=False)
        _REF[n_in] = (x, np.stack(ys), np.stack(zs), np.stack(st))
    return _REF[n_in]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_in", sorted(SHAPES))
def test_rows_bitwise_the_single_channel_call(gpu, n_in, B):
    x, ry, rz, rst = _ref(gpu, n_in)
    y, z, ch = _run(gpu, x[:B])
    assert _same(y, ry[:B]) and _same(z, rz[:B])
    if SHAPES[n_in] is not None:
        paired = [not np.array_equal(s, r) for s, r in zip(_last_states(ch), rst[:B])]
        assert paired == [SHAPES[n_in] and B >= 2] * B, (n_in, B, paired)
    # a second call on the same workspace
    y2, z2, _ = _run(gpu, x[:B], ch=ch)
    assert _same(y2, y) and _same(z2, z)
    if B > 1:
        # the other half, another partner
        yr, zr, _ = _run(gpu, x[:B][::-1], ch=ch)
        assert _same(yr[::-1], ry[:B]) and _same(zr[::-1], rz[:B])
        # y = NULL
        yn, zn, _ = _run(gpu, x[:B], keep_y=False)
        assert yn is None and _same(zn, rz[:B])


@pytest.mark.parametrize("n_in", sorted(SHAPES))
def test_rows_match_the_oracle(gpu, n_in):
    from oracle import dsp_ref_cpu as orc
    x = _input(n_in)[:3]
    y, z, _ = _run(gpu, x)
    for r in range(3):
        oy, oz, _, _, _ = orc.chain(x[r], FS, 3, 2, orc.CONFIG3_GAINS, None, 256)
        assert y[r].shape == oy.shape
        ey = float(np.max(np.abs(y[r] - oy)))
        ez = float(np.max(np.abs(z[r] - oz)))
        print(f"n_in {n_in} row {r}: y err {ey:.3g}, z err {ez:.3g}")
        assert ey <= SRC_ATOL * max(1.0, float(np.abs(oy).max())) and ez <= EQ_ATOL
    assert np.abs(z[1]).max() == 1.0, "row 1 must reach the clip"


@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("where", [2500, 1000], ids=["tail-tile", "tile-before"])
@pytest.mark.parametrize("half", [0, 1])
def test_nonfinite_stays_in_its_channel(gpu, half, where, bad):
    """An inf or NaN in one channel of a pair, in its tail tile's x or in the
    tile before: the partner's rows are those of a clean run, the channel's own
    rows those of its B = 1 call (the repair kernel's rerun)."""
    n_in = 2944
    x, ry, rz, _ = _ref(gpu, n_in)
    xb = x[:2].copy()
    xb[half, where] = bad
    ys, zs, _ = _run(gpu, xb[half:half + 1])   # the channel alone
    assert not (np.isfinite(ys).all() and np.isfinite(zs).all())
    y, z, _ = _run(gpu, xb)
    other = 1 - half
    assert _same(y[other], ry[other]) and _same(z[other], rz[other])
    assert _same(y[half], ys[0]) and _same(z[half], zs[0])


def test_graph_replay(gpu):
    """Chain.run captured and replayed as bench.py does it, B = 4, fresh x
    before each replay."""
    n_in, B = 2944, 4
    ch = _chain(gpu, n_in, B)
    gen = torch.Generator(device=gpu).manual_seed(77)
    xs = [torch.rand((B, n_in), generator=gen, device=gpu) * 2 - 1 for _ in range(3)]
    with _chained():
        eager = []
        for x in xs:
            y, z, m = ch.run(x)
            eager.append((y.clone(), z.clone(), m.clone()))
        assert _clean(ch)
        x_static = xs[2].clone()
        graph = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(gpu)
        cap.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(cap):
            ch.run(x_static)
            with torch.cuda.graph(graph, stream=cap):
                ch.run(x_static, check=False)
        torch.cuda.current_stream(gpu).wait_stream(cap)
        torch.cuda.synchronize(gpu)
    for rep in range(4):
        x_static.copy_(xs[rep % 3])
        graph.replay()
        torch.cuda.synchronize(gpu)
        ye, ze, me = eager[rep % 3]
        assert torch.equal(ch.y, ye) and torch.equal(ch.z, ze) and torch.equal(ch.mag, me), rep
        assert _clean(ch), rep
    # the eager rows are the single-channel rows
    one = _chain(gpu, n_in, 1)
    for b in (0, 3):
        y1, z1, _ = _run(gpu, xs[0][b:b + 1].cpu().numpy(), ch=one)
        assert _same(eager[0][0][b].cpu().numpy(), y1[0])
        assert _same(eager[0][1][b].cpu().numpy(), z1[0])
    del graph
