"""The path bench.py times, parity-tested: Chain.run captured into a HIP graph
(torch.cuda.CUDAGraph, as bench.py:measure captures it) and replayed with a
fresh x copied into the captured input before every replay (VERDICT round 5,
item 1).

What the replays rest on: the single-pass kernels hand each tile's end state
to the next tile of the channel through the workspace, and a completed launch
leaves every hand-off flag zero for the next one (csrc/chain_tile.hip, file
comment).  A flag left set would hand a later replay the previous call's
state -- wrong z, and no give-up to report it.  So after every replay:
  * y, z and |X| are bitwise the eager Chain.run on the same x;
  * spot rows are within the parity tolerances of the oracle
    (reference dsp_core.py:133-254 for y and z, :68-98 for |X|);
  * the workspace's status word and its whole flag array read zero.
Geometries: config 3 at full size (k_chain_tile, 4096 channels x 24 tiles:
many dispatch generations), config 5 at full size (the persistent
k_chain_gcp<160, 147>), the config-4 kernel at 16384 channels, two of the
app's ratios on the per-phase kernels (2/1 and 3/4, 4096 channels) and the
app's default 1/1 (the cascade alone: chained tiles at 4096 channels, the
three-launch mode at 2).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SRC_ATOL = 2e-6
EQ_ATOL = 1e-5
CHAIN_MAG_RTOL = 1e-5


def _flag_region(ch):
    """(offset, bytes) of the hand-off flag array in Chain's workspace: the
    layout of csrc/chain_plan.hip tile_ws() -- a 256-byte status header, the
    [B][ntiles][12] float64 end states, then [B][ntiles] uint32 flags, each
    region 256-byte aligned."""
    tile = 64 * ch.tile_len
    ntiles = -(-ch.n_out // tile)
    align = lambda v: (v + 255) & ~255  # noqa: E731
    states = ch.B * ntiles * 12 * 8
    off = 256 + align(states)
    return off, ch.B * ntiles * 4


def _workspace_clear(ch):
    ws = ch.workspace
    off, nbytes = _flag_region(ch)
    assert off + nbytes <= ws.numel()
    status = int(ws[:4].view(torch.int32).item())
    flags_set = int(torch.count_nonzero(ws[off:off + nbytes]).item())
    return status, flags_set


@pytest.mark.parametrize("tag,B,fs,L,M,K,kernel_rows", [
    ("config3", 4096, 48000, 3, 2, None, (0, 2047, 4095)),
    ("config5", 8192, 44100, 160, 147, 1023, (0, 8191)),
    ("config4-kernel", 16384, 48000, 3, 2, None, (0, 16383)),
    # the per-phase kernels (csrc/chain_pp.h): an app ratio up and one down
    ("ratio-2/1", 4096, 48000, 2, 1, None, (0, 4095)),
    ("ratio-3/4", 4096, 48000, 3, 4, None, (0, 4095)),
    # the SRC bypass: the cascade alone (one-tap SRC, y is x)
    ("eq-only", 4096, 48000, 1, 1, None, (0, 4095)),
    # ... and at 2 channels, where it takes the three-launch mode
    ("eq-only-b2", 2, 48000, 1, 1, None, (0, 1)),
])
def test_graph_replay_matches_eager(gpu, tag, B, fs, L, M, K, kernel_rows):
    from dspcore.chain import Chain, ChainConfig
    from oracle import dsp_ref_cpu as orc
    n_in, n_fft = 48000, 4096
    cfg = ChainConfig(n_in, fs, L, M, K, orc.CONFIG3_GAINS, n_fft=n_fft)
    ch = Chain(cfg, B, gpu)
    assert ch.tile_len > 0, "the geometry must take a single-pass kernel"
    gen = torch.Generator(device=gpu).manual_seed(606)
    xs = []
    for r in range(3):
        x = torch.rand((B, n_in), generator=gen, device=gpu) * 2 - 1
        # a clipped row, a different one per replay (x 8 at the app's ratios:
        # tests/test_gpu_pp.py says why)
        x[r % B] *= 8.0 if tag.startswith("ratio") else 40.0
        xs.append(x)
    # eager reference runs (hand-off status checked after each)
    eager = []
    for x in xs:
        y, z, m = ch.run(x)
        eager.append((y.clone(), z.clone(), m.clone()))
    assert _workspace_clear(ch) == (0, 0)

    # capture one step exactly as bench.py does
    x_static = torch.empty_like(xs[0])
    x_static.copy_(xs[2])
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
        i = rep % 3
        x_static.copy_(xs[i])
        graph.replay()
        torch.cuda.synchronize(gpu)
        ye, ze, me = eager[i]
        y_now = x_static if ch.identity_src else ch.y   # the bypass: y is x
        assert torch.equal(y_now, ye), (tag, rep, "y")
        assert torch.equal(ch.z, ze), (tag, rep, "z")
        assert torch.equal(ch.mag, me), (tag, rep, "mag")
        assert _workspace_clear(ch) == (0, 0), (tag, rep)
        assert ch.handoff_ok()
        if rep < 3:
            rows = kernel_rows if rep == 0 else kernel_rows[:1] if tag == "config5" else kernel_rows[-1:]
            for b in rows:
                ry, rz, _, rmag, _ = orc.chain(xs[i][b].cpu().numpy(), fs, L, M, orc.CONFIG3_GAINS,
                                               K, n_fft)
                y = y_now[b].cpu().numpy()
                z = ch.z[b].cpu().numpy()
                mag = ch.mag[b].cpu().numpy()
                assert np.max(np.abs(y - ry)) <= SRC_ATOL * max(1.0, np.abs(ry).max())
                assert np.max(np.abs(z - rz)) <= EQ_ATOL
                assert np.max(np.abs(mag - rmag)) <= CHAIN_MAG_RTOL * np.max(rmag)
    del graph, eager, xs
    torch.cuda.empty_cache()
