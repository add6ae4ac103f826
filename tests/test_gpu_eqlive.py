"""The live EQ on the GPU (include/dspcore_eqlive.h) against its host model
(tests/eqlive_model.py): scipy.signal.lfilter band by band, every band's zi
carried while the gains change from block to block.

Bounds.  z: EQ_ATOL = 1e-5, the project's bound for every EQ path against
float64 scipy.  Exit states: 1e-9 of the row's largest component,
tests/test_gpu_stream.py's bound (the kernel's arithmetic restated in numpy,
chunk scan included, stays below 6e-11 there on these cases)."""
import numpy as np
import pytest
import torch

import eqlive_model as model

pytestmark = pytest.mark.gpu

EQ_ATOL = 1e-5
STATE_RTOL = 1e-9
KEYS8 = ("Sub-Bass", "Bass", "Low Mids", "High Mids", "Presence", "Brilliance", "Air", "Mystery")
CONFIG3 = (6, -4, 3, -3, 5, -6, 2.5, -2.5)
LENGTHS = {2048: (33, 2048, 1, 31, 2047, 32), 2049: (65, 2049, 63)}
# input scale per rate: white noise whose +-15 dB settings leave the clip rare
# (at 5512 Hz three bands sit on the 0.45 fs clamp and stack to +45 dB)
SCALE = {352800: 0.05, 72000: 0.05, 5512: 0.01}


def histories(slots, blocks):
    """Five rows' gains per block (the phase cycles every four blocks)."""
    keys = KEYS8[:slots]
    up, down = dict.fromkeys(keys, 15.0), dict.fromkeys(keys, -15.0)
    alt = {k: (15.0 if i % 2 == 0 else -15.0) for i, k in enumerate(keys)}
    cfg3 = dict(zip(keys, CONFIG3))
    flat = dict.fromkeys(keys, 0.0)
    quiet = dict(flat, **{keys[-1]: 0.05})
    phases = [
        (up, down, alt, cfg3),                 # swung between the extremes
        (cfg3, flat, quiet, down),             # ring-out, then re-activation over a ringing state
        (flat, quiet, flat, flat),             # never active
        (flat, quiet, flat, cfg3),             # active only from block 3
        (up, down, alt, cfg3),                 # row 0 again, overdriven
    ]
    return [[p[i % 4] for i in range(blocks)] for p in phases]


def signal(fs, n, seed):
    x = np.random.default_rng(seed).uniform(-1, 1, (5, n)) * SCALE[fs]
    x[4] = 8 * x[0]
    return x.astype(np.float32)


def live_run(gpu, fs, hist, x, lengths, max_n):
    """The blocks through one LiveEq with set_gains before each: (z, state, the object)."""
    from dspcore.eqlive import LiveEq
    eq = LiveEq(fs, [h[0] for h in hist], max_n, gpu)
    xd = torch.from_numpy(x).to(gpu)
    z = torch.empty_like(xd)
    at = 0
    for i, n in enumerate(lengths):
        if i:
            eq.set_gains([h[i] for h in hist])
        eq.apply(xd[:, at:at + n], out=z[:, at:at + n])
        at += n
    return z.cpu().numpy(), eq.state_dict()["zi"].numpy(), eq


def check_against_model(tag, z, state, want_z, want_state):
    ez = float(np.max(np.abs(z.astype(np.float64) - want_z)))
    es = float(np.max(np.abs(state - want_state)) / np.max(np.abs(want_state)))
    clipped = float(np.mean(np.abs(want_z[:4]) >= 1.0))
    print(f"{tag}: max|z - model| {ez:.3g}, exit state rel {es:.3g}, clipped share {clipped:.3%}")
    assert clipped < 0.10, "the clip must not hide an error in the rows that are not overdriven"
    assert ez <= EQ_ATOL
    assert es <= STATE_RTOL


# ---------------------------------------------------------------------------
# 1. constant gains
# ---------------------------------------------------------------------------
def test_constant_gains_match_the_oracle_and_the_bank(gpu):
    from conftest import golden, golden_gains
    from dspcore.eqbank import EqBank
    from dspcore.eqlive import LiveEq
    g = golden("eq")
    x32 = g["x32"]
    x = torch.from_numpy(np.stack([x32, 0.5 * x32])).to(gpu)
    n = x32.size
    served = 0
    for i in range(10):
        gains, fs = golden_gains(g[f"gains_{i}"]), int(g[f"fs_{i}"])
        if not gains:
            continue
        z = LiveEq(fs, gains, n, gpu, batch=2).apply(x).cpu().numpy()
        ref = g[f"z32_{i}"]
        bank = EqBank(fs, [gains, gains], n, gpu).apply(x)[0].cpu().numpy()
        eo = float(np.max(np.abs(z[0] - ref)))
        eb = float(np.max(np.abs(z - bank)))
        print(f"case {i} fs {fs}: vs reference {eo:.3g}, vs EqBank {eb:.3g}")
        assert eo <= EQ_ATOL and eb <= EQ_ATOL
        if all(abs(v) < 0.1 for v in gains.values()):
            assert np.array_equal(z[0].view(np.uint32), x32.view(np.uint32))   # the copy path
        served += 1
    assert served >= 9


# ---------------------------------------------------------------------------
# 2. gains changed every block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [352800, 72000, 5512])
@pytest.mark.parametrize("max_n", [2048, 2049])
def test_gains_changed_every_block_match_the_model(gpu, fs, max_n):
    lengths = LENGTHS[max_n]
    hist = histories(6, len(lengths))
    x = signal(fs, sum(lengths), 11 + max_n)
    want_z, want_state = model.run(fs, hist, x, lengths)
    z, state, eq = live_run(gpu, fs, hist, x, lengths, max_n)
    assert eq.planner.ever_active.tolist() == [True, True, False, len(lengths) > 3, True]
    check_against_model(f"fs {fs} max_n {max_n}", z, state, want_z, want_state)
    assert np.array_equal(z[2].view(np.uint32), x[2].view(np.uint32)) and not state[2].any()
    assert np.max(np.abs(z[4])) == 1.0                           # the overdriven row clips


@pytest.mark.parametrize("slots", [1, 7, 8])
def test_other_slot_counts_match_the_model(gpu, slots):
    fs, lengths = 72000, LENGTHS[2048]
    hist = histories(slots, len(lengths))
    x = signal(fs, sum(lengths), 40 + slots)
    want_z, want_state = model.run(fs, hist, x, lengths)
    z, state, eq = live_run(gpu, fs, hist, x, lengths, 2048)
    assert eq.slots == slots and state.shape == (5, 2 * slots)
    check_against_model(f"{slots} slots", z, state, want_z, want_state)


# ---------------------------------------------------------------------------
# 3. set_gains semantics, the copy path, non-finite input, layouts
# ---------------------------------------------------------------------------
def test_set_gains_with_the_same_gains_changes_nothing(gpu):
    from dspcore.eqlive import LiveEq
    fs, lengths = 72000, (700, 2048, 33)
    hist = histories(6, 1)
    gains = [h[0] for h in hist]
    x = torch.from_numpy(signal(fs, sum(lengths), 5)).to(gpu)
    a, b = LiveEq(fs, gains, 2048, gpu), LiveEq(fs, gains, 2048, gpu)
    ptrs = (a.table.data_ptr(), a.row_group.data_ptr(), a._state.data_ptr())
    at = 0
    for n in lengths:
        a.set_gains([dict(g) for g in gains])
        za, zb = a.apply(x[:, at:at + n]), b.apply(x[:, at:at + n])
        assert torch.equal(za, zb)
        at += n
    assert torch.equal(a._state, b._state)
    assert ptrs == (a.table.data_ptr(), a.row_group.data_ptr(), a._state.data_ptr())
    with pytest.raises(ValueError, match="band slots"):
        a.set_gains([dict(reversed(list(g.items()))) for g in gains])
    with pytest.raises(ValueError, match="max_groups"):
        LiveEq(fs, gains, 2048, gpu, max_groups=2)


def test_nonfinite_input_copy_rows_and_poisoned_rows(gpu):
    from dspcore.eqlive import LiveEq
    fs, lengths = 72000, (300, 300, 300, 64)
    hist = histories(6, len(lengths))
    clean = signal(fs, sum(lengths), 6)
    x = clean.copy()
    x[2, 10], x[2, 350], x[2, 351] = np.inf, np.nan, -np.inf     # the never-active row
    x[1, 300 + 40] = np.inf                                      # block 2 of an active row
    z, state, _ = live_run(gpu, fs, hist, x, lengths, 2048)
    zc, sc, _ = live_run(gpu, fs, hist, clean, lengths, 2048)
    assert np.array_equal(z[2].view(np.uint32), x[2].view(np.uint32)) and not state[2].any()
    assert np.array_equal(z[1, :340], zc[1, :340]) and np.isfinite(z[1, :340]).all()
    assert np.isnan(z[1, 341:]).all() and np.isnan(state[1]).all()
    for r in (0, 3, 4):
        assert np.array_equal(z[r], zc[r]) and np.array_equal(state[r], sc[r]), r
    # a non-finite entry state: an all-NaN row
    eq = LiveEq(fs, [h[0] for h in hist], 2048, gpu)
    zi = np.zeros((5, 12))
    zi[0, 7] = np.inf
    eq.load_state_dict({"zi": zi})
    out = eq.apply(torch.from_numpy(clean[:, :100].copy()).to(gpu)).cpu().numpy()
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()
    assert np.isnan(eq.state_dict()["zi"].numpy()[0]).all()
    # a foreign row-group index: NaN rows, nothing else touched
    eq = LiveEq(fs, [h[0] for h in hist], 2048, gpu)
    eq.row_group[3] = 99
    out = eq.apply(torch.from_numpy(clean[:, :100].copy()).to(gpu)).cpu().numpy()
    assert np.isnan(out[3]).all() and np.isnan(eq.state_dict()["zi"].numpy()[3]).all()
    assert np.array_equal(out[[0, 1, 2, 4]], zc[[0, 1, 2, 4], :100])


def test_in_place_pitches_misaligned_rows_and_empty_blocks(gpu):
    from dspcore.eqlive import LiveEq
    fs, n = 72000, 777
    hist = histories(6, 4)
    gains = [h[3] for h in hist]
    x = signal(fs, n, 8)
    xd = torch.from_numpy(x).to(gpu)
    ref_eq = LiveEq(fs, gains, 2048, gpu)
    ref = ref_eq.apply(xd)
    ref_state = ref_eq._state.clone()
    for pitch, offset in ((n + 1, 1), (780, 0), (784, 4)):
        flat = torch.zeros(5 * pitch + offset, dtype=torch.float32, device=gpu)
        view = flat[offset:offset + 5 * pitch].view(5, pitch)[:, :n]
        view.copy_(xd)
        eq = LiveEq(fs, gains, 2048, gpu)
        assert eq.apply(view[:, :0]).shape == (5, 0) and not eq._state.any()      # n == 0
        out = eq.apply(view, out=view)                                             # x == y
        assert out is view and torch.equal(view, ref) and torch.equal(eq._state, ref_state)
    with pytest.raises(ValueError):
        ref_eq.apply(xd[:3])
    with pytest.raises(ValueError):
        ref_eq.apply(torch.zeros((5, 2049), dtype=torch.float32, device=gpu))


def test_one_launch_per_block(gpu):
    from dspcore import _lib
    from dspcore.eqlive import LiveEq
    hist = histories(6, 1)
    eq = LiveEq(72000, [h[0] for h in hist], 2048, gpu)
    xd = torch.from_numpy(signal(72000, 2047, 9)).to(gpu)
    _lib.trace_enable(True)
    try:
        eq.apply(xd, out=torch.empty_like(xd))
        names = [k for k, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    assert names == ["iir_live"]


# ---------------------------------------------------------------------------
# 4. StreamChain(live=True)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("L,M", [(3, 2), (1, 1)])
def test_stream_chain_live(gpu, L, M):
    from dspcore.stream import StreamChain
    fs_in, parts = 48000, (1, 700, 0, 1024, 37)
    hist = histories(6, len(parts) + 1)[:3]
    x = np.random.default_rng(12).uniform(-1, 1, (3, sum(parts))).astype(np.float32) * 0.05
    xd = torch.from_numpy(x).to(gpu)

    def run(sc, lo, hi, at):
        ys, zs = [], []
        for i in range(lo, hi):
            if i and sc.live is not None:
                sc.set_gains([h[i] for h in hist])
            if i < len(parts):
                y, z = sc.push(xd[:, at:at + parts[i]])
                at += parts[i]
            else:
                y, z = sc.flush()
            ys.append(y.clone())
            zs.append(z.clone())
        return ys, zs, at

    first = [h[0] for h in hist]
    sc = StreamChain(fs_in, L, M, None, first, 3, 1024, gpu, live=True)
    ys, zs, _ = run(sc, 0, len(parts) + 1, 0)
    plain = StreamChain(fs_in, L, M, None, first[0], 3, 1024, gpu)
    pys, _, _ = run(plain, 0, len(parts) + 1, 0)
    lengths = [int(y.shape[1]) for y in ys]
    y = torch.cat(ys, dim=1)
    assert torch.equal(y, torch.cat(pys, dim=1))                 # y: the plain chain's, bitwise
    assert sum(lengths) == -(-sum(parts) * L // M)
    want_z, want_state = model.run(sc.fs_out, hist, y.cpu().numpy(), lengths)
    z = torch.cat(zs, dim=1)
    check_against_model(f"stream {L}/{M}", z.cpu().numpy(), sc.state_dict()["eq_state"].numpy(),
                        want_z, want_state)
    # checkpoint after three pushes, continue in a fresh object
    sc.reset()
    sc.set_gains(first)
    ys1, zs1, at = run(sc, 0, 3, 0)
    sd = sc.state_dict()
    other = StreamChain(fs_in, L, M, None, [h[2] for h in hist], 3, 1024, gpu, live=True)
    other.load_state_dict(sd)
    ys2, zs2, _ = run(other, 3, len(parts) + 1, at)
    assert torch.equal(torch.cat(ys1 + ys2, dim=1), y)
    assert torch.equal(torch.cat(zs1 + zs2, dim=1), z)
    with pytest.raises(RuntimeError, match="live=True"):
        plain.set_gains(first[0])


# ---------------------------------------------------------------------------
# 5. graph capture
# ---------------------------------------------------------------------------
def test_captured_apply_follows_set_gains(gpu):
    """One apply() in a graph; the table, the row groups and the state keep
    their addresses, so a replay after set_gains() runs the new gains."""
    from dspcore.eqlive import LiveEq
    fs, n = 72000, 1500
    hist = histories(6, 2)
    x = signal(fs, 2 * n, 13)
    want_z, want_state = model.run(fs, hist, x, (n, n))
    eq = LiveEq(fs, [h[0] for h in hist], 2048, gpu)
    x_static = torch.from_numpy(x[:, :n].copy()).to(gpu)
    z_static = torch.empty_like(x_static)
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream(gpu)
    cap.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(cap):
        eq.apply(x_static, out=z_static)
        with torch.cuda.graph(graph, stream=cap):
            eq.apply(x_static, out=z_static)
    torch.cuda.current_stream(gpu).wait_stream(cap)
    torch.cuda.synchronize(gpu)
    eq.reset()                                                   # the warm-up moved the state
    graph.replay()
    z0 = z_static.clone()
    eq.set_gains([h[1] for h in hist])
    x_static.copy_(torch.from_numpy(x[:, n:].copy()))
    graph.replay()
    torch.cuda.synchronize(gpu)
    z = np.concatenate([z0.cpu().numpy(), z_static.cpu().numpy()], axis=1)
    check_against_model("graph", z, eq.state_dict()["zi"].numpy(), want_z, want_state)
    del graph
