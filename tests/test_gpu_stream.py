"""Streaming on the GPU (include/dspcore_stream.h): the stateful cascade
against the one-shot cascade, the oracle and a float64 model of the state;
non-finite input; StreamChain end to end against the one-shot chain and the
oracle; reset and checkpoint.

Bounds.  Stream and one-shot cascade run the same float64 recursion with
different chunking, so their float64 outputs differ by float64 rounding
(~1e-12) and their float32 roundings by at most one ulp of a value in [-1, 1]
(1.2e-7); two ulps are allowed: Z_ULP2.  Against the oracle the project's
EQ_ATOL / SRC_ATOL hold.  The exit state against a float64 host run of
design.state_space's recursion over the same samples: 1e-9 of the largest
state component (float64 rounding over 8000 steps of a recursion whose
40 Hz band has its poles at |r| = 0.9995; measured 2.5e-10 with six to eight
bands, 7e-12 with the 150 Hz band alone).  The SRC
output of the stream is bitwise the one-shot kernel's: the same kernel sums
every output's taps in the same order wherever the block boundaries fall."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Z_ULP2 = 2.4e-7
SRC_ATOL = 2e-6
EQ_ATOL = 1e-5
CROSS_PATH = 2e-6
FS_EQ = 72000
N_EQ = 8000
CUTS = [1, 34, 700, 1420, 2999, 3000]
FORBIDDEN = {"iir_prep", "iir_state", "iir_carry", "iir_apply"}


def _gains():
    from oracle import dsp_ref_cpu as orc
    return orc.CONFIG3_GAINS


def _sos(case):
    from dspcore import design
    g = dict(_gains())
    if case == "s1":
        g = {"Bass": -4}
    elif case == "s7":
        g["Air"] = 2.5
    elif case == "s8":
        g["Air"] = 2.5
        g["Body"] = -1.5
    sos = np.ascontiguousarray(design.eq_plan(FS_EQ, g).sos)
    if case == "b0":    # a stage with b0 == 0: the realisation keeps its gains (not NORM)
        sos = np.vstack([sos[:2], [[0.0, 0.7, 0.2, -0.5, 0.25]]])
    return sos


_ROWS = {}


def _rows():
    if "x" not in _ROWS:
        x = np.random.default_rng(11).uniform(-1, 1, (3, N_EQ)).astype(np.float32)
        x[1] *= 8
        _ROWS["x"] = x
    return _ROWS["x"]


def _blocks(n, cuts):
    edges = [0] + list(cuts) + [n]
    return list(zip(edges[:-1], edges[1:]))


def _stream_cascade(xd, sos, cuts, mode="fresh"):
    """z and the final state of xd filtered block by block.  mode: 'fresh' a
    new zf per block, 'inplace' one tensor as zi and zf, both starting from
    zi=None / zeros respectively."""
    from dspcore import ops
    B, n = xd.shape
    z = torch.empty_like(xd)
    state = None
    if mode == "inplace":
        state = torch.zeros((B, 2 * sos.shape[0]), dtype=torch.float64, device=xd.device)
    for a, b in _blocks(n, cuts):
        if mode == "inplace":
            _, zf = ops.biquad_cascade_state(xd[:, a:b], sos, True, zi=state, out=z[:, a:b],
                                             zf=state)
            assert zf is state
        else:
            _, state = ops.biquad_cascade_state(xd[:, a:b], sos, True, zi=state, out=z[:, a:b])
    return z, state


def _state_model(sos, x):
    """float64 host run of design.state_space's recursion X' = A X + B u."""
    from dspcore import design
    A, Bv = design.state_space(sos)
    X = np.zeros((x.shape[0], Bv.size))
    for u in x.T.astype(np.float64):
        X = X @ A.T + np.outer(u, Bv)
    return X


@pytest.mark.parametrize("case", ["c3", "s1", "s7", "s8", "b0"])
def test_cascade_state_matches_one_shot_oracle_and_state_model(gpu, case):
    from dspcore import ops
    sos = _sos(case)
    x = _rows()
    xd = torch.from_numpy(x).to(gpu)
    one = ops.biquad_cascade(xd, sos, True).cpu().numpy()
    z, zf = _stream_cascade(xd, sos, CUTS)
    z = z.cpu().numpy()
    err = float(np.max(np.abs(z - one)))
    print(f"{case}: stream vs one-shot {err:.3g}")
    assert err <= Z_ULP2
    if case == "c3":
        from oracle import dsp_ref_cpu as orc
        ref = np.stack([orc.equaliser(r.astype(np.float64), FS_EQ, _gains()) for r in x])
        eo = float(np.max(np.abs(z - ref)))
        print(f"{case}: stream vs oracle {eo:.3g}")
        assert eo <= EQ_ATOL
    want = _state_model(sos, x)
    got = zf.cpu().numpy()
    assert got.shape == want.shape == (3, 2 * sos.shape[0])
    es = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{case}: exit state rel err {es:.3g}")
    assert es <= 1e-9
    # the state is that of the unclipped recursion: row 1 (x8) clips hard
    assert np.max(np.abs(one[1])) == 1.0
    # in place (zi is zf) and starting from zi=None are the same computation
    z2, zf2 = _stream_cascade(xd, sos, CUTS, mode="inplace")
    assert torch.equal(z2.cpu(), torch.from_numpy(z))
    assert torch.equal(zf2, zf)
    # rows do not depend on the batch: a B = 1 call on row 2 alone
    z1, zf1 = _stream_cascade(xd[2:3].contiguous(), sos, CUTS)
    assert torch.equal(z1.cpu()[0], torch.from_numpy(z[2]))
    assert torch.equal(zf1[0], zf[2])


def test_cascade_state_edge_arguments(gpu):
    """x == y in place, zf=None with a padded state pitch untouched beyond 2S,
    S == 0 (clip only, no state), n == 0 leaves zf as it is."""
    from dspcore import _lib, ops
    sos = _sos("c3")
    x = _rows()
    xd = torch.from_numpy(x).to(gpu)
    z, zf = _stream_cascade(xd, sos, [700])
    buf = xd.clone()
    st = torch.full((3, 16), 7.0, dtype=torch.float64, device=gpu)
    st[:, :12] = 0
    for a, b in _blocks(N_EQ, [700]):
        ops.biquad_cascade_state(buf[:, a:b], sos, True, zi=st, out=buf[:, a:b], zf=st)
    assert torch.equal(buf, z)
    assert torch.equal(st[:, :12], zf) and bool((st[:, 12:] == 7.0).all())
    # n == 0: nothing launched, zf kept
    keep = st.clone()
    ops.biquad_cascade_state(buf[:, :0], sos, True, zi=st, out=buf[:, :0], zf=st)
    assert torch.equal(st, keep)
    # S == 0: y = clip(x), the state tensor is not touched
    z0, s0 = ops.biquad_cascade_state(xd, np.zeros((0, 5)), True)
    assert torch.equal(z0, xd.clamp(-1, 1)) and not bool(s0.any())
    z0, _ = ops.biquad_cascade_state(xd, np.zeros((0, 5)), False)
    assert torch.equal(z0, xd)
    with pytest.raises(RuntimeError):
        ops.biquad_cascade_state(xd, np.tile([1.0, 0, 0, 0, 0], (9, 1)), True)
    assert "stages" in _lib.last_error()


def test_nonfinite_input_poisons_the_channel_only(gpu):
    from dspcore import ops
    sos = _sos("c3")
    n, cuts = 4000, [1000, 2000, 3000]
    clean = np.random.default_rng(12).uniform(-0.9, 0.9, (3, n)).astype(np.float32)
    x = clean.copy()
    x[0, 1500] = np.nan          # block 2 of 4
    x[1, 1501] = np.inf
    xd = torch.from_numpy(x).to(gpu)
    one = ops.biquad_cascade(xd, sos, True).cpu().numpy()
    z, zf = _stream_cascade(xd, sos, cuts)
    z, zf = z.cpu().numpy(), zf.cpu().numpy()
    assert np.array_equal(np.isnan(z), np.isnan(one))
    fin = ~np.isnan(one)
    assert not np.isinf(z).any()
    assert float(np.max(np.abs(z[fin] - one[fin]))) <= Z_ULP2
    assert np.isfinite(z[0, :1500]).all() and np.isfinite(z[1, :1501]).all()
    assert np.isnan(z[0, 1501:]).all() and np.isnan(z[1, 1502:]).all()
    assert np.isnan(z[:2, 2000:]).all()          # every later block
    assert np.isnan(zf[:2]).all() and np.isfinite(zf[2]).all()
    zc, zfc = _stream_cascade(torch.from_numpy(clean).to(gpu), sos, cuts)
    assert np.array_equal(z[2], zc.cpu().numpy()[2])
    assert np.array_equal(zf[2], zfc.cpu().numpy()[2])
    # a non-finite entry state gives an all-NaN row
    zi = torch.zeros((3, 12), dtype=torch.float64, device=gpu)
    zi[1, 5] = float("inf")
    zn, zfn = ops.biquad_cascade_state(torch.from_numpy(clean).to(gpu)[:, :100], sos, True, zi=zi)
    zn = zn.cpu().numpy()
    assert np.isnan(zn[1]).all() and np.isfinite(zn[[0, 2]]).all()
    assert bool(torch.isnan(zfn[1]).all())


# ---------------------------------------------------------------------------
# StreamChain
# ---------------------------------------------------------------------------
N_IN = 6000
FS_IN = 48000
RATIOS = [(3, 2, None), (2, 1, None), (1, 2, None), (8, 7, None), (1, 8, None), (8, 1, None),
          (1, 1, None), (160, 147, 1023)]
PARTS = {"even": [480] * 12 + [240], "ragged": [1, 37, 3, 500, 1, 959, 2000, 2499]}
MAX_BLOCK = 2499
_REF = {}


def _chain_input():
    if "x" not in _REF:
        _REF["x"] = np.random.default_rng(13).uniform(-1, 1, (3, N_IN)).astype(np.float32)
    return _REF["x"]


def _one_shot(gpu, L, M, K):
    """One-shot references for a ratio, computed once: the SRC kernel's y, the
    two-launch Chain's z (dsp_chain_path(1)), the oracle's y and z."""
    key = (L, M, K)
    if key not in _REF:
        from dspcore import _lib, design, ops
        from dspcore.chain import Chain, ChainConfig
        from oracle import dsp_ref_cpu as orc
        x = _chain_input()
        xd = torch.from_numpy(x).to(gpu)
        if L == 1 and M == 1:
            y = x.copy()
        else:
            y = ops.src_polyphase(xd, design.src_plan(N_IN, FS_IN, M, L, K)).cpu().numpy()
        prev = _lib.chain_path(1)
        try:
            ch = Chain(ChainConfig(N_IN, FS_IN, L, M, K, _gains(), n_fft=256), 3, gpu)
            z = ch.run(xd)[1].cpu().numpy().copy()
        finally:
            _lib.chain_path(prev)
        oy, oz = [], []
        for r in x:
            ry, rz, _, _, _ = orc.chain(r.astype(np.float64), FS_IN, L, M, _gains(), K, 256)
            oy.append(ry)
            oz.append(rz)
        _REF[key] = (y, z, np.stack(oy), np.stack(oz))
    return _REF[key]


def _run_stream(sc, xd, parts, trace=False):
    """Pushes xd through sc in `parts`, then flushes.  Returns (y, z, per-call
    output counts, per-push trace names)."""
    from dspcore import _lib
    ys, zs, counts, names = [], [], [], []
    at = 0
    for n in parts:
        if trace:
            _lib.trace_enable(True)
        y, z = sc.push(xd[:, at:at + n])
        if trace:
            names.append([k for k, _ in _lib.trace_read()])
            _lib.trace_enable(False)
        at += n
        assert z.shape[0] == xd.shape[0] and (y is None or y.shape == z.shape)
        counts.append(z.shape[1])
        ys.append(None if y is None else y.clone())
        zs.append(z.clone())
    y, z = sc.flush()
    counts.append(z.shape[1])
    ys.append(None if y is None else y.clone())
    zs.append(z.clone())
    ycat = None if ys[0] is None else torch.cat(ys, dim=1)
    return ycat, torch.cat(zs, dim=1), counts, names


@pytest.mark.parametrize("parts", list(PARTS))
@pytest.mark.parametrize("L,M,K", RATIOS)
def test_stream_chain_matches_one_shot_and_oracle(gpu, L, M, K, parts):
    from dspcore import design
    from dspcore.stream import StreamChain
    ref_y, ref_z, orc_y, orc_z = _one_shot(gpu, L, M, K)
    xd = torch.from_numpy(_chain_input()).to(gpu)
    sc = StreamChain(FS_IN, L, M, K, _gains(), 3, MAX_BLOCK, gpu)
    assert sc.fs_out == int(FS_IN * L / M)
    y, z, counts, names = _run_stream(sc, xd, PARTS[parts], trace=True)
    total = -(-N_IN * L // M)
    assert y.shape == z.shape == (3, total) and sum(counts) == total
    # per-push counts are the plan's; with L = M = 1 a block comes straight back
    if L == 1 and M == 1:
        assert counts == PARTS[parts] + [0] and sc.hist == 0 and sc.latency_in == 0
    else:
        plan = design.stream_src_plan(FS_IN, M, L, K)
        assert sc.hist == plan.hist and sc.latency_in == plan.c / L
        consumed = produced = 0
        for n, got in zip(PARTS[parts], counts):
            assert got == plan.block(consumed, produced, n)[2]
            consumed += n
            produced += got
        assert counts[-1] == plan.flush(consumed, produced)[2]
    if parts == "ragged" and not (L == 1 and M == 1):
        assert counts[0] == 0                    # one sample in: nothing computable yet
    # launches of a push: the stateful cascade once, never the one-shot cascade's kernels
    for got, push in zip(counts, names):
        assert not FORBIDDEN & set(push), push
        assert push.count("iir_stream") == (1 if got else 0), push
        assert push.count("src_poly") == (1 if got and not (L == 1 and M == 1) else 0), push
    y, z = y.cpu().numpy(), z.cpu().numpy()
    assert np.array_equal(y, ref_y), float(np.max(np.abs(y - ref_y)))     # bitwise
    ez = float(np.max(np.abs(z - ref_z)))
    ey = float(np.max(np.abs(y - orc_y)) / max(1.0, np.max(np.abs(orc_y))))
    eo = float(np.max(np.abs(z - orc_z)))
    print(f"{L}/{M} {parts}: z vs chain {ez:.3g}, y vs oracle {ey:.3g}, z vs oracle {eo:.3g}")
    assert ez <= CROSS_PATH
    assert ey <= SRC_ATOL
    assert eo <= EQ_ATOL


def test_flat_gains_bypass_the_eq(gpu):
    """Every |gain| < 0.1: z is y (the reference returns its input, no clip)."""
    from dspcore.stream import StreamChain
    flat = {k: 0.0 for k in _gains()}
    xd = torch.from_numpy(_chain_input()).to(gpu) * 3
    sc = StreamChain(FS_IN, 3, 2, None, flat, 3, MAX_BLOCK, gpu)
    y, z, _, names = _run_stream(sc, xd, PARTS["even"], trace=True)
    assert torch.equal(y, z) and float(z.abs().max()) > 1.0
    assert all("iir_stream" not in p for p in names)


def test_reset_checkpoint_and_keep_y(gpu):
    from dspcore.stream import StreamChain
    xd = torch.from_numpy(_chain_input()).to(gpu)
    parts = PARTS["ragged"]
    sc = StreamChain(FS_IN, 3, 2, None, _gains(), 3, MAX_BLOCK, gpu)
    y0, z0, counts0, _ = _run_stream(sc, xd, parts)
    with pytest.raises(RuntimeError):
        sc.push(xd[:, :10])                      # flushed
    sc.reset()
    y1, z1, counts1, _ = _run_stream(sc, xd, parts)
    assert torch.equal(y0, y1) and torch.equal(z0, z1) and counts0 == counts1
    # checkpoint after four pushes, continue in a fresh object
    sc.reset()
    at, head = 0, []
    for n in parts[:4]:
        head.append(sc.push(xd[:, at:at + n])[1].clone())
        at += n
    sd = sc.state_dict()
    assert sd["consumed"] == at and tuple(sd["history"].shape) == (3, sc.hist)
    other = StreamChain(FS_IN, 3, 2, None, _gains(), 3, MAX_BLOCK, gpu)
    other.load_state_dict(sd)
    _, tail, _, _ = _run_stream(other, xd[:, at:], parts[4:])
    assert torch.equal(torch.cat(head + [tail], dim=1), z0)
    with pytest.raises(ValueError):
        StreamChain(FS_IN, 1, 2, None, _gains(), 3, MAX_BLOCK, gpu).load_state_dict(sd)
    # keep_y=False: y is None, z the same
    lean = StreamChain(FS_IN, 3, 2, None, _gains(), 3, MAX_BLOCK, gpu, keep_y=False)
    yn, zn, _, _ = _run_stream(lean, xd, parts)
    assert yn is None and torch.equal(zn, z0)
    lean.reset()
    with pytest.raises(ValueError):
        lean.push(xd[:, :MAX_BLOCK + 1])
