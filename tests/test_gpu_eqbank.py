"""The EQ bank on the GPU (include/dspcore_eqbank.h): every row of a mixed
bank against the single-sos streaming cascade on that row alone.

Bounds.  Whenever the bank's chunk length T = 32 ceil(max_n / 2048) is the
single call's 32 ceil(n / 2048), the two kernels run the same instructions on
the same doubles (the shorter groups' identity stages pass their input through
exactly and add fma(0, finite, acc) terms to the scan), so y and the exit state
are compared with np.array_equal.  Outside that class the chunking differs and
the float64 results differ by rounding: the project's CROSS_PATH (2e-6)
between two paths of one recursion, EQ_ATOL (1e-5) and SRC_ATOL (2e-6) against
the oracle, as in tests/test_gpu_stream.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SRC_ATOL = 2e-6
EQ_ATOL = 1e-5
CROSS_PATH = 2e-6
FS_EQ = 72000
TWO = {"Bass": 6, "Presence": -3}
ONE = {"Low Mids": 4}
ROW_MAP = [0, 1, 2, 3, 1, 0, 2]
SENTINEL = 7.0
WIDTH = 16                      # state columns: 12 used by the six-band rows


def _settings():
    """The four groups: config 3's six bands, two bands, one band, all flat."""
    from oracle import dsp_ref_cpu as orc
    six = dict(orc.CONFIG3_GAINS)
    return [six, TWO, ONE, {k: 0.0 for k in six}]


def _row_gains(row_map=ROW_MAP):
    s = _settings()
    return [s[g] for g in row_map]


def _row_plans(row_map=ROW_MAP):
    """(sos, clip) per row, as design.eq_plan gives them."""
    from dspcore import design
    out = []
    for gains in _row_gains(row_map):
        p = design.eq_plan(FS_EQ, gains)
        out.append((np.ascontiguousarray(p.sos, dtype=np.float64).reshape(-1, 5), not p.bypass))
    return out


_DATA = {}


def _input(n):
    """[7, n] float32, row 1 loud enough to clip; [7, WIDTH] finite entry states."""
    if n not in _DATA:
        rng = np.random.default_rng(100 + n)
        x = rng.uniform(-1, 1, (len(ROW_MAP), n)).astype(np.float32)
        x[1] *= 8
        zi = rng.uniform(-2, 2, (len(ROW_MAP), WIDTH))
        _DATA[n] = (x, zi)
    return _DATA[n]


def _single(gpu, x, plans, zi):
    """Every row alone through ops.biquad_cascade_state with its own sos, clip
    and entry state: (y [R, n], [zf_r float64 [2 S_r]])."""
    from dspcore import ops
    ys, zfs = [], []
    for r, (sos, clip) in enumerate(plans):
        S = sos.shape[0]
        xr = torch.from_numpy(np.ascontiguousarray(x[r:r + 1])).to(gpu)
        zr = None
        if zi is not None and S:
            zr = torch.from_numpy(zi[r, :2 * S].copy()).to(gpu).reshape(1, -1)
        y, zf = ops.biquad_cascade_state(xr, sos, clip, zi=zr)
        ys.append(y.cpu().numpy()[0])
        zfs.append(zf.cpu().numpy()[0, :2 * S])
    return np.stack(ys), zfs


_REF = {}


def _reference(gpu, n):
    """The single-sos results for _input(n), computed once."""
    if n not in _REF:
        x, zi = _input(n)
        _REF[n] = _single(gpu, x, _row_plans(), zi)
    return _REF[n]


def _pitched(gpu, x, pitch, offset):
    """x in a device buffer of row pitch `pitch` elements that starts `offset`
    elements into its allocation (offset 1: rows off the 16-byte grid)."""
    R, n = x.shape
    flat = torch.zeros(R * pitch + offset, dtype=torch.float32, device=gpu)
    view = flat[offset:offset + R * pitch].view(R, pitch)[:, :n]
    view.copy_(torch.from_numpy(x))
    return view


def _check_rows(y, zf, ref_y, ref_zf, plans, zi_in):
    for r, (sos, _) in enumerate(plans):
        D = 2 * sos.shape[0]
        assert np.array_equal(y[r], ref_y[r]), (r, float(np.nanmax(np.abs(y[r] - ref_y[r]))))
        assert np.array_equal(zf[r, :D], ref_zf[r]), r
        assert np.array_equal(zf[r, D:], zi_in[r, D:]), r      # past 2 S_g: left alone


def _bank(gpu, max_n, row_map=ROW_MAP):
    from dspcore.eqbank import EqBank
    return EqBank(FS_EQ, _row_gains(row_map), max_n, gpu)


def _run_bitwise(gpu, bank, n):
    x, zi = _input(n)
    plans = _row_plans()
    ref_y, ref_zf = _reference(gpu, n)
    zi_s = zi.copy()
    zi_s[:, 12:] = SENTINEL
    zid = torch.from_numpy(zi_s).to(gpu)
    # row pitch n + 1 from an odd element (scalar loads and stores), and a
    # multiple of 4 on the 16-byte grid (vector path)
    for pitch, offset in ((n + 1, 1), (-(-n // 4) * 4 + 4, 0)):
        xd = _pitched(gpu, x, pitch, offset)
        out = _pitched(gpu, np.zeros_like(x), pitch, offset)
        zf = torch.full((len(ROW_MAP), WIDTH), SENTINEL, dtype=torch.float64, device=gpu)
        y, got = bank.apply(xd, zi=zid, out=out, zf=zf)
        assert y is out and got is zf
        _check_rows(y.cpu().numpy(), zf.cpu().numpy(), ref_y, ref_zf, plans,
                    np.full_like(zi_s, SENTINEL))
        assert torch.equal(xd.cpu(), torch.from_numpy(x))        # the input is not written
        # in place: x is out, zi is zf
        state = zid.clone()
        y2, _ = bank.apply(xd, zi=state, out=xd, zf=state)
        assert y2 is xd
        _check_rows(xd.cpu().numpy(), state.cpu().numpy(), ref_y, ref_zf, plans, zi_s)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 2047, 2048])
def test_rows_are_bitwise_the_single_sos_cascade(gpu, n):
    bank = _bank(gpu, 2048)
    assert bank.G == 4 and bank.max_stages == 6 and bank.row_group.cpu().tolist() == ROW_MAP
    _run_bitwise(gpu, bank, n)


@pytest.mark.parametrize("n", [2049, 4096])
def test_second_chunk_class_is_bitwise_too(gpu, n):
    _run_bitwise(gpu, _bank(gpu, 4096), n)


def test_outside_the_chunk_class_within_the_project_bounds(gpu):
    """max_n = 4096 (T = 64) and n = 100: the single call cuts 32-sample chunks."""
    from oracle import dsp_ref_cpu as orc
    n = 100
    x, _ = _input(n)
    plans = _row_plans()
    y, zf = _bank(gpu, 4096).apply(torch.from_numpy(x).to(gpu))
    y = y.cpu().numpy()
    ref_y, _ = _single(gpu, x, plans, None)
    for r, gains in enumerate(_row_gains()):
        want = orc.equaliser(x[r].astype(np.float64), FS_EQ, gains)
        eo = float(np.max(np.abs(y[r] - want)))
        ec = float(np.max(np.abs(y[r] - ref_y[r])))
        print(f"row {r}: vs oracle {eo:.3g}, vs single-sos {ec:.3g}")
        assert eo <= EQ_ATOL
        assert ec <= CROSS_PATH
    assert tuple(zf.shape) == (len(ROW_MAP), 12)


def test_rows_do_not_depend_on_the_batch(gpu):
    """B = 1 banks (instantiated for the row's own stage count), the rows in
    reverse order, and the groups renumbered: the same rows, bitwise."""
    from dspcore.eqbank import EqBank
    n = 2047
    x, zi = _input(n)
    plans = _row_plans()
    ref_y, ref_zf = _reference(gpu, n)
    zid = torch.from_numpy(zi).to(gpu)
    for r in range(len(ROW_MAP)):
        one = EqBank(FS_EQ, [_row_gains()[r]], 2048, gpu)
        D = 2 * plans[r][0].shape[0]
        y, zf = one.apply(torch.from_numpy(x[r:r + 1].copy()).to(gpu),
                          zi=zid[r, :max(D, 1)].clone().reshape(1, -1))
        assert one.max_stages == plans[r][0].shape[0]
        assert np.array_equal(y.cpu().numpy()[0], ref_y[r]), r
        assert np.array_equal(zf.cpu().numpy()[0, :D], ref_zf[r]), r
    rev = list(reversed(range(len(ROW_MAP))))
    bank = _bank(gpu, 2048, [ROW_MAP[r] for r in rev])
    assert bank.row_group.cpu().tolist() == [0, 1, 2, 3, 0, 2, 1]     # groups in order of first use
    state = zid[rev].contiguous()
    y, _ = bank.apply(torch.from_numpy(x[rev].copy()).to(gpu), zi=state, zf=state)
    _check_rows(y.cpu().numpy()[rev], state.cpu().numpy()[rev], ref_y, ref_zf, plans, zi)
    # the same cascades under other group numbers
    order = [3, 0, 2, 1]                                          # new index -> old group
    groups = [_row_plans(list(range(4)))[g] for g in order]
    renum = EqBank.from_sos([s for s, _ in groups], [c for _, c in groups],
                            [order.index(g) for g in ROW_MAP], 2048, gpu)
    state = zid.clone()
    y, _ = renum.apply(torch.from_numpy(x).to(gpu), zi=state, zf=state)
    _check_rows(y.cpu().numpy(), state.cpu().numpy(), ref_y, ref_zf, plans, zi)
    with pytest.raises(ValueError):
        renum.apply(torch.from_numpy(x[:3].copy()).to(gpu))       # three rows for seven gain sets
    with pytest.raises(ValueError):
        renum.apply(torch.zeros((len(ROW_MAP), 2049), dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        renum.apply(torch.from_numpy(x).to(gpu), zf=torch.zeros((7, 11), dtype=torch.float64,
                                                                 device=gpu))


def test_blocks_continue_bitwise(gpu):
    """Blocks [1, 700, 2048, 37], zf fed to zi, against the single-sos kernel
    fed the same blocks (every n is in max_n = 2048's chunk class)."""
    from dspcore import ops
    blocks = [1, 700, 2048, 37]
    total = sum(blocks)
    x = np.random.default_rng(7).uniform(-1, 1, (len(ROW_MAP), total)).astype(np.float32)
    x[1] *= 8
    plans = _row_plans()
    bank = _bank(gpu, 2048)
    xd = torch.from_numpy(x).to(gpu)
    z = torch.empty_like(xd)
    state = torch.zeros((len(ROW_MAP), 12), dtype=torch.float64, device=gpu)
    at = 0
    for nb in blocks:
        bank.apply(xd[:, at:at + nb], zi=state, out=z[:, at:at + nb], zf=state)
        at += nb
    z, state = z.cpu().numpy(), state.cpu().numpy()
    for r, (sos, clip) in enumerate(plans):
        S = sos.shape[0]
        xr = xd[r:r + 1].contiguous()
        zr = torch.empty_like(xr)
        st = torch.zeros((1, max(2 * S, 1)), dtype=torch.float64, device=gpu)
        at = 0
        for nb in blocks:
            ops.biquad_cascade_state(xr[:, at:at + nb], sos, clip, zi=st if S else None,
                                     out=zr[:, at:at + nb], zf=st)
            at += nb
        assert np.array_equal(z[r], zr.cpu().numpy()[0]), r
        assert np.array_equal(state[r, :2 * S], st.cpu().numpy()[0, :2 * S]), r
        assert not state[r, 2 * S:].any(), r
    assert np.max(np.abs(z[1])) == 1.0                             # the loud row clips


def test_nonfinite_rows_match_the_single_call_and_stay_in_their_row(gpu):
    n = 200
    clean = np.random.default_rng(8).uniform(-0.9, 0.9, (len(ROW_MAP), n)).astype(np.float32)
    clean[3] *= 3                                                  # the bypass row is not clipped
    x = clean.copy()
    x[1, 40] = np.inf                                              # a two-band row
    x[3, 40] = np.nan                                              # the bypass row
    plans = _row_plans()
    bank = _bank(gpu, 2048)
    y, zf = bank.apply(torch.from_numpy(x).to(gpu))
    yc, zfc = bank.apply(torch.from_numpy(clean).to(gpu))
    y, zf, yc, zfc = (t.cpu().numpy() for t in (y, zf, yc, zfc))
    ref_y, ref_zf = _single(gpu, x, plans, None)
    for r in (1, 3):
        D = 2 * plans[r][0].shape[0]
        assert np.array_equal(y[r], ref_y[r], equal_nan=True), r
        assert np.array_equal(zf[r, :D], ref_zf[r], equal_nan=True), r
    assert np.isfinite(y[1, :40]).all() and np.isnan(y[1, 41:]).all() and np.isnan(zf[1, :4]).all()
    assert not zf[1, 4:].any()
    # the bypass row comes back bit for bit, its state row untouched
    assert np.array_equal(y[3].view(np.uint32), x[3].view(np.uint32)) and not zf[3].any()
    for r in (0, 2, 4, 5, 6):
        assert np.array_equal(y[r], yc[r]) and np.array_equal(zf[r], zfc[r]), r
        assert np.isfinite(y[r]).all() and np.isfinite(zf[r]).all()
    # an inf passes the bypass too
    x[3, 41] = -np.inf
    y2 = bank.apply(torch.from_numpy(x).to(gpu))[0].cpu().numpy()
    assert np.array_equal(y2[3].view(np.uint32), x[3].view(np.uint32))


def test_one_launch_per_call(gpu):
    """The padded design: one launch for the mixed bank (include/dspcore_eqbank.h)."""
    from dspcore import _lib
    x, zi = _input(2047)
    bank = _bank(gpu, 2048)
    xd, zid = torch.from_numpy(x).to(gpu), torch.from_numpy(zi).to(gpu)
    _lib.trace_enable(True)
    try:
        bank.apply(xd, zi=zid, zf=torch.empty_like(zid))
        names = [k for k, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    assert names == ["iir_bank"]


# ---------------------------------------------------------------------------
# StreamChain with one gains dict per channel
# ---------------------------------------------------------------------------
FS_IN = 48000


def _stream_gains():
    s = _settings()
    return [s[0], {"Bass": 6}, s[3]]


def _push_all(sc, xd, parts):
    ys, zs = [], []
    at = 0
    for n in parts:
        y, z = sc.push(xd[:, at:at + n])
        at += n
        ys.append(y.clone())
        zs.append(z.clone())
    return ys, zs


def _finish(sc, ys, zs):
    y, z = sc.flush()
    return torch.cat(ys + [y.clone()], dim=1), torch.cat(zs + [z.clone()], dim=1)


def test_stream_chain_per_channel_gains_bitwise(gpu):
    from dspcore import _lib
    from dspcore.stream import StreamChain
    parts = [1, 700, 0, 1024, 37]
    x = np.random.default_rng(9).uniform(-1, 1, (3, sum(parts))).astype(np.float32)
    x[1] *= 4
    xd = torch.from_numpy(x).to(gpu)
    gains = _stream_gains()
    sc = StreamChain(FS_IN, 3, 2, None, gains, 3, 1024, gpu)
    assert sc.bank is not None and sc.bank.G == 3 and sc.bank.max_n <= 2048
    assert tuple(sc._state.shape) == (3, 12)
    _lib.trace_enable(True)
    try:
        ys, zs = _push_all(sc, xd, parts)
        names = [k for k, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    assert names.count("iir_bank") == 3 and "iir_stream" not in names   # pushes 2, 4, 5 produce
    y, z = _finish(sc, ys, zs)
    total = -(-sum(parts) * 3 // 2)
    assert tuple(y.shape) == tuple(z.shape) == (3, total)
    # y: the single-gains StreamChain's; z: each channel's own single-gains stream
    ref = StreamChain(FS_IN, 3, 2, None, gains[0], 3, 1024, gpu)
    ry, _ = _finish(ref, *_push_all(ref, xd, parts))
    assert torch.equal(y, ry)
    for c in range(3):
        one = StreamChain(FS_IN, 3, 2, None, gains[c], 1, 1024, gpu)
        xc = xd[c:c + 1].contiguous()
        _, rz = _finish(one, *_push_all(one, xc, parts))
        assert torch.equal(z[c], rz[0]), c
    assert torch.equal(z[2], y[2]) and float(z[1].abs().max()) == 1.0   # bypass row: z = y
    # checkpoint after three pushes, continue in a fresh object; reset replays
    sc.reset()
    ys, zs = _push_all(sc, xd, parts[:3])
    sd = sc.state_dict()
    assert tuple(sd["eq_state"].shape) == (3, 12)
    other = StreamChain(FS_IN, 3, 2, None, gains, 3, 1024, gpu)
    other.load_state_dict(sd)
    at = sum(parts[:3])
    ys2, zs2 = _push_all(other, xd[:, at:], parts[3:])
    y2, z2 = _finish(other, ys + ys2, zs + zs2)
    assert torch.equal(y2, y) and torch.equal(z2, z)
    with pytest.raises(ValueError):
        StreamChain(FS_IN, 3, 2, None, gains[:2], 3, 1024, gpu)          # two dicts, three channels


def test_stream_chain_per_channel_gains_against_the_oracle(gpu):
    """max_block = 2048: max_out > 2048, the bank cuts 64-sample chunks."""
    from dspcore.stream import StreamChain
    from oracle import dsp_ref_cpu as orc
    parts = [2048, 2, 700, 2048]
    x = np.random.default_rng(10).uniform(-1, 1, (3, sum(parts))).astype(np.float32)
    gains = _stream_gains()
    sc = StreamChain(FS_IN, 3, 2, None, gains, 3, 2048, gpu)
    assert sc.bank.max_n > 2048
    xd = torch.from_numpy(x).to(gpu)
    y, z = _finish(sc, *_push_all(sc, xd, parts))
    y, z = y.cpu().numpy(), z.cpu().numpy()
    for c in range(3):
        ry, rz, _, _, _ = orc.chain(x[c].astype(np.float64), FS_IN, 3, 2, gains[c], None, 256)
        ey = float(np.max(np.abs(y[c] - ry)) / max(1.0, np.max(np.abs(ry))))
        ez = float(np.max(np.abs(z[c] - rz)))
        print(f"channel {c}: y vs oracle {ey:.3g}, z vs oracle {ez:.3g}")
        assert ey <= SRC_ATOL
        assert ez <= EQ_ATOL
