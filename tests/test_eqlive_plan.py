"""The live EQ without a GPU (include/dspcore_eqlive.h): the host model against
the oracle, the slot planning of dspcore.design and dspcore.eqlive, the
argument checks of the two entry points and the numbers in a built record."""
import re

import numpy as np
import pytest

import eqlive_model as model
from conftest import golden, golden_gains
from dspcore import _lib, design, eqlive

FS = 72000
SIX = {"Sub-Bass": 6, "Bass": -4, "Low Mids": 3, "High Mids": -3, "Presence": 5, "Brilliance": -6}
FLAT = {k: 0.0 for k in SIX}
REC = _lib.DSP_EQLIVE_RECORD_BYTES


def _record_dtype():
    """numpy mirror of csrc/iir_live.hip's LiveRecord (C layout)."""
    return np.dtype([("c", "<f8", (8, 5)), ("clip", "<i4"), ("copy", "<i4"), ("inst", "<i4"),
                     ("slots", "<i4"), ("T", "<i8"), ("P", "<f8", (16, 16)),
                     ("pad", "u1", (REC - 2392,))])


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def test_model_with_constant_gains_is_the_oracle_bitwise():
    """Every eq.npz case, the signal cut at 1, 1000 and n - 1: the flat slots
    pass their input exactly and lfilter's zi continues the recursion, so the
    float64 result is sistema_ecualizador's to the last bit."""
    from oracle import dsp_ref_cpu as orc
    g = golden("eq")
    for i in range(10):
        gains, fs = golden_gains(g[f"gains_{i}"]), int(g[f"fs_{i}"])
        if not gains:
            continue                                  # no slot: not a live EQ
        for src, key in (("x64", "z64"), ("x32", "z32")):
            x = g[src]
            want = np.asarray(orc.equaliser(x, fs, gains))
            assert np.array_equal(want, g[f"{key}_{i}"])
            for cut in (None, 1, 1000, x.size - 1):
                ch = model.ChannelModel(len(gains))
                parts = [x] if cut is None else [x[:cut], x[cut:]]
                got = np.concatenate([ch.block(fs, gains, p)[1] for p in parts])
                assert np.array_equal(got, want), (i, src, cut)


def test_flat_slot_at_rest_returns_its_input_bitwise():
    x = np.random.default_rng(0).uniform(-3, 3, 5000).astype(np.float32)
    for fs in (352800, 44100, 5512):
        ch = model.ChannelModel(6)
        z, v = ch.block(fs, FLAT, x)
        assert np.array_equal(z.view(np.uint32), x.view(np.uint32)) and not ch.zi.any()
        for b, a in model.slot_coefficients(fs, FLAT):
            assert np.array_equal(b, a) and b[0] == 1.0
        sos, clip = design.live_sos(fs, design.live_slots(fs, FLAT.keys()), FLAT)
        assert np.array_equal(sos[:, 1:3], sos[:, 3:5]) and (sos[:, 0] == 1.0).all() and not clip


# ---------------------------------------------------------------------------
# slot planning
# ---------------------------------------------------------------------------
def test_slots_keys_centres_and_flags():
    slots = design.live_slots(FS, SIX.keys())
    assert slots.keys == tuple(SIX) and slots.fc == (40, 150, 1000, 3000, 5000, 10000)
    assert slots.never == (False,) * 6
    # unknown name -> 1000 Hz
    assert design.live_slots(FS, ["Mystery", "Bass"]).fc == (1000, 150)
    # the clamp at fs = 5512: everything at or above 0.45 fs sits there
    low = design.live_slots(5512, SIX.keys())
    assert low.fc == (40, 150, 1000, 0.45 * 5512, 0.45 * 5512, 0.45 * 5512)
    assert low.fc == tuple(model.slot_centres(5512, SIX.keys()))
    # fc <= 10 Hz is never active, whatever its gain
    tiny = design.live_slots(20, ["Bass"])
    assert tiny.never == (True,) and design.live_active(tiny, {"Bass": 12}) == (False,)
    sos, clip = design.live_sos(20, tiny, {"Bass": 12})
    assert np.array_equal(sos[0, 1:3], sos[0, 3:5]) and sos[0, 0] == 1.0 and clip
    with pytest.raises(ValueError):
        design.live_slots(FS, [])
    with pytest.raises(ValueError):
        design.live_slots(FS, [f"b{i}" for i in range(9)])
    assert len(design.live_slots(FS, [f"b{i}" for i in range(8)]).keys) == 8
    # key order and key set
    for bad in (dict(reversed(list(SIX.items()))), {k: 1.0 for k in list(SIX)[:5]},
                dict(SIX, Air=1.0), {}):
        with pytest.raises(ValueError, match="band slots"):
            design.live_sos(FS, slots, bad)
    # g = 0.1 exactly: flat, but the reference clips
    edge = dict(FLAT, Bass=0.1)
    sos, clip = design.live_sos(FS, slots, edge)
    assert design.live_active(slots, edge) == (False,) * 6 and clip
    assert np.array_equal(sos, design.live_sos(FS, slots, FLAT)[0])
    # the active sections are the reference's designs, the same doubles as eq_plan's
    sos, clip = design.live_sos(FS, slots, SIX)
    assert clip and np.array_equal(sos, design.eq_plan(FS, SIX).sos)
    for (b, a), row in zip(model.slot_coefficients(FS, dict(SIX, Bass=0.05)),
                           design.live_sos(FS, slots, dict(SIX, Bass=0.05))[0]):
        assert np.array_equal(row, [b[0], b[1], b[2], a[1], a[2]])


def test_planner_groups_and_tracks_activity():
    hot = dict(FLAT, Bass=6.0)
    gains = [SIX, FLAT, dict(SIX), hot, FLAT, dict(FLAT, Bass=0.1)]
    pl = eqlive.LivePlanner(FS, gains)
    assert pl.B == 6 and pl.max_groups == 6 and pl.n_slots == 6
    plan = pl.plan(gains)
    assert plan.G == 4 and plan.row_group.dtype == np.int32
    assert list(plan.row_group) == [0, 1, 0, 2, 1, 3]            # groups in order of first use
    assert list(plan.clip) == [1, 0, 1, 1] and list(plan.copy) == [0, 1, 0, 1]
    assert list(pl.ever_active) == [True, False, True, True, False, False]
    assert plan.sos.shape == (4, 6, 5)
    # a row that was active stays in the cascade when its gains go flat; the
    # flat row that never was stays a copy: two groups of the same sections
    pl.commit(pl.plan([FLAT] * 6), [FLAT] * 6)
    plan = pl.plan([FLAT] * 6)
    assert plan.G == 2 and list(plan.row_group) == [0, 1, 0, 0, 1, 1]
    assert list(plan.copy) == [0, 1] and np.array_equal(plan.sos[0], plan.sos[1])
    assert list(pl.ever_active) == [True, False, True, True, False, False]
    # activity survives further changes, a new one is recorded
    later = [FLAT, hot, FLAT, FLAT, FLAT, FLAT]
    pl.commit(pl.plan(later), later)
    assert list(pl.ever_active) == [True, True, True, True, False, False]
    # reset: only what the current gains make active
    plan = pl.reset()
    assert list(pl.ever_active) == [False, True, False, False, False, False]
    assert list(plan.copy[plan.row_group]) == [1, 0, 1, 1, 1, 1]
    # one dict serves every row
    one = eqlive.LivePlanner(FS, SIX, batch=5)
    assert one.plan(SIX).G == 1 and one.max_groups == 5 and one.ever_active.all()
    assert eqlive.LivePlanner(FS, [SIX] * 300).max_groups == 256


def test_planner_errors_change_nothing():
    gains = [SIX, FLAT, FLAT]
    pl = eqlive.LivePlanner(FS, gains, max_groups=2)
    before = (pl.ever_active.copy(), [dict(g) for g in pl.gains])
    three = [SIX, dict(FLAT, Bass=3.0), dict(FLAT, Bass=4.0)]
    with pytest.raises(ValueError, match="max_groups"):
        pl.plan(three)                                         # raised by the pure planning step
    with pytest.raises(ValueError, match="band slots"):
        pl.plan([SIX, FLAT, dict(reversed(list(FLAT.items())))])
    with pytest.raises(ValueError, match="2 gain sets for 3"):
        pl.plan([SIX, FLAT])
    assert np.array_equal(pl.ever_active, before[0]) and pl.gains == before[1]
    with pytest.raises(ValueError, match="max_groups"):
        eqlive.LivePlanner(FS, three, max_groups=2)
    with pytest.raises(ValueError, match="max_groups"):
        eqlive.LiveEq(FS, three, 2048, max_groups=2)           # before any GPU work
    with pytest.raises(ValueError):
        eqlive.LiveEq(FS, SIX, 0)                              # max_n < 1
    with pytest.raises(ValueError):
        eqlive.LivePlanner(FS, [])
    with pytest.raises(ValueError):
        eqlive.LivePlanner(FS, {f"b{i}": 1.0 for i in range(9)})


# ---------------------------------------------------------------------------
# the C ABI, host side
# ---------------------------------------------------------------------------
def _build(sos, clip, copy, G, slots, max_n, nbytes=None, null=()):
    lib = _lib.load()
    nbytes = int(lib.dsp_eqlive_bytes(max(G, 1))) if nbytes is None else nbytes
    buf = np.zeros(max(nbytes, 1), dtype=np.uint8)
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    clip = np.asarray(clip, dtype=np.int32)
    copy = np.asarray(copy, dtype=np.int32)
    rc = lib.dsp_eqlive_build(None if "table" in null else buf.ctypes.data, nbytes,
                              None if "sos" in null else sos.ctypes.data_as(_lib._dp),
                              None if "clip" in null else clip.ctypes.data,
                              None if "copy" in null else copy.ctypes.data, G, slots, max_n)
    return rc, buf


def test_version_exports_and_signatures():
    lib = _lib.load()
    assert lib.dsp_eqlive_version() == 10000
    with open(_lib.EQLIVE_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|size_t) (dsp_eqlive_[a-z0-9_]+)\(", text, flags=re.M))
    assert declared == {"dsp_eqlive_version", "dsp_eqlive_bytes", "dsp_eqlive_build",
                        "dsp_eqlive_cascade_f32"}
    for name in _lib.header_symbols(_lib.EQLIVE_HEADER_PATH):
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"
    assert "lfilter" in text and "imported from and exported" in text
    assert _lib.DSP_EQLIVE_MAX_SLOTS == design.MAX_LIVE_SLOTS == 8
    assert lib.dsp_eqlive_bytes(1) == REC == _record_dtype().itemsize and REC % 256 == 0
    assert lib.dsp_eqlive_bytes(7) == 7 * REC
    assert lib.dsp_eqlive_bytes(0) == 0 and lib.dsp_eqlive_bytes(-3) == 0
    # the other headers keep their symbols and versions
    assert len(_lib.header_symbols()) == 35
    assert (lib.dsp_version(), lib.dsp_stream_version(), lib.dsp_eqbank_version()) == \
        (20700, 10000, 10000)


def test_build_rejects_bad_arguments_without_a_gpu():
    ident = np.tile([1.0, 0, 0, 0, 0], (2, 8, 1))
    ok = ([1, 0], [0, 1], 2, 8, 2048)
    assert _build(ident, *ok)[0] == 0
    assert _build(ident, *ok, nbytes=2 * REC - 1)[0] == _lib.DSP_EINVAL
    assert "bytes" in _lib.last_error()
    assert _build(ident, [1, 0], [0, 1], 0, 8, 2048)[0] == _lib.DSP_EINVAL      # G < 1
    assert _build(ident, [1, 0], [0, 1], -1, 8, 2048)[0] == _lib.DSP_EINVAL
    assert _build(ident, [1, 0], [0, 1], 2, 0, 2048)[0] == _lib.DSP_EINVAL      # slots < 1
    assert _build(ident, [1, 0], [0, 1], 2, 9, 2048)[0] == _lib.DSP_ENOTSUP     # slots > 8
    assert "slots" in _lib.last_error()
    assert _build(ident, *ok[:4], 0)[0] == _lib.DSP_EINVAL                      # max_n
    assert _build(ident, *ok[:4], (1 << 30) + 1)[0] == _lib.DSP_EINVAL
    for which in ("table", "sos", "clip", "copy"):
        assert _build(ident, *ok, null=(which,))[0] == _lib.DSP_EINVAL, which
        assert "null" in _lib.last_error()
    zero = ident.copy()
    zero[1, 0] = [0.0, 0.7, 0.2, -0.5, 0.25]                                    # b0 == 0 is allowed
    rc, buf = _build(zero, *ok)
    assert rc == 0
    assert list(buf.view(_record_dtype())["c"][1, 0]) == [0.0, 0.7, 0.2, -0.5, 0.25]


def test_cascade_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    table, bytes3 = 4096, 3 * REC

    def call(B=2, n=100, ld_x=100, ld_y=100, table=table, nbytes=bytes3, G=3, S=6, max_n=2048,
             rows=64, ld_state=12, x=64, y=64):
        return lib.dsp_eqlive_cascade_f32(x, y, B, n, ld_x, ld_y, table, nbytes, G, S, max_n, rows,
                                          None, None, ld_state, None)

    assert call(B=0) == 0 and call(n=0) == 0              # no-ops launch nothing
    assert call(B=0, x=None, y=None, table=None, rows=None) == 0
    assert call(n=2049) == _lib.DSP_EINVAL and "max_n" in _lib.last_error()
    assert call(n=2049, ld_x=4096, ld_y=4096, max_n=4096, B=0) == 0
    assert call(ld_state=11) == _lib.DSP_EINVAL and "ld_state" in _lib.last_error()
    assert call(ld_x=99) == _lib.DSP_EINVAL and call(ld_y=99) == _lib.DSP_EINVAL
    assert call(B=-1) == _lib.DSP_EINVAL and call(n=-1) == _lib.DSP_EINVAL
    assert call(G=0) == _lib.DSP_EINVAL
    assert call(S=9, ld_state=18) == _lib.DSP_EINVAL and call(S=0) == _lib.DSP_EINVAL
    assert call(max_n=0, n=0) == _lib.DSP_EINVAL
    assert call(nbytes=bytes3 - 1) == _lib.DSP_EINVAL and "bytes" in _lib.last_error()
    assert call(table=4096 + 128) == _lib.DSP_EINVAL and "aligned" in _lib.last_error()
    for which in ("x", "y", "table", "rows"):
        assert call(**{which: None}) == _lib.DSP_EINVAL, which
        assert "null" in _lib.last_error()


def _one_step(c):
    """A [2S][2S] of the record's step function (csrc/iir_live.hip), rows
    {b0, d1, d2, a1, a2}: y = b0 u + s1, s1' = d1 u + s2 - a1 s1, s2' = d2 u -
    a2 s1, stage k's u the previous stage's y."""
    S = c.shape[0]
    A = np.zeros((2 * S, 2 * S))
    for col in range(2 * S):
        X = np.zeros(2 * S)
        X[col] = 1.0
        u = 0.0
        for k in range(S):
            b0, d1, d2, a1, a2 = c[k]
            s1, s2 = X[2 * k], X[2 * k + 1]
            y = b0 * u + s1
            X[2 * k], X[2 * k + 1] = d1 * u + (s2 - a1 * s1), d2 * u - a2 * s1
            u = y
        A[:, col] = X
    return A


def test_records_hold_the_d_form_and_the_chunk_transition():
    hot = dict(FLAT, Bass=6.0, Presence=-15.0)
    pl = eqlive.LivePlanner(FS, [SIX, FLAT, hot, dict(FLAT, Bass=0.1)])
    plan = pl.plan(pl.gains)
    for max_n, T in ((1, 32), (2048, 32), (2049, 64), (100000, 32 * 49)):
        rec = eqlive.build_table(plan, max_n).view(_record_dtype())
        assert rec.shape == (4,) and list(rec["T"]) == [T] * 4
        assert list(rec["inst"]) == [6] * 4 and list(rec["slots"]) == [6] * 4
        assert list(rec["clip"]) == [1, 0, 1, 1] and list(rec["copy"]) == [0, 1, 0, 1]
        assert not rec["pad"].any()
        for g in range(4):
            sos = plan.sos[g]
            c = rec["c"][g]
            np.testing.assert_array_equal(c[:6, 0], sos[:, 0])
            np.testing.assert_array_equal(c[:6, 3:], sos[:, 3:])
            np.testing.assert_array_equal(c[:6, 1], sos[:, 1] - sos[:, 3] * sos[:, 0])
            np.testing.assert_array_equal(c[:6, 2], sos[:, 2] - sos[:, 4] * sos[:, 0])
            np.testing.assert_array_equal(c[6:], np.tile([1.0, 0, 0, 0, 0], (2, 1)))
            flat = [k for k in range(6) if np.array_equal(sos[k, 1:3], sos[k, 3:5])]
            assert len(flat) == (0, 6, 4, 6)[g]
            for k in flat:                                     # a flat slot: exactly zero
                assert c[k, 0] == 1.0 and c[k, 1] == 0.0 and c[k, 2] == 0.0
            want = np.linalg.matrix_power(_one_step(c[:6]), T)
            P = rec["P"][g]
            assert np.max(np.abs(P[:12, :12] - want)) <= 1e-12 * np.max(np.abs(want)), (max_n, g)
            assert not P[12:].any() and not P[:, 12:].any()
    # the unused records of a larger buffer stay zero (T == 0 matches no call)
    big = eqlive.build_table(plan, 2048, 7).view(_record_dtype())
    assert big.shape == (7,) and not big[4:].view(np.uint8).any()
    with pytest.raises(ValueError):
        eqlive.build_table(plan, 2048, 3)
    # seven slots run as eight: the eighth section passes its input through
    seven = dict(SIX, Air=2.5)
    p7 = eqlive.LivePlanner(FS, seven)
    rec7 = eqlive.build_table(p7.plan(seven), 2048).view(_record_dtype())
    assert list(rec7["inst"]) == [8] and list(rec7["slots"]) == [7]
    want = np.linalg.matrix_power(_one_step(rec7["c"][0]), 32)
    assert np.max(np.abs(rec7["P"][0] - want)) <= 1e-12 * np.max(np.abs(want))
    assert not rec7["P"][0][:14, 14:].any()                    # nothing reads the eighth's state

