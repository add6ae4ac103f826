"""The EQ bank without a GPU (include/dspcore_eqbank.h): the header's names
are exported and bound, dsp_eqbank_build and dsp_eqbank_cascade_f32 validate
their arguments before any device work, the built records hold the numbers
the single-sos call computes, and the Python planner merges identical plans."""
import re

import numpy as np
import pytest

from dspcore import _lib, design, eqbank

FS = 72000
SIX = {"Sub-Bass": 6, "Bass": -4, "Low Mids": 3, "High Mids": -3, "Presence": 5, "Brilliance": -6}
TWO = {"Bass": 6, "Presence": -3}
ONE = {"Low Mids": 4}
FLAT = {k: 0.0 for k in SIX}
REC = _lib.DSP_EQBANK_RECORD_BYTES


def _record_dtype():
    """numpy mirror of csrc/iir_bank.hip's BankRecord (C layout)."""
    return np.dtype([("c", "<f8", (16, 5)), ("G", "<f8"), ("stages", "<i4"), ("clip", "<i4"),
                     ("inst", "<i4"), ("max_stages", "<i4"), ("T", "<i8"), ("P", "<f8", (16, 16)),
                     ("pad", "u1", (REC - 2720,))])


def _build(sos, stages, clip, G, ld, max_n, nbytes=None, null=()):
    lib = _lib.load()
    nbytes = int(lib.dsp_eqbank_bytes(max(G, 1))) if nbytes is None else nbytes
    buf = np.zeros(max(nbytes, 1), dtype=np.uint8)
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    stages = np.asarray(stages, dtype=np.int32)
    clip = np.asarray(clip, dtype=np.int32)
    rc = lib.dsp_eqbank_build(None if "bank" in null else buf.ctypes.data, nbytes,
                              None if "sos" in null else sos.ctypes.data_as(_lib._dp),
                              None if "stages" in null else stages.ctypes.data,
                              None if "clip" in null else clip.ctypes.data, G, ld, max_n)
    return rc, buf


def test_version_exports_and_signatures():
    lib = _lib.load()
    assert lib.dsp_eqbank_version() == 10000
    with open(_lib.EQBANK_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^(?:int|size_t) (dsp_eqbank_[a-z0-9_]+)\(", text, flags=re.M))
    assert declared == {"dsp_eqbank_version", "dsp_eqbank_bytes", "dsp_eqbank_build",
                        "dsp_eqbank_cascade_f32"}
    for name in _lib.header_symbols(_lib.EQBANK_HEADER_PATH):
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"
    assert _lib.DSP_EQBANK_MAX_STAGES == 8
    assert lib.dsp_eqbank_bytes(1) == REC == _record_dtype().itemsize and REC % 256 == 0
    assert lib.dsp_eqbank_bytes(5) == 5 * REC
    assert lib.dsp_eqbank_bytes(0) == 0 and lib.dsp_eqbank_bytes(-3) == 0


def test_the_other_headers_are_unchanged():
    assert len(_lib.header_symbols()) == 35
    assert _lib.load().dsp_version() == 20700 and _lib.load().dsp_stream_version() == 10000
    for path in (_lib.HEADER_PATH, _lib.STREAM_HEADER_PATH):
        with open(path) as f:
            assert "eqbank" not in f.read()


def test_build_rejects_bad_arguments_without_a_gpu():
    ident = np.tile([1.0, 0, 0, 0, 0], (2, 9, 1))
    ok = ([2, 1], [1, 0], 2, 9, 2048)
    assert _build(ident, *ok)[0] == 0
    assert _build(ident, *ok, nbytes=2 * REC - 1)[0] == _lib.DSP_EINVAL        # short buffer
    assert "bank_bytes" in _lib.last_error()
    assert _build(ident, [2, 1], [1, 0], 0, 9, 2048)[0] == _lib.DSP_EINVAL      # G < 1
    assert _build(ident, [2, 1], [1, 0], -1, 9, 2048)[0] == _lib.DSP_EINVAL
    assert _build(ident, [2, -1], [1, 0], 2, 9, 2048)[0] == _lib.DSP_EINVAL     # stages < 0
    assert _build(ident, [2, 9], [1, 0], 2, 9, 2048)[0] == _lib.DSP_ENOTSUP     # stages > 8
    assert "stages" in _lib.last_error()
    assert _build(ident[:, :4], [2, 5], [1, 0], 2, 4, 2048)[0] == _lib.DSP_EINVAL   # > ld_stages
    assert _build(ident, *ok[:4], 0)[0] == _lib.DSP_EINVAL                      # max_n < 1
    assert _build(ident, *ok[:4], -7)[0] == _lib.DSP_EINVAL
    assert _build(ident, *ok[:4], (1 << 30) + 1)[0] == _lib.DSP_EINVAL
    for which in ("bank", "sos", "stages", "clip"):
        assert _build(ident, *ok, null=(which,))[0] == _lib.DSP_EINVAL, which
        assert "null" in _lib.last_error()
    assert _build(ident, [0, 0], [1, 0], 2, 9, 2048, null=("sos",))[0] == 0     # no stage: no sos
    zero = ident.copy()
    zero[1, 0, 0] = 0.0                                                         # b0 == 0
    assert _build(zero, *ok)[0] == _lib.DSP_ENOTSUP and "b0" in _lib.last_error()
    assert _build(zero, [2, 0], [1, 0], 2, 9, 2048)[0] == 0                    # ...in an unused row


def test_cascade_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    bank, bytes3 = 4096, 3 * REC

    def call(B=2, n=100, ld_x=100, ld_y=100, bank=bank, nbytes=bytes3, G=3, S=6, max_n=2048,
             rows=64, ld_state=12, x=64, y=64):
        return lib.dsp_eqbank_cascade_f32(x, y, B, n, ld_x, ld_y, bank, nbytes, G, S, max_n, rows,
                                          None, None, ld_state, None)

    assert call(B=0) == 0 and call(n=0) == 0              # no-ops launch nothing
    assert call(B=0, x=None, y=None, bank=None, rows=None) == 0
    assert call(n=2049) == _lib.DSP_EINVAL and "max_n" in _lib.last_error()
    assert call(n=2049, ld_x=4096, ld_y=4096, max_n=4096, B=0) == 0
    assert call(ld_state=11) == _lib.DSP_EINVAL and "ld_state" in _lib.last_error()
    assert call(ld_x=99) == _lib.DSP_EINVAL and call(ld_y=99) == _lib.DSP_EINVAL
    assert call(B=-1) == _lib.DSP_EINVAL and call(n=-1) == _lib.DSP_EINVAL
    assert call(G=0) == _lib.DSP_EINVAL
    assert call(S=9, ld_state=18) == _lib.DSP_EINVAL and call(S=-1) == _lib.DSP_EINVAL
    assert call(max_n=0, n=0) == _lib.DSP_EINVAL
    assert call(nbytes=bytes3 - 1) == _lib.DSP_EINVAL and "bank_bytes" in _lib.last_error()
    assert call(bank=4096 + 128) == _lib.DSP_EINVAL and "aligned" in _lib.last_error()
    for which in ("x", "y", "bank", "rows"):
        assert call(**{which: None}) == _lib.DSP_EINVAL, which
        assert "null" in _lib.last_error()


def _power(A, T):
    """cascade.h's chunk_transition in numpy: the same products in the same
    order (square and multiply, every entry one fma chain over k)."""
    D = A.shape[0]

    def mm(a, b):
        c = np.zeros((D, D))
        for i in range(D):
            for k in range(D):
                for j in range(D):
                    c[i, j] = _fma(float(a[i, k]), float(b[k, j]), float(c[i, j]))
        return c

    r, base, e = np.eye(D), A.copy(), T
    while e > 0:
        if e & 1:
            r = mm(r, base)
        if e > 1:
            base = mm(base, base)
        e >>= 1
    return r


def _fma(a, b, c):
    import math
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_records_hold_the_single_call_numbers():
    """Realisation {1, b1/b0, b2/b0, a1, a2} and prod b0 (design.df2_realization,
    the model of cascade.h's realize), identity stages past the group's own,
    the table's geometry in every record, A^T against the state matrix's power."""
    plan = eqbank.plan_bank(FS, [SIX, TWO, ONE, FLAT])
    assert plan.stages == (6, 2, 1, 0)
    for max_n, T in ((1, 32), (2048, 32), (2049, 64), (4096, 64), (100000, 32 * 49)):
        rec = eqbank.build_table(plan, max_n).view(_record_dtype())
        assert rec.shape == (4,)
        assert list(rec["T"]) == [T] * 4
        assert list(rec["inst"]) == [6] * 4 and list(rec["max_stages"]) == [6] * 4
    assert list(rec["stages"]) == [6, 2, 1, 0] and list(rec["clip"]) == [1, 1, 1, 0]
    assert not rec["pad"].any()
    rec = eqbank.build_table(plan, 2048).view(_record_dtype())
    ident = np.array([1.0, 0, 0, 0, 0])
    for g, (sos, _) in enumerate(plan.groups):
        S = sos.shape[0]
        if S:
            rows, gain, norm = design.df2_realization(sos)
            assert norm
            np.testing.assert_array_equal(rec["c"][g, :S], rows)
            assert rec["G"][g] == gain
        else:
            assert rec["G"][g] == 1.0 and not rec["P"][g].any()
        np.testing.assert_array_equal(rec["c"][g, S:], np.tile(ident, (16 - S, 1)))
    # A^T of the two-band group, padded to six stages: the 4 x 4 block of its
    # own stages is the two-stage system's A^32 to the last bit, and nothing
    # of the identity stages' columns reaches those rows
    sos2 = plan.groups[1][0]
    A, _ = design.state_space(sos2)
    P = rec["P"][1]
    np.testing.assert_array_equal(P[:4, :4], _power(np.asarray(A, dtype=np.float64), 32))
    assert not P[:4, 4:].any() and not P[12:].any() and not P[:, 12:].any()
    # seven stages run as eight
    seven = dict(SIX, Air=2.5)
    rec7 = eqbank.build_table(eqbank.plan_bank(FS, [seven, ONE]), 2048).view(_record_dtype())
    assert list(rec7["inst"]) == [8, 8] and list(rec7["max_stages"]) == [7, 7]
    # an all-bypass bank still builds
    rec0 = eqbank.build_table(eqbank.plan_bank(FS, [FLAT, {}]), 64).view(_record_dtype())
    assert rec0.shape == (1,) and rec0["stages"][0] == 0 and rec0["inst"][0] == 1


def test_planner_merges_identical_plans():
    gains = [SIX, TWO, dict(SIX), FLAT, TWO, ONE, {}, dict(TWO, Brilliance=0.05)]
    plan = eqbank.plan_bank(FS, gains)
    assert plan.B == 8 and plan.G == 4
    assert plan.row_group.dtype == np.int32
    assert list(plan.row_group) == [0, 1, 0, 2, 1, 3, 2, 1]      # groups in order of first use
    assert plan.stages == (6, 2, 0, 1) and plan.max_stages == 6
    for g, src in ((0, SIX), (1, TWO), (3, ONE)):
        np.testing.assert_array_equal(plan.groups[g][0], design.eq_plan(FS, src).sos)
        assert plan.groups[g][1] is True
    # all flat (and the empty dict): the bypass, no stage and no clip
    assert plan.groups[2][0].shape == (0, 5) and plan.groups[2][1] is False
    # dict order is the order of the stages: the reversed dict is another plan
    rev = dict(reversed(list(TWO.items())))
    p2 = eqbank.plan_bank(FS, [TWO, rev])
    assert p2.G == 2
    np.testing.assert_array_equal(p2.groups[1][0], p2.groups[0][0][::-1])
    np.testing.assert_array_equal(p2.groups[0][0], design.eq_plan(FS, TWO).sos)
    # B distinct settings stay B groups
    many = [{"Bass": 1.0 + 0.25 * i} for i in range(40)]
    assert eqbank.plan_bank(FS, many).G == 40


def test_planner_errors_are_raised_on_the_host():
    with pytest.raises(ValueError, match="3 gain sets for 4"):
        eqbank.plan_bank(FS, [SIX, TWO, ONE], batch=4)
    with pytest.raises(ValueError, match="3 gain sets for 4"):
        eqbank.EqBank(FS, [SIX, TWO, ONE], 2048, batch=4)        # before any GPU work
    with pytest.raises(ValueError):
        eqbank.plan_bank(FS, [])
    with pytest.raises(ValueError):
        eqbank.plan_bank(FS, SIX)                                 # one dict is not a bank
    sos = [design.eq_plan(FS, SIX).sos, design.eq_plan(FS, ONE).sos]
    ok = eqbank.plan_from_sos(sos, [True, False], [0, 1, 1, 0])
    assert ok.G == 2 and list(ok.row_group) == [0, 1, 1, 0] and ok.groups[1][1] is False
    assert eqbank.plan_from_sos(sos, True, [1]).groups[0][1] is True
    for bad in ([0, 2], [-1, 0], [], [0.5, 1.0]):
        with pytest.raises(ValueError):
            eqbank.plan_from_sos(sos, True, bad)
        with pytest.raises(ValueError):
            eqbank.EqBank.from_sos(sos, True, bad, 2048)          # before any GPU work
    with pytest.raises(ValueError):
        eqbank.plan_from_sos(sos, [True], [0, 1])                 # one clip flag for two groups
    with pytest.raises(RuntimeError, match="stages"):
        eqbank.plan_from_sos([np.tile([1.0, 0, 0, 0, 0], (9, 1))], True, [0])
    with pytest.raises(ValueError):
        eqbank.EqBank(FS, [SIX], 0)                               # max_n < 1
    # b0 == 0 is the library's answer (DSP_ENOTSUP)
    with pytest.raises(RuntimeError, match="b0"):
        eqbank.build_table(eqbank.plan_from_sos([[[0.0, 0.7, 0.2, -0.5, 0.25]]], True, [0]), 64)
