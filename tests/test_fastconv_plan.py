"""Fast convolution without a GPU (include/dspcore_fastconv.h): the default
transform size, design.fastconv_plan's tables, the numpy model of the kernel
(tests/fastconv_model.py) against float64 np.convolve at the GPU test's shapes,
and the argument checks of dsp_fastconv_f32, which come before any device
work."""
import re

import numpy as np
import pytest

import fastconv_model as fm
from dspcore import _lib, design

EINVAL, ENOTSUP = _lib.DSP_EINVAL, _lib.DSP_ENOTSUP


def test_default_transform_size():
    lib = _lib.load()
    want = {1: 6, 2: 6, 17: 6, 18: 7, 1023: 12, 4097: 14, 8193: 14}
    for K, lg in want.items():
        assert lib.dsp_fastconv_log2n(K) == lg, K
        assert design.fastconv_log2n(K) == lg, K
        N = 1 << lg
        assert K <= N // 2 + 1 and (N >= 4 * (K - 1) or lg == 14)
        assert lg == 6 or (N // 2) < 4 * (K - 1)          # the smallest such size
    assert lib.dsp_fastconv_log2n(8194) == ENOTSUP and _lib.last_error()
    for K in (0, -5):
        assert lib.dsp_fastconv_log2n(K) == EINVAL and _lib.last_error()
    with pytest.raises(RuntimeError):
        design.fastconv_log2n(8194)
    with pytest.raises(ValueError):
        design.fastconv_log2n(0)


@pytest.mark.parametrize("K", [1, 2, 121, 1023, 8193])
def test_plan_tables(K):
    taps64 = np.random.default_rng(K).standard_normal(K) / 3
    p = design.fastconv_plan(taps64)
    N = 1 << design.fastconv_log2n(K)
    assert (p.K, p.log2n, p.n_fft, p.hop) == (K, N.bit_length() - 1, N, N - (K - 1))
    assert p.taps.dtype == np.float32 and p.hf.dtype == np.complex64 and p.hf.shape == (N,)
    assert np.array_equal(p.taps, taps64.astype(np.float32))
    # float64 FFT of the float32 tap values, divided by N, rounded once
    want = np.fft.fft(p.taps.astype(np.float64), N) / N
    assert np.array_equal(p.hf, want.astype(np.complex64))
    assert np.max(np.abs(p.hf - want)) <= 2.0 ** -24 * np.max(np.abs(want)) * 1.5
    if K > 1:
        # an explicit size: the smallest that holds the taps, and one too small
        lg = max(6, (2 * (K - 1) - 1).bit_length())
        q = design.fastconv_plan(taps64, log2n=lg)
        assert q.n_fft == 1 << lg and q.hop == q.n_fft - (K - 1) >= 1
        if lg > 6:
            with pytest.raises(ValueError):
                design.fastconv_plan(taps64, log2n=lg - 1)
    for lg in (5, 15):
        with pytest.raises(RuntimeError):
            design.fastconv_plan(taps64[:1], log2n=lg)
    with pytest.raises(ValueError):
        design.fastconv_plan(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        design.fastconv_plan([])


@pytest.mark.parametrize("N", fm.SIZES)
def test_model_meets_the_bound_at_the_gpu_shapes(N):
    """The kernel's arithmetic in numpy against float64 np.convolve: every tap
    count, offset and row length of tests/test_gpu_fastconv.py, both n_out."""
    lg = N.bit_length() - 1
    worst = 0.0
    for K in fm.tap_counts(N):
        taps = fm.make_taps(K)
        for n in fm.row_lengths(N, K):
            x = fm.make_rows(N, K, n)
            ref = fm.full_reference(x, taps)
            b = fm.bound(taps, x)
            for off in fm.offsets(K):
                n_full = n + K - 1 - off
                got = fm.model(x, taps, lg, off, n_full)
                err = float(np.max(np.abs(got - ref[:, off:off + n_full])))
                worst = max(worst, err / b)
                assert err <= b, (N, K, n, off, err / b)
    print(f"N={N}: model worst error / bound {worst:.3f}")


def test_model_stream_and_history():
    """Cuts at multiples of 2 V are bitwise the one call (the same blocks and
    pairs); ragged cuts stay within the bound."""
    N, K = 512, 129
    V = N - (K - 1)
    taps = fm.make_taps(K)
    n = 6 * V + 11
    x = np.random.default_rng(5).uniform(-1, 1, (3, n)).astype(np.float32)
    one = fm.model(x, taps, 9)
    ref = fm.full_reference(x, taps)[:, :n]
    for cuts, exact in (([2 * V, 4 * V, 11], True), ([4 * V, 2 * V + 11], True),
                        ([1, V, 0, 3 * V + 5, 2 * V + 5], False)):
        assert sum(cuts) == n
        hist, pos, outs = np.zeros((3, K - 1), np.float32), 0, []
        for c in cuts:
            outs.append(fm.model(x[:, pos:pos + c], taps, 9, hist=hist))
            hist = np.concatenate([hist, x[:, pos:pos + c]], axis=1)[:, -(K - 1):]
            pos += c
        got = np.concatenate(outs, axis=1)
        if exact:
            assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), cuts
        assert np.max(np.abs(got - ref)) <= fm.bound(taps, x), cuts


def _conv(x=0x10000, y=0x80000, B=3, n_in=100, ld_x=None, n_out=None, ld_y=None, offset=0,
          hist_in=0x100000, hist_out=0x180000, ld_hist=None, taps=0x200000, K=17, hf=0x280000,
          log2n=6, tw=0x300000):
    """dsp_fastconv_f32 with dummy pointers that no check dereferences."""
    n_out = n_in if n_out is None else n_out
    return _lib.load().dsp_fastconv_f32(
        x, y, B, n_in, n_in if ld_x is None else ld_x, n_out, n_out if ld_y is None else ld_y,
        offset, hist_in, hist_out, max(K - 1, 0) if ld_hist is None else ld_hist, taps, K, hf,
        log2n, tw, None)


def test_status_codes_before_any_device_work():
    N = 64
    einval = [dict(K=0), dict(K=-1), dict(K=N // 2 + 2), dict(B=-1), dict(n_in=-1),
              dict(n_out=-1), dict(offset=-1), dict(offset=17), dict(n_out=100 + 16 + 1),
              dict(n_out=100 + 16 - 3 + 1, offset=3), dict(ld_x=99), dict(ld_y=99),
              dict(ld_hist=15), dict(ld_hist=15, hist_in=None), dict(ld_hist=15, hist_out=None),
              dict(hist_out=0x100000)]
    for kw in einval:
        assert _conv(**kw) == EINVAL, kw
        assert _lib.last_error(), kw
    for lg in (5, 15, 0, -1, 31):
        assert _conv(log2n=lg) == ENOTSUP, lg
        assert _lib.last_error()
        # ... also with every pointer null, and whatever else is wrong
        assert _conv(log2n=lg, x=None, y=None, hist_in=None, hist_out=None, taps=None, hf=None,
                     tw=None, K=0) == ENOTSUP
    # null pointers where one is read or written (still no device work); a null
    # hist_in is a zero history and a null hist_out is not written
    for name in ("x", "y", "taps", "hf", "tw"):
        assert _conv(**{name: None}) == EINVAL, name
        assert _lib.last_error(), name
    # x and y must not overlap
    assert _conv(y=0x10000 + 4 * 50) == EINVAL
    # every check precedes B == 0, which launches nothing
    assert _conv(B=0) == 0
    assert _conv(B=0, x=None, y=None, hist_in=None, hist_out=None, taps=None, hf=None,
                 tw=None) == 0
    assert _conv(B=0, K=0) == EINVAL
    assert _conv(B=0, offset=17) == EINVAL
    # the limits themselves pass the checks (B == 0: nothing launched)
    assert _conv(B=0, K=N // 2 + 1, ld_hist=N // 2, offset=N // 2, n_out=100) == 0
    assert _conv(B=0, K=1, ld_hist=0, n_out=100) == 0
    assert _conv(B=0, n_out=116) == 0
    assert _conv(B=0, n_out=113, offset=3) == 0
    assert _conv(B=0, n_in=0, n_out=0) == 0
    assert _conv(B=0, ld_hist=0, hist_in=None, hist_out=None) == 0      # no history: no pitch
    for lg in (6, 14):
        assert _conv(B=0, log2n=lg, K=(1 << lg) // 2 + 1) == 0


def test_version_exports_and_signatures():
    lib = _lib.load()
    assert lib.dsp_fastconv_version() == 10000
    with open(_lib.FASTCONV_HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^int (dsp_fastconv_[a-z0-9_]+)\(", text, flags=re.M))
    assert declared == {"dsp_fastconv_version", "dsp_fastconv_log2n", "dsp_fastconv_f32"}
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == {n for n in _lib._SIGNATURES if n.startswith("dsp_fastconv_")}
    # the other headers keep their symbols and versions
    assert len(_lib.header_symbols()) == 35
    assert (lib.dsp_version(), lib.dsp_stream_version(), lib.dsp_eqbank_version(),
            lib.dsp_eqlive_version(), lib.dsp_stspec_version()) == (20700, 10000, 10000, 10000,
                                                                    10000)


def test_drop_in_and_package_layers():
    import dspcore
    from modules import dsp_core
    assert "fastconv" in dspcore.__all__ and dspcore.__version__ == "1.8.0"
    assert "convolucion_rapida" in dsp_core.__all__
    assert 1 <= design.FASTCONV_MIN_TAPS <= design.FASTCONV_MAX_TAPS == 8193
