"""The models behind tests/test_gpu_src_edges.py, checked where no GPU is
needed: tests/src_model.py's vectorised float64 SRC against the per-output loop
of tests/test_stream_plan.py (exactly, on integers) and against the oracle's
resample (<= 1e-12), its non-finite classes against float32 arithmetic, its
mirror of the generic kernel's tile planner against a table worked out from
csrc/src_poly.hip's formula, and dsp_src_polyphase_f32's argument checks, which
answer before any launch."""
import numpy as np
import pytest

import src_model as sm
from test_stream_plan import src_model as loop_model

# (L, M, K, n_in, c, n_out); natural n_out is ceil(((n_in - 1) L + K - c) / M)
EXACT_CASES = [
    (3, 2, 121, 50, 60, 75),          # a plan's own geometry
    (3, 2, 122, 50, 0, 140),          # K even; n_out past the end of the convolution
    (2, 1, 128, 9, 5, 40),            # K even, n_in < T
    (8, 3, 5, 40, 2, 120),            # K < L: phases without a tap
    (5, 4, 10, 33, 7, 20),            # n_out smaller than natural
    (7, 5, 289, 30, 400, 80),         # c inside, outputs run past the end
    (7, 5, 289, 30, 491, 11),         # c on the last sample of the convolution (492 long)
    (7, 5, 289, 30, 492, 11),         # c past the end: all zero
    (1, 16, 641, 700, 320, 60),
    (300, 7, 901, 12, 450, 600),
    (1, 1, 1, 17, 0, 17),             # one tap: the identity
    (4, 4, 9, 1, 3, 3),               # one input sample
]


@pytest.mark.parametrize("L,M,K,n_in,c,n_out", EXACT_CASES)
def test_vectorised_model_is_the_per_output_loop(L, M, K, n_in, c, n_out):
    rng = np.random.default_rng(K * 1000 + n_in)
    taps = rng.integers(-7, 8, K).astype(np.float64)
    x = rng.integers(-7, 8, (2, n_in)).astype(np.float64)
    got = sm.src_model(x, n_out, taps, L, M, c)
    assert got.shape == (2, n_out) and got.dtype == np.float64
    for b in range(2):
        np.testing.assert_array_equal(got[b], loop_model(x[b], n_out, taps, L, M, c))
    np.testing.assert_array_equal(sm.src_model(x[0], n_out, taps, L, M, c), got[0])
    full = (n_in - 1) * L + K
    if c >= full:
        assert not got.any()
    # the absolute model bounds the model, and is it for non-negative data
    a = sm.abs_model(x, n_out, taps, L, M, c)
    assert bool(np.all(np.abs(got) <= a))
    np.testing.assert_array_equal(sm.abs_model(np.abs(x), n_out, np.abs(taps), L, M, c), a)


@pytest.mark.parametrize("L,K,n_in", [(3, 121, 50), (3, 122, 7), (8, 5, 40), (1, 33, 20),
                                      (160, 1023, 12), (300, 901, 3), (4, 9, 1)])
def test_full_conv_is_numpy_convolve_of_the_zero_stuffed_row(L, K, n_in):
    rng = np.random.default_rng(L + K)
    for ints in (True, False):
        taps = rng.integers(-7, 8, K).astype(np.float64) if ints else rng.uniform(-1, 1, K)
        x = rng.integers(-7, 8, n_in).astype(np.float64) if ints else rng.uniform(-1, 1, n_in)
        xe = np.zeros(n_in * L)
        xe[::L] = x
        want = np.convolve(xe, taps)[:(n_in - 1) * L + K]      # (the rest: the last L - 1 zeros)
        got = sm.full_conv(x, taps, L)
        assert got.shape == want.shape
        if ints:
            np.testing.assert_array_equal(got, want)
        else:
            assert float(np.max(np.abs(got - want))) <= 1e-12


@pytest.mark.parametrize("L,M,num_taps,n_in", [(3, 2, None, 4800), (2, 1, 127, 4800),
                                               (5, 7, None, 3001), (1, 3, None, 7)])
def test_model_is_the_oracle_at_plan_geometry(L, M, num_taps, n_in):
    from dspcore import design
    from oracle import dsp_ref_cpu as orc
    plan = design.src_plan(n_in, 48000, M, L, num_taps)
    x = np.random.default_rng(n_in).uniform(-1, 1, n_in)
    want, _ = orc.resample(x, 48000, M, L, num_taps)
    got = sm.src_model(x, plan.n_out, plan.taps, L, M, plan.c_offset)
    assert got.shape == want.shape
    err = float(np.max(np.abs(got - want)))
    print(f"L{L}/M{M} K={plan.K} n_in={n_in}: model vs oracle {err:.3g}")
    assert err <= 1e-12


def test_nf_class_is_float32_arithmetic():
    """nf_class against sum taps . xn accumulated with numpy float32 in the
    kernel's order (t descending), zero taps included."""
    L, M, K, n_in, c, n_out = 3, 2, 21, 40, 4, 70
    rng = np.random.default_rng(5)
    taps = rng.uniform(-1, 1, K).astype(np.float32)
    taps[[0, 7, 20]] = 0.0
    rows = [[(0, np.nan)], [(39, np.inf)], [(10, np.inf), (12, -np.inf)], [(10, -np.inf), (30, np.inf)],
            [(20, np.inf), (21, np.inf)], []]
    x = rng.uniform(-1, 1, (len(rows), n_in)).astype(np.float32)
    for r, sp in enumerate(rows):
        for p, v in sp:
            x[r, p] = v
    got = sm.nf_class(x, n_out, taps, L, M, c)
    assert got.shape == (len(rows), n_out)
    with np.errstate(invalid="ignore"):
        for r in range(len(rows)):
            xn = np.where(np.isfinite(x[r]), np.float32(0), x[r])
            for m in range(n_out):
                j = m * M + c
                phi, q = j % L, j // L
                s = np.float32(0)
                for t in range((K - 1 - phi) // L, -1, -1):
                    if 0 <= q - t < n_in:
                        s = np.float32(s + taps[phi + L * t] * xn[q - t])
                assert got[r, m] == sm.classify(s), (r, m)
    assert set(np.unique(got)) == {sm.FINITE, sm.PINF, sm.NINF, sm.NAN_}
    assert not got[-1].any()
    np.testing.assert_array_equal(sm.classify(np.array([1.0, np.inf, -np.inf, np.nan, -0.0])),
                                  [sm.FINITE, sm.PINF, sm.NINF, sm.NAN_, sm.FINITE])


# (L, M, K) -> the generic kernel's tile (None: refused), from launch_src_rows:
# bank = ceil4(L T) floats, window = ceil4((t - 1) M / L + T + 10) floats,
# 4 (bank + window) <= 160 * 1024 - 64, t halved from 4096 down to 64
PLANNER = [((1, 16, 641), 2048), ((1, 64, 2561), 512), ((1, 400, 801), 64), ((1, 1, 20000), 512),
           ((1, 1, 20435), 64), ((1, 1, 20436), None), ((160, 147, 6401), 4096)]


def test_planner_mirror():
    assert (sm.GEN_NT, sm.GEN_TILE, sm.GEN_TILE_MIN, sm.LDS_MAX) == (256, 4096, 64, 163776)
    for (L, M, K), tile in PLANNER:
        assert sm.gen_tile(L, M, K) == tile, (L, M, K)
    # the formula itself, spelled out for two rows of the table
    assert sm.branch_taps(6401, 160) == 41
    assert sm.gen_lds_bytes(160, 147, 6401, 4096) == 4 * (160 * 41 + 3816)   # 4095*147/160 + 51 = 3813
    assert sm.gen_lds_bytes(1, 1, 20435, 64) == 4 * (20436 + 20508) == sm.LDS_MAX
    assert sm.gen_lds_bytes(1, 1, 20436, 64) == sm.LDS_MAX + 16
    # each shrunk tile is the largest that fits
    for (L, M, K), tile in PLANNER:
        if tile is not None and tile < sm.GEN_TILE:
            assert sm.gen_lds_bytes(L, M, K, 2 * tile) > sm.LDS_MAX >= sm.gen_lds_bytes(L, M, K, tile)
    # the default designs of the benchmark ratios keep the full tile
    for L, M, K in [(160, 147, 1023), (147, 160, 1023), (7, 5, 289), (300, 7, 901), (8, 3, 5)]:
        assert sm.gen_tile(L, M, K) == sm.GEN_TILE


P = 1024      # a non-null address no check dereferences


def _src(x=P, y=P, B=1, n_in=10, ld_x=10, n_out=15, ld_y=15, taps=P, K=121, L=3, M=2, c=60):
    from dspcore import _lib
    rc = _lib.load().dsp_src_polyphase_f32(x, y, B, n_in, ld_x, n_out, ld_y, taps, K, L, M, c, None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,text", [
    (dict(B=-1), "bad sizes B=-1 n_in=10 n_out=15"),
    (dict(n_in=0, ld_x=0), "bad sizes B=1 n_in=0 n_out=15"),
    (dict(n_in=-3), "bad sizes B=1 n_in=-3 n_out=15"),
    (dict(n_out=-1), "bad sizes B=1 n_in=10 n_out=-1"),
    (dict(L=0), "bad L=0 M=2 K=121"),
    (dict(M=0), "bad L=3 M=0 K=121"),
    (dict(K=0), "bad L=3 M=2 K=0"),
    (dict(L=-2), "bad L=-2 M=2 K=121"),
    (dict(c=-1), "bad c_offset -1"),
    (dict(ld_x=9), "leading dimension too small"),
    (dict(ld_y=14), "leading dimension too small"),
    (dict(x=None), "null pointer"),
    (dict(y=None), "null pointer"),
    (dict(taps=None), "null pointer"),
    (dict(x=None, y=None, taps=None), "null pointer"),
])
def test_launch_src_argument_checks(kw, text):
    """Every DSP_REQUIRE of launch_src answers DSP_EINVAL with its text, before
    any launch (no GPU here)."""
    from dspcore import _lib
    rc, msg = _src(**kw)
    assert rc == _lib.DSP_EINVAL and text in msg, (rc, msg)
    with pytest.raises(ValueError):
        _lib.check(rc, "dsp_src_polyphase_f32")


def test_launch_src_nothing_to_do():
    """B == 0 and n_out == 0 return DSP_OK with null pointers; the size checks
    still come first."""
    from dspcore import _lib
    assert _src(x=None, y=None, taps=None, B=0)[0] == _lib.DSP_OK
    assert _src(x=None, y=None, taps=None, n_out=0, ld_y=0)[0] == _lib.DSP_OK
    assert _src(x=None, y=None, taps=None, B=0, n_out=0, ld_y=0)[0] == _lib.DSP_OK
    assert _src(x=None, y=None, taps=None, B=0, L=0)[0] == _lib.DSP_EINVAL
    assert _src(x=None, y=None, taps=None, n_out=0, ld_y=0, c=-1)[0] == _lib.DSP_EINVAL
