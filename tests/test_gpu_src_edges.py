"""The standalone polyphase SRC (csrc/src_poly.hip, dsp_src_polyphase_f32) at
the edges of both of its kernels, against the float64 model of the contract in
include/dspcore.h (tests/src_model.py; tests/test_src_model.py pins it).

Every call is ops.src_polyphase(x, plan, taps=..., out=...) with a
design.SrcPlan made here, so K, c_offset and n_out are free, the test's own
taps, and x / out / taps as views inside larger buffers: x's surroundings are
NaN (a load outside [0, n_in) shows in y), the taps' are 1.0 (so does a tap
read at or past K), out's are a sentinel whose bits must survive (pitch
padding, the floats before row 0 and after the last row).

The dispatch rule is REG below: the register-blocked kernel's (L, M, ceil(K/L))
and outputs per block; everything else is the generic kernel with the tile of
src_model.gen_tile.  Both kernels trace as `src_poly`, so which one ran is
asserted on the case's shape, and every call's trace must be exactly its
launches.

(a) Exact.  Integer taps and samples, |h|, |x| <= 7 (3 for 20 435 taps), so
    every partial sum is an integer below 2^24, float32 FMAs are exact in any
    order, and y must equal the model bit for bit (assert_array_equal; the
    non-zero taps are >= 1, far above the flush threshold; some taps are 0).
    Register-blocked, each of the four instantiations, B = 3:
      n_out in {1, 3, 4, TILE-1, TILE, TILE+1, TILE+6, 2 TILE+2}: one output,
        counts that are no multiple of 4 (store_tile's scalar tail), a ragged
        last tile; n_in so short that the last windows run past the row's end
        and not a multiple of 4 under an aligned pitch (load_window's guarded
        float4); n_in = 1 and n_in < T;
      every K of the instantiation's T: branches one tap shorter (kk < K), even K;
      c_offset 0, 1, 2 (qlo < 0: qa rounds towards -inf), L (T-1) + L r for
        r = 0..3 (qlo - qa = r), the plan's own, one that puts the second tile
        wholly past the input (zeros), 2^31 + 5 (64-bit indices, zeros).
    Generic: (8,3,5) T = 1 with tap-less phases; (5,4,10) T = 2; (7,5,K) for
      K = 287..290, T = 41 and 42 (the u < T tail taken and not); (300,7,901),
      L above the block's 256 threads (phi += dphi wraps); 160/147 and 147/160
      at K = 1023; the same n_out and c_offset families at (7,5,289)'s tile of
      4096; the shrunk tiles (1,16,641) 2048, (1,64,2561) 512, (1,400,801) 64
      with n_out on both sides of a tile boundary; L = M = 1, K = 20 435 with
      all 163 776 bytes of LDS; K = 20 436 and 65 536 refused ("does not fit in
      LDS"), nothing launched, y untouched.
(b) Placement.  (3,2,41) and (160,147,1023): x and out each aligned, shifted by
    one float, or with a pitch = 1 (mod 4) -- all four (vec_x, vec_y) -- give
    bitwise one y; B = 1 with a padded pitch; a row alone is the row in the batch.
(c) Rounding.  The library's designs (design.src_plan) for the four
    instantiations, 160/147 K = 1023 and 1/16, noise in [-1, 1], n_out just
    over two tiles, against the model with design.kernel_taps in float64:
    |y - model| <= (T + 2) 2^-24 sum|h x| per output, no absolute term -- each
    kernel sums two FMA chains of at most ceil((T + 1) / 2) terms and adds
    them, so the standard bound gamma_n with n <= T/2 + 2 roundings holds with
    a factor of about two to spare.  Worst err / bound on an MI355X: 3/2
    K = 121 0.074, 3/2 K = 255 0.043, 2/1 K = 127 0.051, 2/1 K = 81 0.077,
    160/147 K = 1023 0.258, 1/16 K = 641 0.007 (the clean rows of (d): 0.077,
    0.055, 0.061, 0.077, 0.271; 8/3 K = 5: 0.328).
(d) Non-finite.  Design taps (all non-zero), noise, one NaN / +inf / -inf per
    row at the edges of the SRC's own blocks: q(m) and Q(m) = q(m) - (T - 1)
    for m = TILE-1, TILE, TILE+1, and q(m)+1, q(m)+2, Q(m)-1, which the packed
    pairs and the float4-rounded window load but no tap of output m meets (Q of
    both parities); both infs in one window; the row's first and last sample.
    y's NaN / +inf / -inf masks are src_model.nf_class's exactly; every other
    output is bitwise the kernel's own on the row with those samples zeroed,
    and that clean y is inside bound (c).  The same for (8,3,5), K < L, where
    the outputs of phases 5..7 meet no tap and stay 0 beside an inf or NaN.

Each case asserts the edge it is there for: which kernel, the tile, blocks,
count mod 4, qlo - qa, the vec flags, the launch count.  The file takes about
3 s on an MI355X."""
import time

import numpy as np
import pytest
import torch

import src_model as sm
from test_gpu_stream_edges import _bits, _vec

pytestmark = pytest.mark.gpu

# (L, M, ceil(K / L)) of k_src_reg's instantiations -> outputs per block
REG = {(3, 2, 41): 2880, (3, 2, 85): 1344, (2, 1, 64): 3840, (2, 1, 41): 3840}
# every K that maps to the instantiation's T; the last is the library's design
REG_K = {(3, 2, 41): (122, 123, 121), (3, 2, 85): (253, 254, 255), (2, 1, 64): (128, 127),
         (2, 1, 41): (82, 81)}
REG_IDS = ["L3M2T41", "L3M2T85", "L2M1T64", "L2M1T41"]
SENTINEL = -12345.75       # exact in float32
NAN, INF = float("nan"), float("inf")
C_HUGE = (1 << 31) + 5


def _geom(L, M, K):
    """(T, register-blocked?, outputs per block) of a call."""
    T = sm.branch_taps(K, L)
    reg = (L, M, T) in REG
    return T, reg, REG[(L, M, T)] if reg else sm.gen_tile(L, M, K)


def _q(m, L, M, c):
    return (m * M + c) // L


def _qlo_minus_qa(m0, L, M, T, c):
    """Offset of block m0's first window in its float4-aligned LDS window
    (qa = qlo rounded down to a multiple of 4, towards -inf)."""
    qlo = _q(m0, L, M, c) - (T - 1)
    return qlo, qlo - (qlo // 4) * 4


def _ceil4(n):
    return (n + 3) // 4 * 4


def _view(gpu, B, n, fill, lead=0, pad=0):
    """A [B, n] float32 view inside a 1-D buffer of `fill`: 8 + lead floats
    before row 0, pitch ceil4(n) + 4 + pad, 8 floats after the last row.
    lead = pad = 0 is float4-aligned; lead = 1 shifts the view by one float,
    pad = 1 makes the pitch 1 (mod 4)."""
    pitch = _ceil4(n) + 4 + pad
    buf = torch.full((8 + lead + B * pitch + 8,), fill, dtype=torch.float32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    v = torch.as_strided(buf, (B, n), (pitch, 1), 8 + lead)
    assert _vec(v) == int(lead % 4 == 0 and pad % 4 == 0)
    return buf, v


def _traced(fn):
    """(result or exception of fn(), trace names of the library's launches)."""
    from dspcore import _lib
    _lib.trace_enable(True)
    _lib.trace_read()
    try:
        try:
            out = fn()
        except Exception as e:          # the refusal tests look at it
            out = e
        names = [k for k, _ in _lib.trace_read()]
    finally:
        _lib.trace_enable(False)
    return out, names


def _run(gpu, x, taps, L, M, c, n_out, reg, xl=(0, 0), yl=(0, 0), vec=None):
    """y [B, n_out] float32 (numpy) of one dsp_src_polyphase_f32 call on the
    rows of x (numpy float32) with `taps` (numpy float32).  xl, yl: (lead, pad)
    of x's and out's views.  Asserts the dispatch side, the vec flags, the
    trace, and that no float of out's buffer outside the outputs changed."""
    from dspcore import design, ops
    B, n_in = x.shape
    K = taps.size
    assert taps.dtype == np.float32 and x.dtype == np.float32
    T, is_reg, tile = _geom(L, M, K)
    assert is_reg == reg and tile is not None, (L, M, K, T, is_reg, tile)
    _, xd = _view(gpu, B, n_in, NAN, *xl)
    xd.copy_(torch.from_numpy(x))
    obuf, out = _view(gpu, B, n_out, SENTINEL, *yl)
    if vec is not None:
        assert (_vec(xd), _vec(out)) == vec
    # the K taps inside a buffer of ones: a tap read at or past K (kk < K, the
    # branches that are one tap short, the phases without a tap) is in bounds
    # and shows in y
    tbuf = torch.ones(8 + K + L + 8, dtype=torch.float32, device=gpu)
    td = tbuf[8:8 + K]
    td.copy_(torch.from_numpy(taps))
    plan = design.SrcPlan(L, M, K, taps.astype(np.float64), c, n_in, n_out, 0)
    res, names = _traced(lambda: ops.src_polyphase(xd, plan, taps=td, out=out))
    assert not isinstance(res, Exception), res
    assert names == ["src_poly"], names
    y = out.cpu().numpy()
    host = _bits(obuf.cpu().numpy()).copy()
    inside = np.zeros(host.size, dtype=bool)
    for b in range(B):
        at = out.storage_offset() + b * out.stride(0)
        inside[at:at + n_out] = True
    sent = _bits(np.array([SENTINEL], dtype=np.float32))[0]
    changed = np.flatnonzero((host != sent) & ~inside)
    assert changed.size == 0, f"floats outside the outputs written at {changed[:12].tolist()}"
    return y


def _int_taps(rng, K, L, lim):
    """Integer taps in [-lim, lim]: the first and last L (the ends of every
    branch) non-zero, a few zeros inside."""
    t = rng.integers(-lim, lim + 1, K)
    ends = np.r_[np.arange(min(L, K)), np.arange(max(K - L, 0), K)]
    t[ends] = np.where(t[ends] == 0, lim, t[ends])
    if K > 4 * L:
        t[2 * L + 1:K - L:max(1, K // 9)] = 0
    return t.astype(np.float32)


def _int_rows(rng, B, n, lim):
    x = rng.integers(-lim, lim + 1, (B, n))
    x[:, [0, -1]] = np.where(x[:, [0, -1]] == 0, lim, x[:, [0, -1]])
    return x.astype(np.float32)


def _short_n_in(L, M, T, c, n_out):
    """An input length at which the last (T - 1) / 2 + 1 samples of the last
    output's window lie past the row's end."""
    return max(1, _q(n_out - 1, L, M, c) - (T - 1) // 2)


def _exact(gpu, L, M, K, c, n_out, n_in, reg, lim=7, B=3, seed=0, taps=None, **place):
    """One exact case; returns (y, model)."""
    T = sm.branch_taps(K, L)
    assert T * lim * lim < 1 << 24
    rng = np.random.default_rng([seed, L, M, K, n_out, n_in, c % 9973])
    if taps is None:
        taps = _int_taps(rng, K, L, lim)
    x = _int_rows(rng, B, n_in, lim)
    y = _run(gpu, x, taps, L, M, c, n_out, reg, **place)
    want = sm.src_model(x, n_out, taps, L, M, c)
    np.testing.assert_array_equal(
        y.astype(np.float64), want,
        err_msg=f"L={L} M={M} K={K} T={T} c={c} n_in={n_in} n_out={n_out} B={B}")
    return y, want


def _n_out_family(tile):
    fam = [1, 3, 4, tile - 1, tile, tile + 1, tile + 6, 2 * tile + 2]
    # a single output, store tails of 1, 2 and 3 floats, full and ragged last tiles
    assert {(n - 1) % tile + 1 for n in fam} >= {1, 3, 4, tile - 1, tile, 6, 2}
    assert {n % 4 for n in fam} == {0, 1, 2, 3} and tile % 4 == 0
    assert {-(-n // tile) for n in fam} == {1, 2, 3}
    return fam


def _c_family(L, M, K, T, tile):
    """[(c_offset, n_in or None, what)] at n_out = tile + 6."""
    fam = [(c, None, "negative qlo") for c in (0, 1, 2)]
    for c, _, _ in fam:
        qlo, _ = _qlo_minus_qa(0, L, M, T, c)
        assert qlo < 0
    for r in range(4):
        c = L * (T - 1) + L * r
        assert _qlo_minus_qa(0, L, M, T, c) == (r, r)
        fam.append((c, None, f"qlo - qa = {r}"))
    fam.append(((K - 1) // 2, None, "the plan's own"))
    # the second block's first window starts at or after n_in: all of it zero
    c = L * (T - 1) + 1
    n_in = tile * M // L
    assert _q(tile, L, M, c) - (T - 1) >= n_in > _q(0, L, M, c) - (T - 1)
    fam.append((c, n_in, "last tile past the input"))
    fam.append((C_HUGE, 100, "c_offset above 2^31"))
    return fam


# --------------------------------------------------------------------------- (a) register-blocked
@pytest.mark.parametrize("inst", list(REG), ids=REG_IDS)
def test_reg_exact_n_out(gpu, inst):
    L, M, T = inst
    tile, K = REG[inst], REG_K[inst][-1]
    c = (K - 1) // 2
    t0 = time.perf_counter()
    mod4 = set()
    for n_out in _n_out_family(tile):
        n_in = _short_n_in(L, M, T, c, n_out)
        # the last output's window ends (T - 1) / 2 + 1 samples past the row
        assert n_in == 1 or _q(n_out - 1, L, M, c) - n_in + 1 == (T - 1) // 2 + 1
        mod4.add(n_in % 4)
        _exact(gpu, L, M, K, c, n_out, n_in, True, vec=(1, 1))
    # rows that are no multiple of 4 long under an aligned pitch: the last
    # float4 of the window straddles the row's end
    for n_in in (tile * M // L + 1, tile * M // L + 2, tile * M // L + 3):
        _exact(gpu, L, M, K, c, tile + 6, n_in, True, vec=(1, 1))
        mod4.add(n_in % 4)
    assert mod4 >= {1, 2, 3}
    # one sample, and fewer samples than a branch has taps, many outputs
    for n_in in (1, T - 1):
        _exact(gpu, L, M, K, c, tile + 6, n_in, True)
    print(f"{inst}: n_out family, K={K} c={c}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("inst", list(REG), ids=REG_IDS)
def test_reg_exact_every_K(gpu, inst):
    """Every K of the instantiation's T: with K < L T the last tap of some
    branches does not exist (kk < K); even K."""
    L, M, T = inst
    tile = REG[inst]
    assert {sm.branch_taps(K, L) for K in REG_K[inst]} == {T}
    assert {K % 2 for K in REG_K[inst]} == {0, 1}
    assert min(REG_K[inst]) == L * (T - 1) + 1 and max(REG_K[inst]) == L * T
    for K in REG_K[inst]:
        for c in ((K - 1) // 2, 0):
            n_out = tile + 6
            _exact(gpu, L, M, K, c, n_out, _short_n_in(L, M, T, c, n_out), True, seed=K)


@pytest.mark.parametrize("inst", list(REG), ids=REG_IDS)
def test_reg_exact_c_offset(gpu, inst):
    L, M, T = inst
    tile, K = REG[inst], REG_K[inst][-1]
    n_out = tile + 6
    for c, n_in, what in _c_family(L, M, K, T, tile):
        if n_in is None:
            n_in = _short_n_in(L, M, T, c, n_out)
        y, want = _exact(gpu, L, M, K, c, n_out, n_in, True)
        if what == "last tile past the input":
            assert want[:, :tile].any() and not want[:, tile:].any()
            assert not _bits(y[:, tile:]).any()            # +0.0, not -0.0
        if c == C_HUGE:
            assert not _bits(y).any()


# --------------------------------------------------------------------------- (a) generic
# (L, M, K) -> n_outs; all at the full tile of 4096
GENERIC = {
    (8, 3, 5): (1, 4097),               # T = 1; phases 5, 6, 7 have no tap
    (5, 4, 10): (4095, 4097),           # T = 2
    (7, 5, 287): (4097,),               # T = 41, odd: the u < T tail
    (7, 5, 288): (4097,),               # T = 42, K even: the last branch one tap short
    (7, 5, 289): (4097,),
    (7, 5, 290): (4097,),
    (300, 7, 901): (255, 4097),         # L > 256 threads
    (160, 147, 1023): (4097,),          # T = 7
    (147, 160, 1023): (4097,),
}
# the (7, 5) cases meet the generic kernel's odd-T tail both ways
assert {sm.branch_taps(K, L) % 2 for L, M, K in GENERIC if (L, M) == (7, 5)} == {0, 1}


@pytest.mark.parametrize("L,M,K", list(GENERIC), ids=[f"L{a}M{b}K{c}" for a, b, c in GENERIC])
def test_generic_exact(gpu, L, M, K):
    T, reg, tile = _geom(L, M, K)
    assert not reg and tile == sm.GEN_TILE == 4096
    if (L, M) == (8, 3):
        assert T == 1 and K < L
    if (L, M) == (5, 4):
        assert T == 2
    if (L, M) == (7, 5):
        assert T == (41 if K == 287 else 42)
    if L == 300:
        step = sm.GEN_NT * M        # the kernel's per-iteration advance: (dq, dphi)
        assert L > sm.GEN_NT and step % L + (L - 1) >= L
    t0 = time.perf_counter()
    for n_out in GENERIC[(L, M, K)]:
        for c in ((K - 1) // 2, 0):
            _exact(gpu, L, M, K, c, n_out, _short_n_in(L, M, T, c, n_out), False)
    print(f"L{L}/M{M} K={K} T={T}: {time.perf_counter() - t0:.2f} s")


def test_generic_exact_families(gpu):
    """The register-blocked cases' n_out and c_offset families at the generic
    kernel's tile."""
    L, M, K = 7, 5, 289
    T, reg, tile = _geom(L, M, K)
    assert not reg and tile == 4096 and T == 42
    c = (K - 1) // 2
    t0 = time.perf_counter()
    for n_out in _n_out_family(tile):
        _exact(gpu, L, M, K, c, n_out, _short_n_in(L, M, T, c, n_out), False)
    n_out = tile + 6
    for c, n_in, what in _c_family(L, M, K, T, tile):
        if n_in is None:
            n_in = _short_n_in(L, M, T, c, n_out)
        y, want = _exact(gpu, L, M, K, c, n_out, n_in, False)
        if what == "last tile past the input":
            assert want[:, :tile].any() and not want[:, tile:].any()
            assert not _bits(y[:, tile:]).any()
        if c == C_HUGE:
            assert not _bits(y).any()
    for n_in in (1, T - 1, tile * M // L + 1, tile * M // L + 3):
        _exact(gpu, L, M, K, (K - 1) // 2, n_out, n_in, False, vec=(1, 1))
    print(f"generic families at L7/M5 K=289: {time.perf_counter() - t0:.2f} s")


# (L, M, K) -> (tile, n_outs on both sides of a tile boundary)
SHRUNK = {(1, 16, 641): (2048, (2047, 2048, 2049, 4097)), (1, 64, 2561): (512, (513,)),
          (1, 400, 801): (64, (65, 129))}


@pytest.mark.parametrize("L,M,K", list(SHRUNK), ids=[f"L{a}M{b}K{c}" for a, b, c in SHRUNK])
def test_generic_shrunk_tile(gpu, L, M, K):
    """M / L so large that a 4096-output window does not fit: launch_src_rows
    halves the tile."""
    want_tile, n_outs = SHRUNK[(L, M, K)]
    T, reg, tile = _geom(L, M, K)
    assert not reg and tile == want_tile < sm.GEN_TILE
    assert sm.gen_lds_bytes(L, M, K, 2 * tile) > sm.LDS_MAX >= sm.gen_lds_bytes(L, M, K, tile)
    assert {-(-n // tile) for n in n_outs} >= {2} and any(n % tile == 1 for n in n_outs)
    t0 = time.perf_counter()
    c = (K - 1) // 2
    for n_out in n_outs:
        _exact(gpu, L, M, K, c, n_out, _short_n_in(L, M, T, c, n_out), False)
    print(f"L{L}/M{M} K={K} tile {tile}: {time.perf_counter() - t0:.2f} s")


def test_generic_whole_lds(gpu):
    """L = M = 1, K = 20 435: bank and a 64-output window take exactly the
    160 KiB - 64 bytes the planner allows."""
    L = M = 1
    K, n_in, n_out, c = 20435, 300, 130, 20000
    T, reg, tile = _geom(L, M, K)
    assert not reg and tile == sm.GEN_TILE_MIN == 64 and T == K
    assert sm.gen_lds_bytes(L, M, K, tile) == sm.LDS_MAX == 163776
    assert -(-n_out // tile) == 3 and n_out % tile == 2
    t0 = time.perf_counter()
    y, want = _exact(gpu, L, M, K, c, n_out, n_in, False, lim=3)
    assert np.count_nonzero(want) > want.size // 2
    # and a 20 000-tap bank that leaves room for a tile of 512
    K = 20000
    assert _geom(L, M, K) == (K, False, 512)
    _exact(gpu, L, M, K, 19000, 515, 700, False, lim=3)
    print(f"K=20435 / 20000 at L=M=1: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("K", [20436, 65536])
def test_generic_bank_does_not_fit(gpu, K):
    """A tap bank that leaves no room for a 64-output window is refused with
    DSP_ENOTSUP before anything is launched."""
    from dspcore import design, ops
    L = M = 1
    assert _geom(L, M, K) == (K, False, None)
    n_in, n_out = 300, 130
    x = torch.ones((3, n_in), dtype=torch.float32, device=gpu)
    taps = torch.ones(K, dtype=torch.float32, device=gpu)
    obuf, out = _view(gpu, 3, n_out, SENTINEL)
    plan = design.SrcPlan(L, M, K, np.ones(K), 20000, n_in, n_out, 0)
    res, names = _traced(lambda: ops.src_polyphase(x, plan, taps=taps, out=out))
    assert isinstance(res, RuntimeError) and "does not fit in LDS" in str(res), res
    assert names == []
    assert bool((obuf == SENTINEL).all())


# --------------------------------------------------------------------------- (b) placement
ALIGNED, SHIFTED, PITCH1 = (0, 0), (1, 0), (0, 1)       # (lead, pad) of _view


def _design(L, M, K):
    """(caller's float32 taps, the library's flushed taps in float64, K) of
    the library's design for the ratio."""
    from dspcore import design
    plan = design.src_plan(4800, 48000, M, L, K)
    assert plan.K == K
    return design.caller_taps(plan), design.kernel_taps(plan).astype(np.float64)


@pytest.mark.parametrize("L,M,K,reg", [(3, 2, 121, True), (160, 147, 1023, False)],
                         ids=["L3M2T41", "L160M147K1023"])
def test_placements_give_one_y(gpu, L, M, K, reg):
    T, _, tile = _geom(L, M, K)
    taps, _ = _design(L, M, K)
    c, n_out = (K - 1) // 2, tile + 6
    n_in = _short_n_in(L, M, T, c, n_out)
    x = np.random.default_rng(31).uniform(-1, 1, (3, n_in)).astype(np.float32)
    flags = {ALIGNED: 1, SHIFTED: 0, PITCH1: 0}
    seen, base = set(), None
    for xl in (ALIGNED, SHIFTED, PITCH1):
        for yl in (ALIGNED, SHIFTED, PITCH1):
            vec = (flags[xl], flags[yl])
            y = _run(gpu, x, taps, L, M, c, n_out, reg, xl=xl, yl=yl, vec=vec)
            seen.add(vec)
            base = y if base is None else base
            assert np.array_equal(_bits(y), _bits(base)), (xl, yl)
    assert seen == {(1, 1), (0, 1), (1, 0), (0, 0)}
    assert np.isfinite(base).all() and np.count_nonzero(base) > base.size // 2
    # a row alone, its padded pitch kept (ops.ld), is the row in the batch
    for b in range(3):
        for yl, vec in ((ALIGNED, (1, 1)), (PITCH1, (1, 0))):
            y1 = _run(gpu, x[b:b + 1], taps, L, M, c, n_out, reg, yl=yl, vec=vec)
            assert np.array_equal(_bits(y1[0]), _bits(base[b])), (b, yl)


# --------------------------------------------------------------------------- (c) rounding
# (L, M, K, register-blocked)
DESIGNS = [(3, 2, 121, True), (3, 2, 255, True), (2, 1, 127, True), (2, 1, 81, True),
           (160, 147, 1023, False), (1, 16, 641, False)]
DESIGN_IDS = ["L3M2K121", "L3M2K255", "L2M1K127", "L2M1K81", "L160M147K1023", "L1M16K641"]


def _bound(x, n_out, ktaps, L, M, c, T):
    return (T + 2) * 2.0 ** -24 * sm.abs_model(x, n_out, ktaps, L, M, c)


def _assert_rounding(y, x, n_out, ktaps, L, M, c, T, what):
    """|y - model| <= (T + 2) 2^-24 sum|h x| for every output; returns the
    worst err / bound."""
    want = sm.src_model(x, n_out, ktaps, L, M, c)
    bound = _bound(x, n_out, ktaps, L, M, c, T)
    err = np.abs(y.astype(np.float64) - want)
    zero = bound == 0
    assert not y[zero].any(), f"{what}: non-zero outputs where sum|h x| is 0"
    worst = float(np.max(err[~zero] / bound[~zero])) if (~zero).any() else 0.0
    print(f"{what}: worst err / bound {worst:.3f} (max err {float(err.max()):.3g})")
    assert bool(np.all(err <= bound)), f"{what}: err / bound {worst:.3f}"
    return worst


@pytest.mark.parametrize("L,M,K,reg", DESIGNS, ids=DESIGN_IDS)
def test_rounding_bound_with_the_designs(gpu, L, M, K, reg):
    T, _, tile = _geom(L, M, K)
    taps, ktaps = _design(L, M, K)
    if L > 1:
        assert np.count_nonzero(ktaps) <= np.count_nonzero(taps)
    c, n_out = (K - 1) // 2, 2 * tile + 10
    assert -(-n_out // tile) == 3
    n_in = -(-n_out * M // L)
    x = np.random.default_rng(K).uniform(-1, 1, (2, n_in)).astype(np.float32)
    y = _run(gpu, x, taps, L, M, c, n_out, reg)
    _assert_rounding(y, x, n_out, ktaps, L, M, c, T, f"L{L}/M{M} K={K}")


# --------------------------------------------------------------------------- (d) non-finite
def _nf_rows(L, M, T, c, tile, n_in, taps):
    """[(position, value)] lists, one per row."""
    vals = [NAN, INF, -INF]
    specs, parities = [], set()
    for m in (tile - 1, tile, tile + 1):
        q = _q(m, L, M, c)
        Q = q - (T - 1)
        parities.add(Q % 2)
        for p in (q, Q, q + 1, q + 2, Q - 1):
            specs.append([(p, vals[len(specs) % 3])])
    assert parities == {0, 1}
    # the two ends of output TILE's window, infs whose products with their
    # taps differ in sign: NaN there
    q, phi = _q(tile, L, M, c), (tile * M + c) % L
    t_last = (taps.size - 1 - phi) // L
    assert t_last >= 1
    specs.append([(q, INF), (q - t_last, -INF if np.sign(taps[phi]) == np.sign(taps[phi + L * t_last]) else INF)])
    specs.append([(0, vals[len(specs) % 3])])
    specs.append([(n_in - 1, vals[len(specs) % 3])])
    specs.append([])
    for sp in specs:
        for p, _ in sp:
            assert 0 <= p < n_in
    return specs


def _assert_nonfinite(gpu, x, clean, taps, ktaps, L, M, c, n_out, reg):
    """y of x has src_model.nf_class's NaN / +inf / -inf masks exactly and is
    elsewhere bitwise y of `clean` (x with the non-finite samples zeroed), which
    is inside the rounding bound.  Returns the classes."""
    T = sm.branch_taps(taps.size, L)
    y = _run(gpu, x, taps, L, M, c, n_out, reg)
    y0 = _run(gpu, clean, taps, L, M, c, n_out, reg)
    assert np.isfinite(y0).all()
    cls = sm.nf_class(x, n_out, taps, L, M, c)
    got = sm.classify(y)
    for code, name in ((sm.NAN_, "NaN"), (sm.PINF, "+inf"), (sm.NINF, "-inf")):
        np.testing.assert_array_equal(got == code, cls == code, err_msg=f"{name} mask")
    fin = cls == sm.FINITE
    differ = fin & (_bits(y) != _bits(y0))
    assert not differ.any(), (f"{np.count_nonzero(differ)} finite outputs differ from the clean "
                              f"row's, first at {np.argwhere(differ)[:6].tolist()}")
    _assert_rounding(y0, clean, n_out, ktaps, L, M, c, T, f"clean rows L{L}/M{M} K={taps.size}")
    return cls


@pytest.mark.parametrize("L,M,K,reg", DESIGNS[:5], ids=DESIGN_IDS[:5])
def test_nonfinite_at_the_src_tile_edges(gpu, L, M, K, reg):
    T, _, tile = _geom(L, M, K)
    taps, ktaps = _design(L, M, K)
    assert bool(np.all(taps != 0))
    c, n_out = (K - 1) // 2, tile + 10
    n_in = _q(n_out - 1, L, M, c) + 1           # the last window ends on the last sample
    specs = _nf_rows(L, M, T, c, tile, n_in, taps)
    B = len(specs)
    t0 = time.perf_counter()
    clean = np.random.default_rng(K + 1).uniform(-0.9, 0.9, (B, n_in)).astype(np.float32)
    x = clean.copy()
    for r, sp in enumerate(specs):
        for p, v in sp:
            x[r, p], clean[r, p] = v, 0.0
    cls = _assert_nonfinite(gpu, x, clean, taps, ktaps, L, M, c, n_out, reg)
    # every sample lies in some output's window (q + 1, q + 2 and Q - 1 in a
    # neighbour's)
    for r, sp in enumerate(specs):
        assert bool((cls[r] != sm.FINITE).any()) == bool(sp), r
    assert cls[-4, tile] == sm.NAN_ and set(np.unique(cls)) == {sm.FINITE, sm.PINF, sm.NINF, sm.NAN_}
    print(f"L{L}/M{M} K={K}: {B} rows, {int((cls != sm.FINITE).sum())} non-finite outputs, "
          f"{time.perf_counter() - t0:.2f} s")


def test_nonfinite_beside_phases_without_a_tap(gpu):
    """K < L: the outputs of phases K .. L-1 meet no tap and stay 0 beside an
    inf or NaN (window_sums must not read a tap for them)."""
    L, M, K = 8, 3, 5
    T, reg, tile = _geom(L, M, K)
    assert T == 1 and not reg
    rng = np.random.default_rng(85)
    taps = rng.uniform(0.2, 1.0, K).astype(np.float32) * np.array([1, -1, 1, 1, -1], np.float32)
    c, n_out, n_in = 2, 600, 230
    clean = rng.uniform(-0.9, 0.9, (4, n_in)).astype(np.float32)
    x = clean.copy()
    for r, v in enumerate((NAN, INF, -INF)):
        for p in (0, 57 + r, 58 + r, n_in - 1):
            x[r, p], clean[r, p] = v, 0.0
    cls = _assert_nonfinite(gpu, x, clean, taps, taps.astype(np.float64), L, M, c, n_out, reg)
    phi = (np.arange(n_out) * M + c) % L
    q = (np.arange(n_out) * M + c) // L
    # outputs of tap-less phases whose only sample is the inf or NaN: finite, and 0
    lone = (phi >= K) & np.isin(q, (57, 58, 59, 60))
    assert lone.sum() >= 4 and not cls[:, phi >= K].any()
    assert set(np.unique(cls)) == {sm.FINITE, sm.PINF, sm.NINF, sm.NAN_}
