"""The one-shot biquad cascade (csrc/iir.hip, dsp_biquad_cascade_f32) at every
load, store and wave variant -- what the parity, stream-edge and wide-batch
files, with their contiguous 16-byte aligned rows, never execute.

1. k_iir_wave<S, P1, VM, NORM, W> for S = 1..8 (7 runs as 8), NORM and a
   b0 == 0 stage, with and without the state table (P1 = 1 / 0), at rows whose
   chunk count C hits 2, 64 | 65, 128 | 129, 256 (W = 1 | 2 | 4) with a last
   chunk of 1, 2, 3, 31 or T samples, rows ending in a partial vector, and
   chunks of two and three tiles; through six layouts (VM 1 / 2 buffer stores,
   VM 0 guarded stores with scalar loads, in place), bitwise one result.
2. clip = 0.
3. The general path (k_iir_prep / k_iir_pass / k_iir_carry): S <= 8 at
   C = 257, S = 9..16 (padded to 12 and 16), vec_x 0 / 1, n % 4 != 0, a batch
   of 257 (two carry blocks), and C == 1 (pass 2 alone) for S = 0..16.
4. The workspace contract: 0 bytes exactly when fused or C <= 1, a workspace
   of exactly the answered size, one byte less refused.
5. inf / NaN at chunk edges through nf_poison, the fused scan and k_iir_carry,
   with the EQ's cascades and with a stage that keeps an inf an inf, whose
   later chunks only nf_poison turns into NaN.
6. Argument errors tests/test_abi.py does not have.

Truth is scipy.signal.sosfilt in float64 over the float32 rows (+ np.clip),
bound EQ_ATOL.  Every chunked result is also held against the same rows run
as one chunk (chunk_len = 32 ceil(n / 32): pass 2 alone) within ONE_CHUNK =
1e-6, tests/test_gpu_parity.py's bound; with clip = 0 both bounds scale with
max(1, |truth|) per sample.  Layouts of one (sos, clip, chunk_len, n,
use_table) differ only in how the same floats are loaded and stored: bitwise.

Rows: uniform(-0.9, 0.9) float32 noise (seed 5), the same row times 8 (it
must clip: max |z| == 1.0) and a second noise row of the same generator plus
a DC offset of 0.15 (the 40 Hz band's state is large at every chunk edge).
For the first and third the share of truth samples with |z| >= 1 is asserted
below 10 %, so the clip cannot hide an error.  (An offset of 0.3 breaks that
cap in the float64 reference alone: 24 % of the first 33 samples and 16 % of
the first 2017 with the five-band cascade, whatever noise row it is added
to; 0.15 on the second row gives 9.1 % at the worst, S = 6 with a b0 == 0
stage over 2047 samples.  Host measurements of sosfilt, no kernel involved.)

Every view is cut from a larger flat buffer: x's from one filled with NaN
(the kernels read pitch padding, it must reach no output), y's from one
filled with a sentinel, and every float outside the B x n window must be
untouched after the call.

odd_pitch is n + 1 for even n and n + 2 for odd n (n + 3 would be even there
and, at n = 33 or 2017, a multiple of 4: not the VM 0 layout it stands for).

Left out on purpose: rows too long for a seconds-scale test (every row here
is shorter than 8200 samples), and the x-state pass (P1 = 2), which the chain
tests own."""
import time

import numpy as np
import pytest
import torch

from test_gpu_stream import EQ_ATOL, FS_EQ, Z_ULP2, _gains
from test_gpu_stream_edges import B0_STAGE, _bits, _cascade, _sosfilt_clip, _traced, _vec

pytestmark = pytest.mark.gpu

ONE_CHUNK = 1e-6          # tests/test_gpu_parity.py: chunked against unchunked
SHARE_CAP = 0.10
AMP, DC, SEED = 0.9, 0.15, 5
N_MAX = 8193
NAN, INF = float("nan"), float("inf")
SENTINEL = 12345.0
FRONT, BACK = 8, 16       # floats before the first row (32 bytes) and after the last
GENERAL = ["iir_prep", "iir_state", "iir_carry", "iir_apply"]
KWAVE, KCBMAX, KNT = 64, 256, 256    # csrc/iir.hip kWave (common.h), kCBMax, kNT


def _ceil(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- rows and truth
_CACHE = {}


def _rows(n):
    """[3, n]: noise, 8 x that noise, other noise + DC -- prefixes of two
    8193-sample rows."""
    if "base" not in _CACHE:
        _CACHE["base"] = np.random.default_rng(SEED).uniform(-AMP, AMP,
                                                             (2, N_MAX)).astype(np.float32)
    key = ("x", n)
    if key not in _CACHE:
        r, r2 = _CACHE["base"][:, :n]
        x = np.stack([r, np.float32(8) * r, r2 + np.float32(DC)]).astype(np.float32)
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def _cascade_any(S, norm):
    """tests/test_gpu_stream_edges.py's cascade up to 8 stages; above, the
    eight bands followed by the same bands at opposite gains (the response
    stays bounded), cut to S stages; norm=False: the last stage has b0 == 0."""
    if S == 0:
        return np.zeros((0, 5))
    if S <= 8:
        return _cascade(S, norm)
    from dspcore import design
    g = dict(_gains())
    g["Air"] = 2.5
    g["Body"] = -1.5
    sos = np.vstack([design.eq_plan(FS_EQ, g).sos,
                     design.eq_plan(FS_EQ, {k: -v for k, v in g.items()}).sos])
    assert sos.shape == (16, 5)
    sos = np.ascontiguousarray(sos[:S]).copy()
    if not norm:
        sos[-1] = B0_STAGE
    assert design.df2_realization(sos)[2] == norm
    return sos


def _truth(sos, n, clip=True):
    """float64 sosfilt of _rows(n) (+ clip), once per sos over the whole
    8193-sample rows: the filter is causal, a prefix's truth is the prefix."""
    key = ("t", sos.tobytes(), bool(clip))
    if key not in _CACHE:
        x = _rows(N_MAX)
        if sos.shape[0] == 0:
            z = x.astype(np.float64)
            z = np.clip(z, -1.0, 1.0) if clip else z
        elif clip:
            z = _sosfilt_clip(sos, x)
        else:
            from scipy.signal import sosfilt
            sos6 = np.column_stack([sos[:, :3], np.ones(sos.shape[0]), sos[:, 3:]])
            z = sosfilt(sos6, x.astype(np.float64), axis=1)
        z.setflags(write=False)
        _CACHE[key] = z
    return _CACHE[key][:, :n]


def _conditions(sos, n, need_clip=True):
    """The rows can show an error: few truth samples of rows 0 and 2 sit on
    the clip, and row 1 does clip (checked on the host, on the truth)."""
    t = _truth(sos, n, True)
    for r in (0, 2):
        share = float(np.mean(np.abs(t[r]) >= 1.0))
        assert share < SHARE_CAP, (sos.shape[0], n, r, share)
    if need_clip:
        assert float(np.max(np.abs(t[1]))) == 1.0, (sos.shape[0], n)


def _errs(z, ref, scaled=False):
    """Worst |z - ref|, per sample over max(1, |ref|) when scaled (clip = 0)."""
    d = np.abs(z.astype(np.float64) - ref)
    if scaled:
        d = d / np.maximum(1.0, np.abs(ref))
    return float(np.max(d)) if d.size else 0.0


# --------------------------------------------------------------------------- layouts
# name: (x pitch, x base offset in floats, y pitch or None = in place)
LAYOUTS = {"aligned": ("a", 0, "a"), "odd_pitch": ("o", 0, "o"), "offset": ("a", 1, "a"),
           "y_odd": ("a", 0, "o"), "in_place": ("a", 0, None), "in_place_odd": ("o", 0, None)}
# (vec_x, vec_y) each realises
VEC = {"aligned": (1, 1), "odd_pitch": (0, 0), "offset": (0, 1), "y_odd": (1, 0),
       "in_place": (1, 1), "in_place_odd": (0, 0)}


def _pitch(kind, n):
    if kind == "a":
        return ((n + 3) & ~3) + 4
    p = n + 1 if n % 2 == 0 else n + 2
    assert p % 2 == 1
    return p


def _view(flat, B, n, pitch, off):
    return torch.as_strided(flat, (B, n), (pitch, 1), FRONT + off)


def _outside_untouched(flat, B, n, pitch, off, fill):
    """Every float of `flat` outside the B x n window still holds `fill`."""
    chk = flat.clone()
    _view(chk, B, n, pitch, off).fill_(fill)
    return bool(torch.equal(_bits(chk), _bits(torch.full_like(chk, fill))))


def _plan(S, n, chunk_len, vec):
    """run_cascade / run_fused's host rules: (fused, C, W, VM, trace names)."""
    Sp = 8 if S == 7 else S
    C = 1 if S == 0 else _ceil(n, chunk_len)
    fused = Sp in (1, 2, 3, 4, 5, 6, 8) and 2 <= C <= KCBMAX
    W = 1 if C <= KWAVE else 2 if C <= 2 * KWAVE else 4
    VM = 0 if not (vec[0] and vec[1]) else 1 if n % 4 == 0 else 2
    names = ["iir_fused"] if fused else ["iir_apply"] if C <= 1 else GENERAL
    return fused, C, W, VM, names


def _call(gpu, layout, x, sos, clip, chunk_len, use_table):
    """x [B, n] (host) through ops.biquad_cascade in `layout`.  Returns
    (z as a contiguous device tensor, (fused, C, W, VM)); asserts the vec
    flags, the trace names and that nothing outside the window was written."""
    from dspcore import ops
    B, n = x.shape
    xk, xoff, yk = LAYOUTS[layout]
    px = _pitch(xk, n)
    xflat = torch.full((FRONT + 1 + B * px + BACK,), NAN, dtype=torch.float32, device=gpu)
    xv = _view(xflat, B, n, px, xoff)
    xv.copy_(torch.from_numpy(np.array(x)).to(gpu))
    if yk is None:
        yflat, yv, py, yoff, fill = xflat, xv, px, xoff, NAN
        before = None
    else:
        py, yoff, fill = _pitch(yk, n), 0, SENTINEL
        yflat = torch.full((FRONT + 1 + B * py + BACK,), fill, dtype=torch.float32, device=gpu)
        yv = _view(yflat, B, n, py, yoff)
        before = xflat.clone()
    vec = (_vec(xv), _vec(yv))
    assert vec == VEC[layout], (layout, n, vec)
    fused, C, W, VM, want = _plan(sos.shape[0], n, chunk_len, vec)
    out, names = _traced(lambda: ops.biquad_cascade(xv, sos, clip, out=yv, chunk_len=chunk_len,
                                                    use_table=use_table))
    assert out is yv and names == want, (layout, n, names, want)
    assert _outside_untouched(yflat, B, n, py, yoff, fill), (layout, n, "stored outside the rows")
    if before is not None:
        assert bool(torch.equal(_bits(xflat), _bits(before))), (layout, n, "x changed")
        assert bool((yv != SENTINEL).all()), (layout, n, "samples left unwritten")
    return yv.clone(memory_format=torch.contiguous_format), (fused, C, W, VM)


def _same(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _one_chunk(gpu, x, sos, clip):
    """The rows as one chunk: pass 2 alone from the zero state."""
    n = x.shape[1]
    z, (fused, C, _, _) = _call(gpu, "aligned", x, sos, clip, 32 * _ceil(n, 32), False)
    assert not fused and C == 1
    return z.cpu().numpy()


# --------------------------------------------------------------------------- 1: the fused kernel
# (n, chunk_len, (C, W, last-chunk length))
FUSED_SHAPES = [(33, 32, (2, 1, 1)), (2017, 32, (64, 1, 1)), (2048, 32, (64, 1, 32)),
                (2049, 32, (65, 2, 1)), (4096, 32, (128, 2, 32)), (4097, 32, (129, 4, 1)),
                (8161, 32, (256, 4, 1)), (8192, 32, (256, 4, 32)),
                # rows ending in a partial vector
                (2018, 32, (64, 1, 2)), (2047, 32, (64, 1, 31)), (4099, 32, (129, 4, 3)),
                (6145, 32, (193, 4, 1)),
                # chunks of two and three tiles: the prefetch loop
                (4097, 64, (65, 2, 1)), (6145, 96, (65, 2, 1))]
# VM of each layout, by n % 4 == 0
FUSED_VM = {"aligned": (2, 1), "odd_pitch": (0, 0), "offset": (0, 0), "y_odd": (0, 0),
            "in_place": (2, 1), "in_place_odd": (0, 0)}


def test_fused_shapes_cover_every_edge():
    """The shape list realises what it is there for (host arithmetic only)."""
    geo = {(n, T): g for n, T, g in FUSED_SHAPES}
    for (n, T), (C, W, last) in geo.items():
        assert C == _ceil(n, T) and last == n - (C - 1) * T, (n, T)
        assert W == (1 if C <= 64 else 2 if C <= 128 else 4) and 2 <= C <= 256
    Cs = {g[0] for g in geo.values()}
    assert Cs >= {2, 64, 65, 128, 129, 256}
    assert {n % 4 for n, _ in geo} == {0, 1, 2, 3}
    assert {g[2] for (n, T), g in geo.items() if T == 32} >= {1, 2, 3, 31, 32}
    assert {T // 32 for _, T in geo} == {1, 2, 3}
    assert max(n for n, _ in geo) < 8200


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "b0"])
@pytest.mark.parametrize("S", range(1, 9))
def test_fused_every_instantiation_at_every_edge(gpu, S, norm):
    t0 = time.perf_counter()
    sos = _cascade(S, norm)
    table_used = norm and S != 7        # run_fused: P1 = 1 only for NORM with a table of S stages
    worst_t = worst_c = worst_p = 0.0
    launches = 0
    for n, T, (C, W, last) in FUSED_SHAPES:
        _conditions(sos, n)
        x = _rows(n)
        truth = _truth(sos, n)
        one = _one_chunk(gpu, x, sos, True)
        z_by_table = {}
        for use_table in (True, False):
            za, got = _call(gpu, "aligned", x, sos, True, T, use_table)
            assert got == (True, C, W, 1 if n % 4 == 0 else 2), (n, T, got)
            z = za.cpu().numpy()
            et, ec = _errs(z, truth), _errs(z, one)
            worst_t, worst_c = max(worst_t, et), max(worst_c, ec)
            assert et <= EQ_ATOL, (n, T, use_table, et)
            assert ec <= ONE_CHUNK, (n, T, use_table, ec)
            assert float(np.max(np.abs(z[1]))) == 1.0
            for layout in LAYOUTS:
                if layout == "aligned":
                    continue
                zl, got = _call(gpu, layout, x, sos, True, T, use_table)
                assert got == (True, C, W, FUSED_VM[layout][n % 4 == 0]), (layout, n, T, got)
                assert _same(zl, za), (layout, n, T, use_table)
            launches += len(LAYOUTS)
            z_by_table[use_table] = z
        if table_used:
            ep = _errs(z_by_table[True], z_by_table[False].astype(np.float64))
            worst_p = max(worst_p, ep)
            assert ep <= Z_ULP2, (n, T, ep)
        else:       # the table is ignored: one kernel, one result
            assert np.array_equal(_bits(z_by_table[True]), _bits(z_by_table[False])), (n, T)
    print(f"fused S={S} {'NORM' if norm else 'b0'}: vs sosfilt {worst_t:.3g} (tol {EQ_ATOL:g}), vs "
          f"one chunk {worst_c:.3g} (tol {ONE_CHUNK:g}), table vs cascade pass 1 {worst_p:.3g} "
          f"(tol {Z_ULP2:g}); {launches} fused launches, {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 2: clip = 0
@pytest.mark.parametrize("S", [1, 6, 8])
def test_fused_without_clip(gpu, S):
    t0 = time.perf_counter()
    sos = _cascade(S, True)
    worst_t = worst_c = 0.0
    for n in (2049, 8161):
        _conditions(sos, n)
        x = _rows(n)
        truth = _truth(sos, n, clip=False)
        assert float(np.max(np.abs(truth[1]))) > 1.0
        one = _one_chunk(gpu, x, sos, False)
        for use_table in (True, False):
            za, got = _call(gpu, "aligned", x, sos, False, 32, use_table)
            assert got[0] and got[3] == 2
            z = za.cpu().numpy()
            assert float(np.max(np.abs(z[1]))) > 1.0
            et, ec = _errs(z, truth, scaled=True), _errs(z, one.astype(np.float64), scaled=True)
            worst_t, worst_c = max(worst_t, et), max(worst_c, ec)
            assert et <= EQ_ATOL, (n, use_table, et)
            assert ec <= ONE_CHUNK, (n, use_table, ec)
            zo, got = _call(gpu, "odd_pitch", x, sos, False, 32, use_table)
            assert got[0] and got[3] == 0
            assert _same(zo, za), (n, use_table)
    print(f"clip = 0, S={S}: vs sosfilt {worst_t:.3g} (tol {EQ_ATOL:g} max(1,|z|)), vs one chunk "
          f"{worst_c:.3g} (tol {ONE_CHUNK:g} max(1,|z|)); {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 3: the general path
GENERAL_LAYOUTS = ["aligned", "odd_pitch", "offset", "y_odd", "in_place"]
GENERAL_CASES = ([(S, norm, (8193,)) for S in (1, 6, 8) for norm in (True, False)]
                 + [(S, norm, (33, 2047, 8193)) for S in (9, 12, 13, 16) for norm in (True, False)])


@pytest.mark.parametrize("S,norm,lengths", GENERAL_CASES,
                         ids=[f"S{s}-{'norm' if m else 'b0'}" for s, m, _ in GENERAL_CASES])
def test_general_path(gpu, S, norm, lengths):
    t0 = time.perf_counter()
    sos = _cascade_any(S, norm)
    worst_t = worst_c = 0.0
    for n in lengths:
        _conditions(sos, n)
        x = _rows(n)
        truth = _truth(sos, n)
        C = _ceil(n, 32)
        assert S > 8 or C == 257
        one = _one_chunk(gpu, x, sos, True)
        za, got = _call(gpu, "aligned", x, sos, True, 32, True)
        assert got[:2] == (False, C)            # _call asserted the four launches
        z = za.cpu().numpy()
        et, ec = _errs(z, truth), _errs(z, one)
        worst_t, worst_c = max(worst_t, et), max(worst_c, ec)
        assert et <= EQ_ATOL, (n, et)
        assert ec <= ONE_CHUNK, (n, ec)
        assert float(np.max(np.abs(z[1]))) == 1.0
        for layout in GENERAL_LAYOUTS[1:]:
            zl, got = _call(gpu, layout, x, sos, True, 32, True)
            assert got[:2] == (False, C)
            assert _same(zl, za), (layout, n)
    print(f"general S={S} {'NORM' if norm else 'b0'}: vs sosfilt {worst_t:.3g} (tol {EQ_ATOL:g}), "
          f"vs one chunk {worst_c:.3g} (tol {ONE_CHUNK:g}); {time.perf_counter() - t0:.2f} s")


def test_general_path_batch_257(gpu):
    """Two k_iir_carry blocks (the second with one live lane), B C no
    multiple of the pass kernel's 256 lanes: every row bitwise its row of the
    3-row run."""
    t0 = time.perf_counter()
    S, n, B = 16, 8193, 257
    C = _ceil(n, 32)
    assert _ceil(B, 256) == 2 and (B * C) % KNT
    sos = _cascade_any(S, True)
    x3 = _rows(n)
    z3, got = _call(gpu, "aligned", x3, sos, True, 32, True)
    assert got[:2] == (False, C)
    idx = np.arange(B) % 3
    zw, got = _call(gpu, "aligned", x3[idx], sos, True, 32, True)
    assert got[:2] == (False, C)
    want = z3[torch.from_numpy(idx).to(gpu)]
    bad = (~(_bits(zw) == _bits(want)).all(dim=1)).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} rows differ from their base rows: {bad[:12].tolist()}"
    print(f"general S={S} B={B}: {time.perf_counter() - t0:.2f} s")


# (n, chunk_len)
ONE_CHUNK_SHAPES = [(1, 32), (31, 32), (32, 32), (100, 128)]


@pytest.mark.parametrize("S", [0, 1, 7, 8, 9, 16])
def test_single_chunk_rows(gpu, S):
    """C == 1, the path of every row with n <= chunk_len: pass 2 alone."""
    t0 = time.perf_counter()
    worst = 0.0
    for norm in ((True,) if S == 0 else (True, False)):
        sos = _cascade_any(S, norm)
        for n, T in ONE_CHUNK_SHAPES:
            x = _rows(n)
            for clip in (True, False):
                truth = _truth(sos, n, clip)
                za, got = _call(gpu, "aligned", x, sos, clip, T, True)
                assert got[:2] == (False, 1)    # _call asserted ["iir_apply"]
                z = za.cpu().numpy()
                if S == 0:
                    assert np.array_equal(_bits(z), _bits(truth.astype(np.float32))), (n, clip)
                e = _errs(z, truth, scaled=not clip)
                worst = max(worst, e)
                assert e <= EQ_ATOL, (n, T, clip, e)
                zo, _ = _call(gpu, "odd_pitch", x, sos, clip, T, True)
                assert _same(zo, za), (n, T, clip)
    print(f"single chunk S={S}: vs sosfilt {worst:.3g} (tol {EQ_ATOL:g}); "
          f"{time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 4: the workspace
def test_workspace_is_zero_exactly_when_fused_or_single_chunk():
    from dspcore import _lib
    lib = _lib.load()
    for S in range(0, 17):
        for n, T in [(33, 32), (2048, 32), (8192, 32), (8193, 32), (32, 32), (100, 128),
                     (8193, 64), (8193, 8224)]:
            fused, C, _, _, _ = _plan(S, n, T, (1, 1))
            if 9 <= S:
                assert not fused
            need = int(lib.dsp_biquad_workspace_bytes(3, n, S, T))
            assert (need == 0) == (fused or C <= 1), (S, n, T, need)


def _raw_cascade(xd, yd, sos, chunk_len, ws_ptr, ws_bytes, S=None, ld_x=None, ld_y=None):
    """(status, dsp_last_error's text) of the C entry point on xd, yd as they
    lie (the text is read at once: a later call that succeeds clears it)."""
    from dspcore import _lib
    B, n = xd.shape
    with torch.cuda.device(xd.device):
        rc = _lib.load().dsp_biquad_cascade_f32(
            xd.data_ptr(), yd.data_ptr(), B, n, xd.stride(0) if ld_x is None else ld_x,
            yd.stride(0) if ld_y is None else ld_y, _lib.sos_pointer(sos),
            sos.shape[0] if S is None else S, 1, chunk_len, None, ws_ptr, ws_bytes,
            torch.cuda.current_stream(xd.device).cuda_stream)
        return rc, (_lib.last_error() if rc else "")


@pytest.mark.parametrize("S,n", [(6, 8193), (16, 2047)])
def test_workspace_of_exactly_the_required_size(gpu, S, n):
    from dspcore import _lib
    lib = _lib.load()
    sos = _cascade_any(S, True)
    x = _rows(n)
    B = x.shape[0]
    need = int(lib.dsp_biquad_workspace_bytes(B, n, S, 32))
    assert need > 0
    want, got = _call(gpu, "aligned", x, sos, True, 32, False)
    assert not got[0]
    xd = torch.from_numpy(np.array(x)).to(gpu)
    yd = torch.full_like(xd, SENTINEL)
    guard = 4096
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=gpu)
    # one byte less: refused before any launch
    (rc, err), names = _traced(lambda: _raw_cascade(xd, yd, sos, 32, ws.data_ptr(), need - 1))
    assert rc == _lib.DSP_EINVAL and "workspace too small" in err and names == [], (rc, err, names)
    assert bool((yd == SENTINEL).all()) and bool((ws == 0xA5).all())
    (rc, err), names = _traced(lambda: _raw_cascade(xd, yd, sos, 32, ws.data_ptr(), need))
    assert rc == _lib.DSP_OK and names == GENERAL, (rc, err, names)
    assert _same(yd, want)
    assert bool((ws[need:] == 0xA5).all()), "wrote past the workspace it asked for"
    assert not bool((ws[:need] == 0xA5).all())


# --------------------------------------------------------------------------- 5: inf / NaN
# One stage with poles at 0.5 and -0.2 and every product of the recursion
# positive (-a1, -a2, b1 / b0, b2 / b0 > 0): after a +inf its state and output
# stay +inf, no inf - inf ever makes a NaN of them, and the clip would turn the
# later chunks into +1 -- there only nf_poison makes them NaN.  (The EQ's
# peaking sections reach NaN by themselves within two samples.)
SUM_STAGE = np.array([[1.0, 0.5, 0.25, -0.3, -0.1]])
# (cascade, use_table, n): fused with and without the table, a b0 stage, the general path
NF_CASES = {"S6-table": ((6, True), True, 4097), "S6-cascade": ((6, True), False, 4097),
            "S6-b0": ((6, False), True, 4097), "S9-general": ((9, True), True, 8193),
            "sum-table": (SUM_STAGE, True, 4097), "sum-cascade": (SUM_STAGE, False, 4097),
            "sum-general": (SUM_STAGE, True, 8193)}


@pytest.mark.parametrize("case", list(NF_CASES))
def test_nonfinite_input_at_chunk_edges(gpu, case):
    """nf_poison's hand-off: a chunk that held an inf or NaN hands NaN on."""
    cascade, use_table, n = NF_CASES[case]
    sos = cascade if isinstance(cascade, np.ndarray) else _cascade_any(*cascade)
    S = sos.shape[0]
    t0 = time.perf_counter()
    clean = np.random.default_rng(SEED + 1).uniform(-AMP, AMP, (5, n)).astype(np.float32)
    poison = [(31, NAN), (32, NAN), (n - 1, NAN), (40, INF)]    # row r: (position, value)
    assert 31 // 32 == 0 and 32 // 32 == 1 and (n - 1) // 32 == _ceil(n, 32) - 1 and 40 // 32 == 1
    x = clean.copy()
    for r, (p, v) in enumerate(poison):
        x[r, p] = v
    zc_d, got_c = _call(gpu, "aligned", clean, sos, True, 32, use_table)
    zp_d, got_p = _call(gpu, "aligned", x, sos, True, 32, use_table)
    assert got_c == got_p and got_c[0] == (S <= 8 and n == 4097)
    zc, zp = zc_d.cpu().numpy(), zp_d.cpu().numpy()
    assert np.isfinite(zc).all()
    assert _errs(zc, _sosfilt_clip(sos, clean)) <= EQ_ATOL
    for r, (p, v) in enumerate(poison):
        assert np.array_equal(_bits(zp[r, :p]), _bits(zc[r, :p])), (r, "changed before the sample")
        if np.isnan(v):
            assert np.isnan(zp[r, p:]).all(), (r, np.nonzero(~np.isnan(zp[r, p:]))[0][:8] + p)
        else:   # inside its own chunk the recursion may hold infinities (the clip: +-1)
            later = 32 * (p // 32 + 1)
            assert np.isnan(zp[r, later:]).all(), (r, np.nonzero(~np.isnan(zp[r, later:]))[0][:8])
    assert np.array_equal(_bits(zp[4]), _bits(zc[4])), "the clean row changed"
    # loads and stores of another kind carry the same bits, NaNs included
    zo, _ = _call(gpu, "odd_pitch", x, sos, True, 32, use_table)
    assert _same(zo, zp_d)
    print(f"non-finite {case}: {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- 6: argument errors
def test_argument_errors_leave_y_untouched(gpu):
    """What tests/test_abi.py does not refuse already (it has S = 17 and a
    chunk_len that is no multiple of 32, with null pointers)."""
    from dspcore import _lib
    n = 8193
    sos = _cascade_any(6, True)
    xd = torch.from_numpy(np.array(_rows(n))).to(gpu)
    yd = torch.full_like(xd, SENTINEL)
    ws = torch.zeros(int(_lib.load().dsp_biquad_workspace_bytes(3, n, 6, 32)), dtype=torch.uint8,
                     device=gpu)
    assert ws.numel() > 0
    bad = {"chunk_len 0": (dict(chunk_len=0), "chunk_len"),
           "chunk_len 31": (dict(chunk_len=31), "chunk_len"),
           "chunk_len 48": (dict(chunk_len=48), "chunk_len"),
           "ld_y < n": (dict(ld_y=n - 1), "leading dimension"),
           "ld_x < n": (dict(ld_x=n - 1), "leading dimension"),
           "S = 17": (dict(S=17), "S=17"),
           "null workspace": (dict(ws_ptr=None), "null workspace")}
    for what, (kw, msg) in bad.items():
        args = dict(chunk_len=32, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel())
        args.update(kw)
        (rc, err), names = _traced(lambda: _raw_cascade(xd, yd, sos, **args))
        assert rc == _lib.DSP_EINVAL and names == [], (what, rc, names)
        assert msg in err, (what, err)
        assert bool((yd == SENTINEL).all()), what
    # and the same call with nothing wrong runs
    rc, err = _raw_cascade(xd, yd, sos, 32, ws.data_ptr(), ws.numel())
    assert rc == _lib.DSP_OK and bool((yd != SENTINEL).all()), (rc, err)
