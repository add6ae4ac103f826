"""Fast convolution on the GPU (include/dspcore_fastconv.h, csrc/fft_conv.hip
k_fastconv, dspcore.fastconv.FastConv, modules.dsp_core.convolucion_rapida),
through the C ABI and the class.

Sizes N = 64, 512, 4096, 16384: Plan<log2 N> packs 64, 8, 1 and 1 transforms
per workgroup at 4, 32, 256 and 1024 threads per transform.  K = 1, 2,
N/4 + 1, N/2, N/2 + 1; offset 0, (K - 1)/2, K - 1; rows of 1, V - 1, V, V + 1,
2 V, 2 V + 1 and 3 V + 5 samples (V = N - (K - 1)), n_out = n_in and the full
length.  Cases and the numpy model are tests/fastconv_model.py's.

The C-ABI harness (_call) keeps 1.0e3 in everything the kernel must not read
(x's padding and lead columns, hist_in past K - 1) and in hist_out, the
sentinel bits 0xCAFEF00D in y's padding, and checks after every call that the
sentinels are intact and that hist_out[:K - 1] is bitwise the last K - 1
samples of (history | row).  Rows sit at an odd pitch unless a test says
otherwise, so consecutive rows start at every 4-byte residue.

Reference: float64 np.convolve of the float32 data; bound 2e-6 * ||taps||_2 *
max|x| (fastconv_model.BOUND_REL).  Every case prints its worst error / bound
ratio, the direct kernel's (dsp_src_polyphase_f32, L = M = 1) beside it.
Largest ratio measured on an MI355X: 0.436 (stream cuts, N = 16384, K = 4097);
values per size 0.19, 0.38, 0.37, 0.40; the direct kernel 1.34 at K = 8193.
"""
import numpy as np
import pytest
import torch

import fastconv_model as fm
from conv_gpu_helpers import SENT, YSENT, _bits, _design, _direct, _ops, _tail

pytestmark = pytest.mark.gpu


def _plan(taps, N):
    return _design().fastconv_plan(taps, log2n=N.bit_length() - 1)


def _call(gpu, x, plan, offset=0, n_out=None, hist=None, odd=1, lead=0, tag=""):
    """dsp_fastconv_f32 on the rows of x [B, n] (device float32) with the
    sentinel harness; returns (y [B, n_out], hist_out [B, K - 1])."""
    from dspcore import _lib
    lib = _lib.load()
    B, n = x.shape
    K, k1 = plan.K, plan.K - 1
    n_out = n if n_out is None else n_out
    pitch = (lambda w: (w + 4) | 1) if odd else (lambda w: (w + 7) & ~3)
    ldx, ldy, ldh = pitch(n + lead), pitch(n_out), pitch(k1)
    xb = torch.full((B, ldx), SENT, dtype=torch.float32, device=gpu)
    xb[:, lead:lead + n] = x
    yb = torch.full((B, ldy), YSENT, dtype=torch.int32, device=gpu)
    hin = torch.full((B, ldh), SENT, dtype=torch.float32, device=gpu)
    if hist is not None:
        hin[:, :k1] = hist
    hout = torch.full((B, ldh), SENT, dtype=torch.float32, device=gpu)
    taps, hf, tw = _ops().fastconv_tables(plan, gpu)
    rc = lib.dsp_fastconv_f32(
        xb.data_ptr() + 4 * lead, yb.data_ptr(), B, n, ldx, n_out, ldy, offset,
        hin.data_ptr() if hist is not None else None, hout.data_ptr(), ldh, taps.data_ptr(), K,
        hf.data_ptr(), plan.log2n, tw.data_ptr(), torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, (tag, _lib.last_error())
    assert bool((yb[:, n_out:] == YSENT).all()), (tag, "y's padding written")
    assert bool((hout[:, k1:] == SENT).all()), (tag, "hist_out past K - 1 written")
    want = _tail(hist, x, k1)
    assert torch.equal(_bits(hout[:, :k1]), _bits(want)), (tag, "hist_out")
    if hist is not None:
        assert torch.equal(_bits(hin[:, :k1]), _bits(hist)) and bool((hin[:, k1:] == SENT).all())
    return yb[:, :n_out].view(torch.float32).clone(), hout[:, :k1].clone()


# --------------------------------------------------------------------------- values
@pytest.mark.parametrize("N", fm.SIZES)
@pytest.mark.parametrize("ki", range(5))
def test_values_against_float64_convolve(gpu, N, ki):
    """Every row length, offset and both n_out for one (N, K): the nine rows
    (five impulses of amplitude 1, which return the taps; two tones; noise)
    within the bound of float64 np.convolve."""
    K = fm.tap_counts(N)[ki]
    taps = fm.make_taps(K)
    plan = _plan(taps, N)
    assert plan.hop == N - (K - 1)
    worst = worst_direct = 0.0
    for n in fm.row_lengths(N, K):
        x = fm.make_rows(N, K, n)
        ref = fm.full_reference(x, taps)
        b = fm.bound(taps, x)
        xd = torch.from_numpy(x.copy()).to(gpu)
        for off in fm.offsets(K):
            for n_out in sorted({n, n + K - 1 - off}):
                tag = f"N={N} K={K} n={n} off={off} n_out={n_out}"
                y, _ = _call(gpu, xd, plan, off, n_out, tag=tag)
                want = ref[:, off:off + n_out]
                yn = y.cpu().numpy()
                err = np.abs(yn.astype(np.float64) - want)
                d = _direct(xd, taps, off, n_out).cpu().numpy().astype(np.float64)
                worst_direct = max(worst_direct, float(np.max(np.abs(d - want))) / b)
                worst = max(worst, float(np.max(err)) / b)
                assert np.max(err) <= b, (tag, float(np.max(err)) / b,
                                          np.unravel_index(np.argmax(err), err.shape))
                # the impulse rows return the taps (the same bound)
                for r, p in enumerate(fm.impulse_positions(N, K, n)):
                    m = np.arange(n_out)
                    t = m + off - p
                    imp = np.where((t >= 0) & (t < K), taps[np.clip(t, 0, K - 1)], 0.0)
                    assert np.max(np.abs(yn[r] - imp)) <= b, (tag, "impulse", r)
    print(f"[fastconv] values N={N} K={K}: worst err / bound = {worst:.3f} "
          f"(direct kernel {worst_direct:.3f})")


# --------------------------------------------------------------------------- rows
@pytest.mark.parametrize("N", fm.SIZES)
def test_rows_do_not_depend_on_the_batch_or_the_layout(gpu, N):
    """Each row alone, the batch reversed, aligned rows and a column-offset
    view: bitwise the odd-pitch batch's rows."""
    K = N // 4 + 1
    V = N - (K - 1)
    n = 3 * V + 5
    off = (K - 1) // 2
    plan = _plan(fm.make_taps(K), N)
    x = torch.from_numpy(fm.make_rows(N, K, n).copy()).to(gpu)
    y, _ = _call(gpu, x, plan, off, tag=f"batch N={N}")
    for r in range(x.shape[0]):
        one, _ = _call(gpu, x[r:r + 1], plan, off, tag=f"row {r} N={N}")
        assert torch.equal(_bits(one), _bits(y[r:r + 1])), (N, r)
    rev, _ = _call(gpu, x.flip(0), plan, off, tag=f"reversed N={N}")
    assert torch.equal(_bits(rev.flip(0)), _bits(y)), N
    al, _ = _call(gpu, x, plan, off, odd=0, tag=f"aligned N={N}")
    assert torch.equal(_bits(al), _bits(y)), N
    for lead in (1, 2, 3):
        v, _ = _call(gpu, x, plan, off, odd=lead & 1, lead=lead, tag=f"view {lead} N={N}")
        assert torch.equal(_bits(v), _bits(y)), (N, lead)
    # no output asked for: the history is still written (_call checks it)
    e, h = _call(gpu, x[:, :7], plan, off, n_out=0, tag=f"n_out 0 N={N}")
    assert e.shape == (x.shape[0], 0) and h.shape == (x.shape[0], K - 1)
    # through the operator, on a column-offset view of a wider tensor
    wide = torch.full((x.shape[0], n + 7), SENT, dtype=torch.float32, device=gpu)
    wide[:, 3:3 + n] = x
    o = _ops().fastconv(wide[:, 3:3 + n], plan, off)
    assert torch.equal(_bits(o), _bits(y)), N


def test_pairs_of_one_row_straddle_workgroups(gpu):
    """N = 64 packs 64 transforms per workgroup: 51 rows of 3 pairs are 153
    transforms in 3 workgroups, the last with dead transforms, and rows whose
    pairs lie in two workgroups; every row is bitwise its base row."""
    N, K = 64, 17
    V = N - (K - 1)
    n = 5 * V + 1
    plan = _plan(fm.make_taps(K), N)
    base = torch.from_numpy(fm.make_rows(N, K, n).copy()).to(gpu)
    B = 51
    assert -(-n // (2 * V)) == 3 and fm.TPB[N] % 3 != 0 and B * 3 > 2 * fm.TPB[N]
    idx = torch.arange(B, device=gpu) % base.shape[0]
    narrow, _ = _call(gpu, base, plan, 0, tag="base")
    wide, _ = _call(gpu, base[idx], plan, 0, tag="wide")
    same = (_bits(wide) == _bits(narrow)[idx]).all(1)
    assert bool(same.all()), torch.nonzero(~same).flatten()[:8].tolist()


# --------------------------------------------------------------------------- stream
def _stream(gpu, x, plan, cuts, lead=lambda i: 0, odd=1, tag=""):
    """x [B, n] through the C ABI block by block, the history chained."""
    outs, pos, hist = [], 0, None
    for i, c in enumerate(cuts):
        y, hist = _call(gpu, x[:, pos:pos + c], plan, 0, c, hist, odd, lead(i), f"{tag} call {i}")
        outs.append(y)
        pos += c
    assert pos == x.shape[1]
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("N", fm.SIZES)
@pytest.mark.parametrize("kk", ("quarter", "half"))
def test_stream_cuts(gpu, N, kk):
    """Cuts at multiples of 2 V are bitwise the one call; ragged, reversed and
    view cuts (zero-length and 1-sample pushes included) are within the bound;
    hist_out is checked after every call (_call)."""
    K = N // 4 + 1 if kk == "quarter" else N // 2 + 1
    V = N - (K - 1)
    taps = fm.make_taps(K)
    plan = _plan(taps, N)
    sizes = [0, 1, V - 1, V, V + 1, 2 * V, 2 * V + 5]
    n = sum(sizes)
    x = np.random.default_rng(N + K).uniform(-1, 1, (5, n)).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    ref = fm.full_reference(x, taps)[:, :n]
    b = fm.bound(taps, x)
    one = _stream(gpu, xd, plan, [n], tag=f"one N={N}")
    for cuts in ([2 * V, 4 * V, n - 6 * V], [4 * V, 2 * V, n - 6 * V], [6 * V, n - 6 * V]):
        got = _stream(gpu, xd, plan, cuts, tag=f"2V cuts N={N}")
        assert torch.equal(_bits(got), _bits(one)), (N, K, cuts)
    worst = float(np.max(np.abs(one.cpu().numpy() - ref))) / b
    for name, cuts, lead in (("ragged", sizes, lambda i: 0), ("reversed", sizes[::-1], lambda i: 0),
                             ("views", [V + 1, 2 * V + 5, 0, V - 1, 1, 2 * V, V],
                              lambda i: 1 + i % 3)):
        got = _stream(gpu, xd, plan, cuts, lead, tag=f"{name} N={N}")
        err = float(np.max(np.abs(got.cpu().numpy() - ref)))
        worst = max(worst, err / b)
        assert err <= b, (N, K, name, err / b)
    print(f"[fastconv] stream N={N} K={K}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("N", (64, 4096))
def test_class_stream_state_and_modes(gpu, N):
    """FastConv.push over ragged cuts is bitwise the C-ABI stream with the same
    cuts (the class has aligned rows); a state_dict round trip continues
    bitwise; the one-shot modes are np.convolve's."""
    from dspcore.fastconv import FastConv
    K = N // 4 + 1
    V = N - (K - 1)
    taps = fm.make_taps(K)
    plan = _plan(taps, N)
    sizes = [0, 1, V - 1, V, V + 1, 2 * V, 2 * V + 5]
    n = sum(sizes)
    x = np.random.default_rng(N + K).uniform(-1, 1, (5, n)).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    abi = _stream(gpu, xd, plan, sizes, tag=f"class N={N}")
    fc = FastConv(taps, batch=5, max_block=2 * V + 5, log2n=plan.log2n, device=gpu)
    assert (fc.K, fc.n_fft, fc.hop, fc.latency) == (K, N, V, (K - 1) / 2)
    outs, pos, cut = [], 0, 4
    for i, c in enumerate(sizes):
        if i == cut:
            sd = fc.state_dict()
            assert sd["samples"] == pos and sd["hist"].shape == (5, K - 1)
        y = fc.push(xd[:, pos:pos + c])
        assert y.shape == (5, c)
        outs.append(y.clone())
        pos += c
    assert fc.samples == n
    assert torch.equal(_bits(torch.cat(outs, dim=1)), _bits(abi))
    other = FastConv(taps, batch=5, max_block=2 * V + 5, log2n=plan.log2n, device=gpu)
    other._hist.fill_(SENT)                             # nothing but the state is read
    other.load_state_dict(sd)
    pos = sum(sizes[:cut])
    for i, c in enumerate(sizes[cut:]):
        assert torch.equal(_bits(other.push(xd[:, pos:pos + c])), _bits(outs[cut + i])), i
        pos += c
    other.reset()
    assert torch.equal(_bits(other.push(xd[:, :1])), _bits(outs[1]))
    with pytest.raises(ValueError):
        FastConv(taps, batch=4, log2n=plan.log2n, device=gpu).load_state_dict(sd)
    for bad in (xd[:4, :8], xd[:, :2 * V + 6], xd[:, :8].double(), xd[0, :8], xd[:, :8].cpu()):
        with pytest.raises(ValueError):
            fc.push(bad)
    # one-shot, leaving the stream state alone
    before = fc.state_dict()["hist"]
    b = fm.bound(taps, x)
    for mode in ("causal", "same", "full"):
        for m in (n, K - 3):
            got = fc(xd[:, :m], mode).cpu().numpy()
            for r in range(5):
                full = np.convolve(x[r, :m].astype(np.float64), taps.astype(np.float64))
                want = full[:m] if mode == "causal" else np.convolve(
                    x[r, :m].astype(np.float64), taps.astype(np.float64), mode)
                assert got[r].shape == want.shape, (mode, m)
                assert np.max(np.abs(got[r] - want)) <= b, (N, mode, m, r)
    assert torch.equal(fc.state_dict()["hist"], before)
    with pytest.raises(ValueError):
        fc(xd, "valid")


def test_a_push_is_one_launch_and_replays_from_a_graph(gpu):
    """One push is the one `fastconv` launch; captured into a graph it replays
    bitwise."""
    from dspcore.fastconv import FastConv
    from test_gpu_parity import _traced
    N, K = 512, 129
    V = N - (K - 1)
    taps = fm.make_taps(K)
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 2 * V + 9))
                         .astype(np.float32)).to(gpu)
    fc = FastConv(taps, batch=3, max_block=x.shape[1], log2n=9, device=gpu)
    (y0,), names = _traced(lambda: (fc.push(x),))
    assert names == ["fastconv"], names
    h0 = fc.state_dict()["hist"]
    (e,), names = _traced(lambda: (fc.push(x[:, :0]),))
    assert names == ["fastconv"] and e.shape == (3, 0), names
    assert torch.equal(fc.state_dict()["hist"], h0)      # an empty push keeps the history
    x_static = x.clone()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream(gpu)
    cap.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(cap):
        fc.push(x_static)
        fc.reset()                                       # the warm-up moved the state
        with torch.cuda.graph(graph, stream=cap):
            y = fc.push(x_static)
    torch.cuda.current_stream(gpu).wait_stream(cap)
    torch.cuda.synchronize(gpu)
    for _ in range(2):
        y.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(_bits(y), _bits(y0))
        assert torch.equal(fc.state_dict()["hist"], h0)


# --------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("N,zero_tap", [(N, z) for N in fm.SIZES for z in (True, False)
                                        if z or N < 16384])   # (the largest: one tap set)
def test_non_finite_samples_get_convolves_classes(gpu, N, zero_tap):
    """+inf, -inf, NaN and a +inf / -inf pair in one window, at the first
    sample, on either side of a block seam and at the last sample.  Every
    output of a transform that holds such a sample has the class np.convolve
    gives in float64 (one tap set has an exact zero: inf * 0 = NaN) and, where
    finite, is within the bound; every other output is bitwise the run with
    the bad samples replaced by 0."""
    K = N // 4 + 1
    V = N - (K - 1)
    n = 3 * V + 5
    off = (K - 1) // 2 if zero_tap else 0
    n_out = n if zero_tap else n + K - 1
    taps = fm.make_taps(K, K // 3 if zero_tap else None)
    assert (taps == 0).any() == zero_tap
    plan = _plan(taps, N)
    clean = fm.make_rows(N, K, n)[7]
    inf = np.float32(np.inf)
    kinds = [(inf,), (-inf,), (np.float32(np.nan),), (inf, -inf)]
    pos = [0, V - 1, V, n - 1]
    rows, where = [clean.copy()], [[]]
    for p in pos:
        for kind in kinds:
            r = clean.copy()
            ps = [p] if len(kind) == 1 else ([p, p + 1] if p + 1 < n else [p - 1, p])
            for q, v in zip(ps, kind):
                r[q] = v
            rows.append(r)
            where.append(ps)
    x = np.stack(rows)
    x0 = np.where(np.isfinite(x), x, np.float32(0))
    with np.errstate(all="ignore"):
        ref = np.stack([np.convolve(r.astype(np.float64), taps.astype(np.float64)) for r in x])
    ref = ref[:, off:off + n_out]
    b = fm.bound(taps, x0)
    got, _ = _call(gpu, torch.from_numpy(x).to(gpu), plan, off, n_out, tag=f"nf N={N}")
    zer, _ = _call(gpu, torch.from_numpy(x0).to(gpu), plan, off, n_out, tag=f"nf0 N={N}")
    got, zer = got.cpu().numpy(), zer.cpu().numpy()
    # which outputs belong to a transform that loads a bad sample
    pairs = -(-n_out // (2 * V))
    blocks = -(-n_out // V)
    held = np.zeros((x.shape[0], n_out), dtype=bool)
    for r, ps in enumerate(where):
        for q in range(pairs):
            lo = 2 * q * V + off - (K - 1)
            hi = lo + N + (V if 2 * q + 1 < blocks else 0)
            if any(lo <= p < hi for p in ps):
                held[r, 2 * q * V:(2 * q + 2) * V] = True
    assert held[1:].any(1).all() and not held[0].any() and (~held[1:]).any()
    assert np.array_equal(got.view(np.uint32)[~held], zer.view(np.uint32)[~held]), \
        "an output of a clean transform changed"
    assert np.isfinite(ref[~held]).all()
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got)[held], f(ref)[held]), (N, name)
    assert (~np.isfinite(ref[held])).any()
    if zero_tap:
        # the lone +inf at V - 1 meets every tap, the zero one too: NaN from inf * 0
        assert where[5] == [V - 1] and np.isnan(ref[5]).sum() == 1 and np.isinf(ref[5]).any()
    fin = held & np.isfinite(ref)
    assert np.max(np.abs(got[fin] - ref[fin])) <= b
    assert np.max(np.abs(got[~held] - ref[~held])) <= b
    print(f"[fastconv] non-finite N={N} zero_tap={zero_tap}: {int(held.sum())} outputs direct, "
          f"worst finite err / bound = {float(np.max(np.abs(got[fin] - ref[fin]))) / b:.3f}")


# --------------------------------------------------------------------------- drop-in
def test_convolucion_rapida_is_np_convolve(gpu):
    from modules.dsp_core import convolucion_rapida
    from test_gpu_parity import _traced
    design = _design()
    assert design.FASTCONV_MIN_TAPS >= 2
    rng = np.random.default_rng(9)
    for K, name in ((design.FASTCONV_MIN_TAPS - 1, "src_poly"),
                    (design.FASTCONV_MIN_TAPS, "fastconv"), (1023, "fastconv")):
        h = fm.make_taps(K).astype(np.float64)
        for n in (5000, max(K - 7, 1)):
            # (float32 values: the reference convolves the data the kernels see)
            x1 = rng.uniform(-1, 1, n).astype(np.float32).astype(np.float64)
            x2 = rng.uniform(-1, 1, (3, n)).astype(np.float32).astype(np.float64)
            b = fm.bound(h, x2)
            for modo in ("same", "full", "causal"):
                def want(r):
                    return np.convolve(r, h)[:n] if modo == "causal" else np.convolve(r, h, modo)
                g1 = convolucion_rapida(x1, h, modo=modo)
                assert g1.dtype == np.float64 and g1.shape == want(x1).shape, (K, n, modo)
                assert np.max(np.abs(g1 - want(x1))) <= b, (K, n, modo)
                g2 = convolucion_rapida(x2, h, modo=modo)
                assert g2.dtype == np.float64 and g2.shape == (3,) + want(x2[0]).shape
                for r in range(3):
                    assert np.max(np.abs(g2[r] - want(x2[r]))) <= b, (K, n, modo, r)
                t = torch.from_numpy(x2.astype(np.float32)).to(gpu)
                (g3,), names = _traced(lambda: (convolucion_rapida(t, h, modo=modo),))
                assert name in names and g3.is_cuda and g3.dtype == torch.float32, (K, names)
                for r in range(3):
                    assert np.max(np.abs(g3[r].cpu().numpy() - want(x2[r]))) <= b, (K, n, modo, r)
    g = convolucion_rapida(x1, h)                      # the default is np.convolve's 'same'
    assert np.max(np.abs(g - np.convolve(x1, h, "same"))) <= b
    with pytest.raises(ValueError):
        convolucion_rapida(x1, h, modo="valid")
    with pytest.raises(ValueError):
        convolucion_rapida(x1, np.zeros((2, 2)))
