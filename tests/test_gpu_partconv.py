"""Partitioned fast convolution on the GPU (include/dspcore_partconv.h,
csrc/fft_pconv.hip k_partconv_fwd / k_partconv_mac, dspcore.partconv.PartConv,
modules.dsp_core.convolucion_rapida above 8193 taps), through the C ABI and the
class.

Sizes N = 64, 512, 4096 (Plan<log2 N> packs 64, 8 and 1 transforms per
workgroup), one case at N = 16384.  With V = N/4, P = H = N/2: K = P (one
partition), P + 1, 2 P, 2 P + 1, 5 P - 3, at N = 64 also 2049 (65 partitions);
offset 0, (K - 1)/2, K - 1 (beyond H: the pairs before pair 0); rows of 1,
H - 1, H, H + 1, 2 H + 1 and 3 H + 5 samples; n_out = n_in and the full length.
Cases and the numpy model are tests/partconv_model.py's.

The C-ABI harness (_call) keeps 1.0e3 in everything the kernels must not read
(x's padding and lead columns, hist_in past hist_len, a new ring) and in
hist_out, the sentinel bits 0xCAFEF00D in y's padding, and checks after every
call that the sentinels are intact and that hist_out[:hist_len] is bitwise the
last hist_len samples of (history | row).  Rows sit at an odd pitch unless a
test says otherwise, so consecutive rows start at every 4-byte residue.

Reference: float64 np.convolve of the float32 data; bound 2e-6 * ||taps||_2 *
max|x| (fastconv_model.BOUND_REL).  Every case prints its worst error / bound
ratio.  Largest ratio measured on an MI355X: 0.349 (N = 16384, K = 8194);
per size, values 0.20 (N = 64; 0.09 at its 65 partitions), 0.29, 0.34, 0.35 and
stream cuts 0.20, 0.25, 0.31; the ring-wrap stream 0.17; the finite outputs of
the non-finite fallback 0.03.
"""
import numpy as np
import pytest
import torch

import partconv_model as pm
from conv_gpu_helpers import SENT, YSENT, _bits, _design, _ops, _tail

pytestmark = pytest.mark.gpu


def _plan(taps, N):
    return _design().partconv_plan(taps, log2n=N.bit_length() - 1)


class _Ring:
    """A spectra ring for B rows, 1.0e3 in every word (a stale flag word reads
    as set, a stale spectrum as 1.0e3)."""

    def __init__(self, gpu, plan, B, slots):
        self.slots = slots
        self.ws = _ops().partconv_workspace(plan, B, slots, gpu)
        self.ws.view(torch.float32).fill_(SENT)


def _call(gpu, x, plan, offset=0, n_out=None, pos=0, hist=None, ring=None, odd=1, lead=0, tag=""):
    """dsp_partconv_f32 on the rows of x [B, n] (device float32) with the
    sentinel harness; returns (y [B, n_out], hist_out [B, hist_len])."""
    from dspcore import _lib
    lib = _lib.load()
    B, n = x.shape
    K, L = plan.K, plan.hist_len
    n_out = n if n_out is None else n_out
    if ring is None:
        ring = _Ring(gpu, plan, B, _ops().partconv_slots(plan, max(n, n_out), offset))
    pitch = (lambda w: (w + 4) | 1) if odd else (lambda w: (w + 7) & ~3)
    ldx, ldy, ldh = pitch(n + lead), pitch(n_out), pitch(L)
    xb = torch.full((B, ldx), SENT, dtype=torch.float32, device=gpu)
    xb[:, lead:lead + n] = x
    yb = torch.full((B, ldy), YSENT, dtype=torch.int32, device=gpu)
    hin = torch.full((B, ldh), SENT, dtype=torch.float32, device=gpu)
    if hist is not None:
        hin[:, :L] = hist
    hout = torch.full((B, ldh), SENT, dtype=torch.float32, device=gpu)
    taps, hf, tw = _ops().partconv_tables(plan, gpu)
    rc = lib.dsp_partconv_f32(
        xb.data_ptr() + 4 * lead, yb.data_ptr(), B, n, ldx, n_out, ldy, offset, pos,
        hin.data_ptr() if hist is not None else None, hout.data_ptr(), ldh, taps.data_ptr(), K,
        hf.data_ptr(), plan.log2n, ring.ws.data_ptr(), ring.ws.numel(), ring.slots, tw.data_ptr(),
        torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, (tag, _lib.last_error())
    assert bool((yb[:, n_out:] == YSENT).all()), (tag, "y's padding written")
    assert bool((hout[:, L:] == SENT).all()), (tag, "hist_out past hist_len written")
    want = _tail(hist if pos > 0 else None, x, L)
    assert torch.equal(_bits(hout[:, :L]), _bits(want)), (tag, "hist_out")
    if hist is not None:
        assert torch.equal(_bits(hin[:, :L]), _bits(hist)) and bool((hin[:, L:] == SENT).all())
    return yb[:, :n_out].view(torch.float32).clone(), hout[:, :L].clone()


def _check_values(gpu, N, K, lengths, tag):
    taps = pm.make_taps(K)
    plan = _plan(taps, N)
    V, H, S, L = pm.geometry(N, K)
    assert (plan.P, plan.S, plan.hist_len) == (H, S, L)
    worst = 0.0
    for n in lengths:
        x = pm.make_rows(N, n)
        ref = pm.full_reference(x, taps)
        b = pm.bound(taps, x)
        xd = torch.from_numpy(x.copy()).to(gpu)
        for off in pm.offsets(K):
            for n_out in sorted({n, n + K - 1 - off}):
                t = f"{tag} N={N} K={K} n={n} off={off} n_out={n_out}"
                y, _ = _call(gpu, xd, plan, off, n_out, tag=t)
                want = ref[:, off:off + n_out]
                yn = y.cpu().numpy()
                err = np.abs(yn.astype(np.float64) - want)
                worst = max(worst, float(np.max(err)) / b)
                assert np.max(err) <= b, (t, float(np.max(err)) / b,
                                          np.unravel_index(np.argmax(err), err.shape))
                # the impulse rows return the taps (the same bound)
                for r, p in enumerate(pm.impulse_positions(N, n)):
                    m = np.arange(n_out)
                    d = m + off - p
                    imp = np.where((d >= 0) & (d < K), taps[np.clip(d, 0, K - 1)], 0.0)
                    assert np.max(np.abs(yn[r] - imp)) <= b, (t, "impulse", r)
    print(f"[partconv] values N={N} K={K} S={S}: worst err / bound = {worst:.3f}")


# --------------------------------------------------------------------------- values
@pytest.mark.parametrize("N,ki", [(N, ki) for N in pm.SIZES for ki in range(len(pm.tap_counts(N)))])
def test_values_against_float64_convolve(gpu, N, ki):
    """Every row length, offset and both n_out for one (N, K): the nine rows
    (impulses of amplitude 1 at 0, P - 1, P, V and the last sample, which
    return the taps -- a wrong partition order or delay shows at every seam;
    two tones; noise) within the bound of float64 np.convolve."""
    _check_values(gpu, N, pm.tap_counts(N)[ki], pm.row_lengths(N), "values")


def test_values_at_the_largest_size(gpu):
    """N = 16384 (1024 threads a transform): K = 8194 is two partitions."""
    _check_values(gpu, 16384, 8194, (2 * 8192 + 5,), "largest")


# --------------------------------------------------------------------------- rows
@pytest.mark.parametrize("N", pm.SIZES)
def test_rows_do_not_depend_on_the_batch_or_the_layout(gpu, N):
    """Each row alone, the batch reversed, aligned rows, a column-offset view
    and a larger ring: bitwise the odd-pitch batch's rows."""
    H = N // 2
    K = 2 * H + 1
    n = 3 * H + 5
    off = (K - 1) // 2
    plan = _plan(pm.make_taps(K), N)
    x = torch.from_numpy(pm.make_rows(N, n).copy()).to(gpu)
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
    big = _Ring(gpu, plan, x.shape[0], _ops().partconv_slots(plan, n, off) + 3)
    v, _ = _call(gpu, x, plan, off, ring=big, tag=f"larger ring N={N}")
    assert torch.equal(_bits(v), _bits(y)), N
    # no output asked for: the history is still written (_call checks it)
    e, h = _call(gpu, x[:, :7], plan, off, n_out=0, tag=f"n_out 0 N={N}")
    assert e.shape == (x.shape[0], 0) and h.shape == (x.shape[0], plan.hist_len)
    # through the operator, on a column-offset view of a wider tensor
    wide = torch.full((x.shape[0], n + 7), SENT, dtype=torch.float32, device=gpu)
    wide[:, 3:3 + n] = x
    o = _ops().partconv(wide[:, 3:3 + n], plan, off)
    assert torch.equal(_bits(o), _bits(y)), N


def test_pairs_of_one_row_straddle_workgroups(gpu):
    """N = 64 packs 64 transforms per workgroup: 51 rows of 3 output pairs are
    153 transforms in 3 workgroups of the second launch (and 4 pairs a row, 204
    transforms in 4 workgroups, in the first: offset > 0), the last with dead
    transforms, and rows whose pairs lie in two workgroups; every row is
    bitwise its base row."""
    N, K = 64, 65
    H = N // 2
    n = 2 * H + 1
    off = 3
    plan = _plan(pm.make_taps(K), N)
    base = torch.from_numpy(pm.make_rows(N, n).copy()).to(gpu)
    B = 51
    assert -(-n // H) == 3 and pm.TPB[N] % 3 != 0 and B * 3 > 2 * pm.TPB[N]
    idx = torch.arange(B, device=gpu) % base.shape[0]
    narrow, _ = _call(gpu, base, plan, off, tag="base")
    wide, _ = _call(gpu, base[idx], plan, off, tag="wide")
    same = (_bits(wide) == _bits(narrow)[idx]).all(1)
    assert bool(same.all()), torch.nonzero(~same).flatten()[:8].tolist()


# --------------------------------------------------------------------------- stream
def _stream(gpu, x, plan, cuts, lead=lambda i: 0, odd=1, slots=None, tag=""):
    """x [B, n] through the C ABI block by block, history and ring chained."""
    slots = _ops().partconv_slots(plan, max(cuts)) if slots is None else slots
    ring = _Ring(gpu, plan, x.shape[0], slots)
    outs, pos, hist = [], 0, None
    for i, c in enumerate(cuts):
        y, hist = _call(gpu, x[:, pos:pos + c], plan, 0, c, pos, hist, ring, odd, lead(i),
                        f"{tag} call {i}")
        outs.append(y)
        pos += c
    assert pos == x.shape[1]
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("N", pm.SIZES)
@pytest.mark.parametrize("kk", ("one", "three"))
def test_stream_cuts(gpu, N, kk):
    """Cuts at multiples of H are bitwise the one call; ragged, reversed and
    view cuts (zero-length and 1-sample pushes included) are within the bound;
    hist_out is checked after every call (_call)."""
    V, H = N // 4, N // 2
    K = H if kk == "one" else 2 * H + 1
    taps = pm.make_taps(K)
    plan = _plan(taps, N)
    sizes = [0, 1, H - 1, H, H + 1, 2 * H, 2 * H + 5]
    n = sum(sizes)
    assert n == 7 * H + 6
    x = np.random.default_rng(N + K).uniform(-1, 1, (5, n)).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    ref = pm.full_reference(x, taps)[:, :n]
    b = pm.bound(taps, x)
    one = _stream(gpu, xd, plan, [n], tag=f"one N={N}")
    for cuts in ([H, 4 * H, n - 5 * H], [4 * H, 2 * H, n - 6 * H], [6 * H, H, 6]):
        got = _stream(gpu, xd, plan, cuts, tag=f"H cuts N={N}")
        assert torch.equal(_bits(got), _bits(one)), (N, K, cuts)
    worst = float(np.max(np.abs(one.cpu().numpy() - ref))) / b
    for name, cuts, lead in (("ragged", sizes, lambda i: 0), ("reversed", sizes[::-1], lambda i: 0),
                             ("views", [H + 1, 2 * H + 5, 0, H - 1, 1, 2 * H, H],
                              lambda i: 1 + i % 3)):
        got = _stream(gpu, xd, plan, cuts, lead, tag=f"{name} N={N}")
        err = float(np.max(np.abs(got.cpu().numpy() - ref)))
        worst = max(worst, err / b)
        assert err <= b, (N, K, name, err / b)
    print(f"[partconv] stream N={N} K={K}: worst err / bound = {worst:.3f}")


def test_stream_wraps_the_ring(gpu):
    """S = 3 at N = 64 with the smallest ring dsp_partconv_slots gives: blocks
    of H samples (5 slots, 14 pairs: the ring wraps more than twice) are
    bitwise the one call, blocks of at most 7 samples (also 5 slots) within the
    bound."""
    N = 64
    H = N // 2
    K = 2 * H + 1
    taps = pm.make_taps(K)
    plan = _plan(taps, N)
    n = 14 * H
    x = np.random.default_rng(77).uniform(-1, 1, (3, n)).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    ops = _ops()
    assert plan.S == 3 and ops.partconv_slots(plan, H) == 5 == ops.partconv_slots(plan, 7)
    one = _stream(gpu, xd, plan, [n], tag="wrap one")
    got = _stream(gpu, xd, plan, [H] * 14, tag="wrap H")
    assert torch.equal(_bits(got), _bits(one))
    cuts = []
    while sum(cuts) < n:
        cuts.append(min((7, 3, 5, 1, 7, 6, 7, 2)[len(cuts) % 8], n - sum(cuts)))
    assert sum(cuts) == n and max(cuts) == 7 and n // H >= 2 * 5 + 1
    got = _stream(gpu, xd, plan, cuts, tag="wrap ragged")
    ref = pm.full_reference(x, taps)[:, :n]
    err = float(np.max(np.abs(got.cpu().numpy() - ref)))
    assert err <= pm.bound(taps, x), err / pm.bound(taps, x)
    print(f"[partconv] ring wrap: worst err / bound = {err / pm.bound(taps, x):.3f}")


@pytest.mark.parametrize("N", (64, 4096))
def test_class_stream_state_and_modes(gpu, N):
    """PartConv.push over ragged cuts is bitwise the C-ABI stream with the same
    cuts; a state_dict round trip continues bitwise into an object whose
    buffers held the sentinel; the one-shot modes are np.convolve's."""
    from dspcore.partconv import PartConv
    H = N // 2
    K = 2 * H + 1
    taps = pm.make_taps(K)
    plan = _plan(taps, N)
    sizes = [0, 1, H - 1, H, H + 1, 2 * H, 2 * H + 5]
    n = sum(sizes)
    x = np.random.default_rng(N + K).uniform(-1, 1, (5, n)).astype(np.float32)
    xd = torch.from_numpy(x).to(gpu)
    abi = _stream(gpu, xd, plan, sizes, tag=f"class N={N}")
    pc = PartConv(taps, batch=5, max_block=2 * H + 5, log2n=plan.log2n, device=gpu)
    assert (pc.K, pc.n_fft, pc.hop, pc.S, pc.latency) == (K, N, H, 3, (K - 1) / 2)
    outs, pos, cut = [], 0, 4
    for i, c in enumerate(sizes):
        if i == cut:
            sd = pc.state_dict()
            assert sd["samples"] == pos and sd["hist"].shape == (5, plan.hist_len)
        y = pc.push(xd[:, pos:pos + c])
        assert y.shape == (5, c)
        outs.append(y.clone())
        pos += c
    assert pc.samples == n
    assert torch.equal(_bits(torch.cat(outs, dim=1)), _bits(abi))
    other = PartConv(taps, batch=5, max_block=2 * H + 5, log2n=plan.log2n, device=gpu)
    other._hist.fill_(SENT)                             # nothing but the state is read
    other._ws.view(torch.float32).fill_(SENT)
    other._y.fill_(SENT)
    other.load_state_dict(sd)
    pos = sum(sizes[:cut])
    for i, c in enumerate(sizes[cut:]):
        assert torch.equal(_bits(other.push(xd[:, pos:pos + c])), _bits(outs[cut + i])), i
        pos += c
    other.reset()
    assert torch.equal(_bits(other.push(xd[:, :1])), _bits(outs[1]))
    with pytest.raises(ValueError):
        PartConv(taps, batch=4, log2n=plan.log2n, device=gpu).load_state_dict(sd)
    for bad in (xd[:4, :8], xd[:, :2 * H + 6], xd[:, :8].double(), xd[0, :8], xd[:, :8].cpu()):
        with pytest.raises(ValueError):
            pc.push(bad)
    with pytest.raises(ValueError):
        PartConv(taps, batch=0, device=gpu)
    with pytest.raises(ValueError):
        PartConv(np.zeros((2, 2)), device=gpu)
    # one-shot, leaving the stream state alone
    before = pc.state_dict()
    b = pm.bound(taps, x)
    for mode in ("causal", "same", "full"):
        for m in (n, K - 3):
            got = pc(xd[:, :m], mode).cpu().numpy()
            for r in range(5):
                full = np.convolve(x[r, :m].astype(np.float64), taps.astype(np.float64))
                want = full[:m] if mode == "causal" else np.convolve(
                    x[r, :m].astype(np.float64), taps.astype(np.float64), mode)
                assert got[r].shape == want.shape, (mode, m)
                assert np.max(np.abs(got[r] - want)) <= b, (N, mode, m, r)
    after = pc.state_dict()
    assert torch.equal(after["hist"], before["hist"]) and after["samples"] == before["samples"]
    with pytest.raises(ValueError):
        pc(xd, "valid")


def test_a_push_is_two_launches_and_replays_from_a_graph(gpu):
    """One push is the `partconv_fwd` and the `partconv_mac` launch; captured
    into a graph it replays bitwise from the state it was captured at."""
    from dspcore.partconv import PartConv
    from test_gpu_parity import _traced
    N = 512
    H = N // 2
    K = 2 * H + 1
    taps = pm.make_taps(K)
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (3, 2 * H + 9))
                         .astype(np.float32)).to(gpu)
    pc = PartConv(taps, batch=3, max_block=x.shape[1], log2n=9, device=gpu)
    (y0,), names = _traced(lambda: (pc.push(x),))
    assert names == ["partconv_fwd", "partconv_mac"], names
    h0 = pc.state_dict()["hist"]
    (e,), names = _traced(lambda: (pc.push(x[:, :0]),))
    assert names == ["partconv_fwd"] and e.shape == (3, 0), names   # (the history's copy)
    assert torch.equal(pc.state_dict()["hist"], h0)      # an empty push keeps the history
    x_static = x.clone()
    graph = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream(gpu)
    cap.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(cap):
        pc.push(x_static)
        pc.reset()                                       # the warm-up moved the state
        with torch.cuda.graph(graph, stream=cap):
            y = pc.push(x_static)
    torch.cuda.current_stream(gpu).wait_stream(cap)
    torch.cuda.synchronize(gpu)
    for _ in range(2):
        y.fill_(SENT)
        pc._ws.view(torch.float32).fill_(SENT)
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(_bits(y), _bits(y0))
        assert torch.equal(pc.state_dict()["hist"], h0)


# --------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("N,zero_tap", [(N, z) for N in pm.SIZES for z in (True, False)])
def test_non_finite_samples_get_convolves_classes(gpu, N, zero_tap):
    """+inf, -inf, NaN and a +inf / -inf pair in one window, at the first
    sample, on either side of a pair seam and at the last sample.  Every
    output of a pair that reads a spectrum holding such a sample has the class
    np.convolve gives in float64 (one tap set has an exact zero: inf * 0 = NaN)
    and, where finite, is within the bound; every other output is bitwise the
    run with the bad samples replaced by 0."""
    V, H = N // 4, N // 2
    K = 2 * H + 1
    S = 3
    n = 3 * H + 5
    off = (K - 1) // 2 if zero_tap else 0
    n_out = n if zero_tap else n + K - 1
    taps = pm.make_taps(K, K // 3 if zero_tap else None)
    assert (taps == 0).any() == zero_tap
    plan = _plan(taps, N)
    assert plan.S == S
    clean = pm.make_rows(N, n)[7]
    inf = np.float32(np.inf)
    kinds = [(inf,), (-inf,), (np.float32(np.nan),), (inf, -inf)]
    pos = [0, H - 1 + off, H + off, n - 1]
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
    b = pm.bound(taps, x0)
    got, _ = _call(gpu, torch.from_numpy(x).to(gpu), plan, off, n_out, tag=f"nf N={N}")
    zer, _ = _call(gpu, torch.from_numpy(x0).to(gpu), plan, off, n_out, tag=f"nf0 N={N}")
    got, zer = got.cpu().numpy(), zer.cpu().numpy()
    # spectrum j holds the samples x[j H - 3 V + off, j H + 2 V + off); pair q
    # reads spectra q - S + 1 .. q (from the stream's first pair on)
    qfirst = (-off) // H
    held = np.zeros((x.shape[0], n_out), dtype=bool)
    for r, ps in enumerate(where):
        for q in range(-(-n_out // H)):
            js = range(max(qfirst, q - S + 1), q + 1)
            if any(j * H - 3 * V + off <= p < j * H + 2 * V + off for j in js for p in ps):
                held[r, q * H:(q + 1) * H] = True
    assert held[1:].any(1).all() and not held[0].any() and (~held[1:]).any()
    assert np.array_equal(got.view(np.uint32)[~held], zer.view(np.uint32)[~held]), \
        "an output of a clean pair changed"
    assert np.isfinite(ref[~held]).all()
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        assert np.array_equal(f(got)[held], f(ref)[held]), (N, name)
    assert (~np.isfinite(ref[held])).any()
    if zero_tap:
        # the lone +inf at the seam meets every tap, the zero one too: NaN from inf * 0
        assert where[5] == [H - 1 + off] and np.isnan(ref[5]).sum() == 1 and np.isinf(ref[5]).any()
    fin = held & np.isfinite(ref)
    assert fin.any() and np.max(np.abs(got[fin] - ref[fin])) <= b
    assert np.max(np.abs(got[~held] - ref[~held])) <= b
    print(f"[partconv] non-finite N={N} zero_tap={zero_tap}: {int(held.sum())} outputs direct, "
          f"worst finite err / bound = {float(np.max(np.abs(got[fin] - ref[fin]))) / b:.3f}")


# --------------------------------------------------------------------------- drop-in
def test_convolucion_rapida_above_8193_taps(gpu):
    from modules.dsp_core import convolucion_rapida
    from test_gpu_parity import _traced
    rng = np.random.default_rng(9)
    for K, launches in ((8193, {"fastconv"}), (8194, {"partconv_fwd", "partconv_mac"}),
                        (20000, {"partconv_fwd", "partconv_mac"})):
        h = pm.make_taps(K).astype(np.float64)
        for n in (5000, K - 7):
            # (float32 values: the reference convolves the data the kernels see)
            x1 = rng.uniform(-1, 1, n).astype(np.float32).astype(np.float64)
            x2 = rng.uniform(-1, 1, (3, n)).astype(np.float32).astype(np.float64)
            b = pm.bound(h, x2)
            full = {r.tobytes(): np.convolve(r, h) for r in (x1, *x2)}
            for modo in ("same", "full", "causal"):
                def want(r):
                    # np.convolve(r, h, modo), cut from the one 'full' result
                    # of the row: 'same' is its max(n, K) samples from
                    # (min(n, K) - 1) // 2 on
                    lo, m = {"causal": (0, n), "full": (0, n + K - 1),
                             "same": ((min(n, K) - 1) // 2, max(n, K))}[modo]
                    return full[r.tobytes()][lo:lo + m]
                t = torch.from_numpy(x2.astype(np.float32)).to(gpu)
                (g3,), names = _traced(lambda: (convolucion_rapida(t, h, modo=modo),))
                assert launches <= set(names) and "src_poly" not in names, (K, names)
                assert g3.is_cuda and g3.dtype == torch.float32
                for r in range(3):
                    assert np.max(np.abs(g3[r].cpu().numpy() - want(x2[r]))) <= b, (K, n, modo, r)
                if K == 8193:
                    continue
                g1 = convolucion_rapida(x1, h, modo=modo)
                assert g1.dtype == np.float64 and g1.shape == want(x1).shape, (K, n, modo)
                assert np.max(np.abs(g1 - want(x1))) <= b, (K, n, modo)
                g2 = convolucion_rapida(x2, h, modo=modo)
                assert g2.dtype == np.float64 and g2.shape == (3,) + want(x2[0]).shape
                for r in range(3):
                    assert np.max(np.abs(g2[r] - want(x2[r]))) <= b, (K, n, modo, r)
