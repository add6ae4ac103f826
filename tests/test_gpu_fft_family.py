"""Every in-LDS FFT, spectrum and any-length-DFT kernel of csrc/fft.hip,
fft_spec.hip and fft_dft.hip (and fft_large.hip's two-launch four-step) at its
edges: all 15 sizes of both complex modes, the spectrum and the STFT at
n_fft = 2^1..2^14, every Bluestein size M = 2^1..2^14, and the two-launch
four-step sizes that had not run in spectrum or real-input mode.

Up to 2^14 points the dispatch tables pick one of ~75 template instantiations
(fft.hip: k_fft<0..14, C2C | R2C> and <0..4, Spec>, k_spec_real<5, 9, 13>;
fft_spec.hip: k_spec_stream<6, 7, 8, 10, 11, 14>, k_spec_wave12; fft_dft.hip:
k_bluestein<1..14>), each with its own Plan (first
radix, threads per transform TPT, transforms per workgroup TPB, padded LDS
image).  The other modules reach them at a few sizes, with B <= 3 and a Hann
window whose vanishing ends hide the first and last samples of every frame.

Method, for every part:
  * 11 base rows (prime: over a wide batch every base row meets every
    workgroup slot) -- impulses, tones, the rest seeded noise -- run once and
    are checked row by row against float64 (analytic for the structured rows,
    numpy's FFT of the float32 values otherwise) within the project's own
    bound, 1e-5 * the row's max|X| (FFT_RTOL).  An impulse has the same |X| in
    every bin, so for it the bound holds per bin; a tone bounds the leakage
    into every other bin.
  * the wide batch is base[arange(B) % 11], built on the device, with
    B = 2 * TPB + 1 (two full workgroups and a third with one live transform):
    every row of it must equal its base row BITWISE.
  * inputs and outputs are views into larger buffers with padded pitches; the
    input padding holds 1.0e3 (finite: no repair launch), so a read past a
    row's valid samples moves |X| by orders of magnitude; the output padding
    holds a sentinel bit pattern that must be unchanged afterwards.
  * the spectrum and the STFT are called through the C ABI with the module's
    own window w[j] = 0.25 + 0.75 j / N: exact in float32 up to 2^14, nowhere
    zero, every position 0.75 / N away from its neighbour (>= 4.5x the bound at
    2^14).  An impulse of amplitude a at frame position p < valid gives
    |X[k]| = |a| w[p] in every bin, which checks the load mapping sample by
    sample; a frame with no valid sample must give exact zeros.

The trace records scope names only (fft, fft_nf, spectrum, spectrum_nf, stft,
dft); SPEC_ROUTE and TPB_OF below restate csrc/fft.hip's dispatch_spec and
csrc/fft_pass.h's Plan as literals and say which kernel a case is for.  The
spectrum has no other instantiation: k_spec_real<6, 7, 8, 10, 11, 12, 14> and
k_fft<5..14, Spec>, which no size was ever routed to, are no longer compiled.

Every case prints its worst error / bound ratio.
"""
import numpy as np
import pytest
import torch

from test_gpu_parity import FFT_RTOL, _traced

pytestmark = pytest.mark.gpu

R = 11                    # base rows; prime
IN_PAD = 1.0e3            # input padding: finite and far outside [-1, 1]
SENT = -889262067         # output padding: the bits 0xCAFEF00D (a finite float)
AMP = 0.75

# csrc/fft_pass.h Plan (TPT, TPB): TPT = N / RMAX, RMAX = 16 from N = 16 up;
# TPB = 256 / TPT, 1 from TPT = 256 up.
TPB_OF = (256, 256, 256, 256, 256, 128, 64, 32, 16, 8, 4, 2, 1, 1, 1)


def TPT(k):
    return max(1, (1 << k) // 16)


def TPB(k):
    return max(1, 256 // TPT(k))


# csrc/fft.hip dispatch_spec: log2n -> (kernel, Plan index /
# transforms per unit / waves per group).
SPEC_ROUTE = {
    1: ("k_fft", 1), 2: ("k_fft", 2), 3: ("k_fft", 3), 4: ("k_fft", 4),
    5: ("k_spec_real", 4), 9: ("k_spec_real", 8), 13: ("k_spec_real", 12),
    6: ("k_spec_stream", 2), 7: ("k_spec_stream", 2), 8: ("k_spec_stream", 2),
    10: ("k_spec_stream", 2), 11: ("k_spec_stream", 2), 14: ("k_spec_stream", 2),
    12: ("k_spec_wave12", 16),
}


def test_plan_literals():
    assert tuple(TPB(k) for k in range(15)) == TPB_OF
    assert sorted(SPEC_ROUTE) == list(range(1, 15))


def _spec_group(lg):
    """Transforms that share a workgroup (a unit, a group of waves) on lg's route."""
    kern, arg = SPEC_ROUTE[lg]
    return TPB(arg) if kern in ("k_fft", "k_spec_real") else arg


def _spec_batches(lg):
    kern, arg = SPEC_ROUTE[lg]
    if kern in ("k_fft", "k_spec_real"):
        return (2 * TPB(arg) + 1,)
    if kern == "k_spec_stream":
        return (23,)              # odd: the last unit has one dead transform
    return (17, 33)               # a group with one live wave, then three groups


def _ops():
    from dspcore import ops
    return ops


def _lib():
    from dspcore import _lib
    return _lib


# --------------------------------------------------------------------------- buffers
def _pad_in(t, ld, lead=0):
    """t [B, n] (device) as a view at pitch ld into a buffer full of IN_PAD,
    one pitch of padding before the first row."""
    B, n = t.shape
    fill = complex(IN_PAD, IN_PAD) if t.is_complex() else IN_PAD
    buf = torch.full(((B + 2) * ld + lead,), fill, dtype=t.dtype, device=t.device)
    v = buf.as_strided((B, n), (ld, 1), ld + lead)
    v.copy_(t)
    return v


class _Out:
    """A [B, n] output view at pitch ld inside a buffer of sentinels."""

    def __init__(self, dev, B, n, ld, cplx):
        self.c = 2 if cplx else 1
        total = (B + 2) * ld
        self.bits = torch.full((total * self.c,), SENT, dtype=torch.int32, device=dev)
        flat = self.bits.view(torch.float32)
        if cplx:
            flat = torch.view_as_complex(flat.view(-1, 2))
        self.view = flat.as_strided((B, n), (ld, 1), ld)
        self.outside = torch.ones(total, dtype=torch.bool, device=dev)
        self.outside.as_strided((B, n), (ld, 1), ld).fill_(False)

    def check(self, tag):
        pad = self.bits.view(-1, self.c)[self.outside]
        bad = int((pad != SENT).sum())
        assert bad == 0, f"{tag}: {bad} sentinel words beside the output were overwritten"


def _bits(t):
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int32)


def _assert_wide(wide, base, idx, tag):
    same = (_bits(wide) == _bits(base)[idx]).flatten(1).all(1)
    if not bool(same.all()):
        rows = torch.nonzero(~same).flatten()[:8].tolist()
        raise AssertionError(f"{tag}: wide rows {rows} (of {len(idx)}) differ from their base rows")


def _ratios(got, ref, tag):
    """Per row max|got - ref| / (FFT_RTOL * max|ref|); a row whose reference is
    all zero must be exactly zero."""
    err = np.max(np.abs(got - ref), axis=1)
    top = np.max(np.abs(ref), axis=1)
    zero = top == 0
    assert np.all(err[zero] == 0), f"{tag}: rows {np.nonzero(zero & (err != 0))[0]} must be exact zeros"
    ratio = np.zeros_like(err)
    ratio[~zero] = err[~zero] / (FFT_RTOL * top[~zero])
    assert np.all(ratio <= 1.0), (f"{tag}: rows {np.nonzero(ratio > 1)[0].tolist()} exceed "
                                  f"1e-5 max|X|: ratios {ratio[ratio > 1]}")
    return float(ratio.max(initial=0.0))


def _report(family, size, worst):
    print(f"[fft-family] {family} {size}: worst err / bound = {worst:.3f}")


# --------------------------------------------------------------------------- base rows
def _dft_rows(n, real, impulses, tones, seed):
    """(x [11, n] float32 / complex64, X [11, n] complex128): impulses at the
    given positions, tones at the given bins (cos for real rows) with the phase
    reduced mod n in integers, the rest uniform(-1, 1)."""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.int64)
    amp = AMP if real else AMP - 0.5j
    xs, refs = [], []
    for p in sorted({q for q in impulses if 0 <= q < n}):
        x = np.zeros(n, dtype=np.complex128)
        x[p] = amp
        xs.append(x)
        refs.append(amp * np.exp(-2j * np.pi * ((p * j) % n) / n))
    for b in sorted({q for q in tones if 0 <= q < n and n >= 2}):
        ph = 2 * np.pi * ((b * j) % n) / n
        ref = np.zeros(n, dtype=np.complex128)
        if real:
            xs.append(AMP * np.cos(ph) + 0j)
            ref[b] += n * AMP / 2
            ref[(-b) % n] += n * AMP / 2
        else:
            xs.append(amp * np.exp(1j * ph))
            ref[b] = n * amp
        refs.append(ref)
    assert len(xs) <= R
    ft = np.float32 if real else np.complex64
    while len(xs) < R:
        x = rng.uniform(-1, 1, n)
        if not real:
            x = x + 1j * rng.uniform(-1, 1, n)
        x = x.astype(ft)
        xs.append(x.astype(np.complex128))
        refs.append(np.fft.fft(x.astype(np.complex128)))
    x = np.stack(xs)
    x = x.real.astype(np.float32) if real else x.astype(np.complex64)
    return x, np.stack(refs)


def _wide_idx(B, dev):
    return torch.arange(B, device=dev) % R


# --------------------------------------------------------------------------- A: k_fft
@pytest.mark.parametrize("real", (False, True), ids=("c2c", "r2c"))
@pytest.mark.parametrize("k", range(15))
def test_fft_every_plan_packed(gpu, k, real):
    """k_fft<k, C2C | R2C> through ops.fft: base rows against float64, then
    max(2 TPB(k) + 1, 23) rows bitwise; ld_in = N + 3 (real rows start at every
    4-byte residue), ld_out = N + 5 with sentinels."""
    ops = _ops()
    N = 1 << k
    x, ref = _dft_rows(N, real, (0, 1, N // 2 - 1, N // 2, N - 1),
                       (1, N // 2 - 1) if real else (1, N - 1), 100 + k)
    base = torch.from_numpy(x).to(gpu)

    def run(xd, tag):
        xin = _pad_in(xd, N + 3)
        out = _Out(gpu, xd.shape[0], N, N + 5, True)
        (res,), names = _traced(lambda: (ops.fft(xin, out.view),))
        assert names == ["fft", "fft_nf"], names
        out.check(tag)
        return res

    tag = f"k_fft<{k}, {'R2C' if real else 'C2C'}>"
    got = run(base, tag + " base")
    worst = _ratios(got.cpu().numpy().astype(np.complex128), ref, tag)
    B = max(2 * TPB(k) + 1, 23)
    idx = _wide_idx(B, gpu)
    _assert_wide(run(base[idx], tag + f" B={B}"), got, idx, tag + f" B={B}")
    _report(tag, f"N={N} B={B}", worst)


# --------------------------------------------------------------------------- B: spectrum, STFT
def _window(N):
    w = 0.25 + 0.75 * np.arange(N) / N
    w32 = w.astype(np.float32)
    assert np.array_equal(w32.astype(np.float64), w)      # exact in float32
    return w, w32


def _spec_rows(N, seg_len, w, seed):
    """(segments [11, seg_len] float32, |X| [11, N/2+1] float64) for the frame
    of `seg_len` valid samples: impulses at 0, 1, 2, 3 and valid - 1, one empty
    (all-zero) segment standing for the impulses at `valid` and N - 1 that fall
    outside it, the rest uniform(-1, 1)."""
    rng = np.random.default_rng(seed)
    half = N // 2 + 1
    segs, refs = [], []
    for p in sorted({q for q in (0, 1, 2, 3, seg_len - 1) if 0 <= q < seg_len}):
        s = np.zeros(seg_len, dtype=np.float32)
        s[p] = AMP
        segs.append(s)
        refs.append(np.full(half, AMP * w[p]))
    if seg_len < N:
        segs.append(np.zeros(seg_len, dtype=np.float32))
        refs.append(np.zeros(half))
    while len(segs) < R:
        s = rng.uniform(-1, 1, seg_len).astype(np.float32)
        fr = np.zeros(N)
        fr[:seg_len] = s
        segs.append(s)
        refs.append(np.abs(np.fft.rfft(w * fr)))
    return np.stack(segs), np.stack(refs)


def _spec_input(segs, idx, ld_x, seg_start):
    """Rows of pitch ld_x full of IN_PAD with segs[idx] at [seg_start, +seg_len)."""
    B, seg_len = len(idx), segs.shape[1]
    buf = torch.full(((B + 2) * ld_x,), IN_PAD, dtype=torch.float32, device=segs.device)
    rows = buf.as_strided((B, ld_x), (ld_x, 1), ld_x)
    if seg_len:
        rows[:, seg_start:seg_start + seg_len] = segs[idx]
    return rows


def _odd(v):
    return v | 1


def _spec_call(x, mag, seg_start, seg_len, lg, win, tw, hop=None, frames=None):
    """dsp_spectrum_f32 (frames None) or dsp_stft_mag_f32 through the C ABI."""
    L = _lib()
    lib = L.load()
    dev = x.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if frames is None:
            rc = lib.dsp_spectrum_f32(x.data_ptr(), mag.data_ptr(), x.shape[0], x.stride(0),
                                      seg_start, seg_len, lg, mag.stride(0), win.data_ptr(),
                                      tw.data_ptr(), None, 0, stream)
            L.check(rc, "dsp_spectrum_f32")
        else:
            rc = lib.dsp_stft_mag_f32(x.data_ptr(), mag.data_ptr(), x.shape[0], x.stride(0),
                                      seg_start, seg_len, hop, frames, lg, mag.stride(0),
                                      win.data_ptr(), tw.data_ptr(), stream)
            L.check(rc, "dsp_stft_mag_f32")
    return mag


@pytest.mark.parametrize("lg", range(1, 15))
def test_spectrum_every_route_window_and_edges(gpu, lg):
    """dsp_spectrum_f32 with the ramp window: every seg_len of {N, N-1, N-2,
    N-3, N/2+1, 1, 0} at seg_start 1 and every seg_start 0..3 at seg_len N-1,
    odd ld_x (frame bases at every residue mod 16 bytes), ld_mag = N/2+1+3."""
    ops = _ops()
    N = 1 << lg
    half = N // 2 + 1
    w, w32 = _window(N)
    win = torch.from_numpy(w32).to(gpu)
    assert win.data_ptr() % 16 == 0
    tw = ops._table("tw", N, gpu)
    seg_lens = sorted({v for v in (N, N - 1, N - 2, N - 3, N // 2 + 1, 1, 0) if 0 <= v <= N},
                      reverse=True)
    layouts = [(1, v) for v in seg_lens] + [(s, N - 1) for s in (0, 2, 3)]
    kern = SPEC_ROUTE[lg][0]
    worst = 0.0
    for seg_start, seg_len in layouts:
        segs_h, ref = _spec_rows(N, seg_len, w, 1000 * lg + 10 * seg_len + seg_start)
        segs = torch.from_numpy(segs_h).to(gpu)
        ld_x = _odd(seg_start + N + 8)

        def run(idx, tag):
            x = _spec_input(segs, idx, ld_x, seg_start)
            out = _Out(gpu, len(idx), half, half + 3, False)
            (res,), names = _traced(
                lambda: (_spec_call(x, out.view, seg_start, seg_len, lg, win, tw),))
            assert names == ["spectrum", "spectrum_nf"], names
            out.check(tag)
            return res

        tag = f"{kern} N={N} start={seg_start} len={seg_len}"
        got = run(torch.arange(R, device=gpu), tag + " base")
        worst = max(worst, _ratios(got.cpu().numpy().astype(np.float64), ref, tag))
        for B in _spec_batches(lg):
            idx = _wide_idx(B, gpu)
            _assert_wide(run(idx, tag + f" B={B}"), got, idx, tag + f" B={B}")
    _report(f"spectrum {kern}", f"N={N} B={_spec_batches(lg)}", worst)


@pytest.mark.parametrize("lg", range(1, 15))
def test_stft_every_route_frame_edges(gpu, lg):
    """dsp_stft_mag_f32 with the ramp window, hop = max(1, N/4) + 1 (odd from
    N = 8 up: the frame bases walk the alignments), 11 rows, every frame against
    float64.  No one hop puts valid = N - 1 and a valid of 1..3 in the same
    call, so two segment lengths run: 5 frames whose last has valid = N - 1,
    and 7 frames whose last two have valid = v in 1..3 and v - hop <= 0 (a
    frame wholly past the segment: legal by the header, exact zeros).  55 and
    77 transforms: no multiple of 2, 16 or any TPB > 1."""
    ops = _ops()
    N = 1 << lg
    half = N // 2 + 1
    w, w32 = _window(N)
    win = torch.from_numpy(w32).to(gpu)
    tw = ops._table("tw", N, gpu)
    hop = max(1, N // 4) + 1
    v = min(1 + lg % 3, hop)
    group = _spec_group(lg)
    rng = np.random.default_rng(300 + lg)
    worst = 0.0
    for frames, seg_len, last_valid in ((5, 4 * hop + N - 1, (N - 1,)),
                                        (7, 5 * hop + v, (v, v - hop))):
        valid = [seg_len - f * hop for f in range(frames)]
        assert tuple(valid[-len(last_valid):]) == last_valid and valid[-1] <= N - 1
        assert group == 1 or (R * frames) % group != 0
        seg_start = 1 + lg % 3
        ld_x = _odd(seg_start + seg_len + 8)
        segs_h = rng.uniform(-1, 1, (R, seg_len)).astype(np.float32)
        ref = np.zeros((R, frames, half))
        for f in range(frames):
            fr = np.zeros((R, N))
            part = segs_h[:, f * hop:f * hop + N]
            fr[:, :part.shape[1]] = part
            ref[:, f] = np.abs(np.fft.rfft(w * fr, axis=1))
        assert valid[-1] > 0 or not ref[:, -1].any()
        x = _spec_input(torch.from_numpy(segs_h).to(gpu), torch.arange(R, device=gpu), ld_x,
                        seg_start)
        out = _Out(gpu, R * frames, half, half + 3, False)
        tag = f"stft {SPEC_ROUTE[lg][0]} N={N} hop={hop} frames={frames} len={seg_len}"
        (got,), names = _traced(lambda: (_spec_call(x, out.view, seg_start, seg_len, lg, win, tw,
                                                    hop, frames),))
        assert names == ["stft", "spectrum_nf"], names
        out.check(tag)
        worst = max(worst, _ratios(got.cpu().numpy().astype(np.float64),
                                   ref.reshape(R * frames, half), tag))
    _report(f"stft {SPEC_ROUTE[lg][0]}", f"N={N} hop={hop}", worst)


@pytest.mark.parametrize("N", (4, 8, 16, 32, 128, 512, 8192))
def test_spectrum_hann_on_routes_never_run(gpu, N):
    """ops.spectrum (the app's Hann table) at the sizes no test ran it with:
    seg_len = N - 1 at start 1, B = 5, against float64 design.hann."""
    from dspcore import design
    rng = np.random.default_rng(400 + N)
    x = np.full((5, N + 9), IN_PAD, dtype=np.float32)
    x[:, 1:N] = rng.uniform(-1, 1, (5, N - 1))
    fr = np.zeros((5, N))
    fr[:, :N - 1] = x[:, 1:N]
    ref = np.abs(np.fft.rfft(design.hann(N) * fr, axis=1))
    (got,), names = _traced(lambda: (_ops().spectrum(torch.from_numpy(x).to(gpu), 1, N - 1, N),))
    assert names == ["spectrum", "spectrum_nf"], names
    worst = _ratios(got.cpu().numpy().astype(np.float64), ref, f"hann N={N}")
    _report(f"spectrum hann {SPEC_ROUTE[N.bit_length() - 1][0]}", f"N={N}", worst)


# --------------------------------------------------------------------------- C: k_bluestein
def _blu_tables(n, dev):
    """design.bluestein_tables(n) on the device; the chirp table carries one
    entry of IN_PAD behind its n values, so that a kernel that took input
    n (the first zero-padded slot) as a sample would show it."""
    from dspcore import design
    chirp, bf, M = design.bluestein_tables(n)
    chirp = np.concatenate([chirp, [complex(IN_PAD, IN_PAD)]])
    dev_t = [torch.from_numpy(a.astype(np.complex64).view(np.float32)).to(dev) for a in (chirp, bf)]
    return dev_t[0], dev_t[1], _ops()._table("tw", M, dev), M


def _blu_case(gpu, n, m, real, direct):
    L = _lib()
    lib = L.load()
    ops = _ops()
    assert lib.dsp_dft_size(n) == 1 << m
    x, ref = _dft_rows(n, real, (0, 1, n - 1), (1, n - 1), 500 + 2 * n + real)
    base = torch.from_numpy(x).to(gpu)
    tables = _blu_tables(n, gpu) if direct else None

    def call(xin, out):
        if not direct:
            return ops.dft(xin, out)
        chirp, bf, tw, M = tables
        assert M == 1 << m
        with torch.cuda.device(gpu):
            rc = lib.dsp_dft_f32(xin.data_ptr(), out.data_ptr(), xin.shape[0], n, int(real),
                                 xin.stride(0), out.stride(0), chirp.data_ptr(), bf.data_ptr(),
                                 tw.data_ptr(), torch.cuda.current_stream(gpu).cuda_stream)
        L.check(rc, "dsp_dft_f32")
        return out

    def run(xd, tag):
        xin = _pad_in(xd, n + 3)
        out = _Out(gpu, xd.shape[0], n, n + 5, True)
        (res,), names = _traced(lambda: (call(xin, out.view),))
        assert names == ["dft"], names
        out.check(tag)
        return res

    tag = f"k_bluestein<{m}> n={n} {'real' if real else 'complex'}"
    got = run(base, tag + " base")
    worst = _ratios(got.cpu().numpy().astype(np.complex128), ref, tag)
    B = max(2 * TPB(m) + 1, 23)
    idx = _wide_idx(B, gpu)
    _assert_wide(run(base[idx], tag + f" B={B}"), got, idx, tag + f" B={B}")
    _report(f"k_bluestein<{m}>", f"n={n} {'real' if real else 'complex'} B={B}", worst)


@pytest.mark.parametrize("real", (False, True), ids=("complex", "real"))
@pytest.mark.parametrize("m", range(1, 15))
def test_bluestein_tightest_length(gpu, m, real):
    """n = 2^(m-1), where 2n - 1 = M - 1 leaves the circular convolution one
    spare slot, through dsp_dft_f32 itself (ops.dft sends powers of two to the
    FFT) with design.bluestein_tables(n)."""
    _blu_case(gpu, 1 << (m - 1), m, real, True)


@pytest.mark.parametrize("real", (False, True), ids=("complex", "real"))
@pytest.mark.parametrize("m", range(3, 15))
def test_bluestein_first_and_last_length(gpu, m, real):
    """The shortest and the longest non-power-of-two length of every M = 2^m,
    n = 2^(m-2) + 1 and 2^(m-1) - 1, through ops.dft."""
    for n in sorted({(1 << (m - 2)) + 1, (1 << (m - 1)) - 1}):
        assert n & (n - 1)
        _blu_case(gpu, n, m, real, False)


# --------------------------------------------------------------------------- D: four-step
@pytest.mark.parametrize("lg", (16, 17, 19, 20, 21, 22))
def test_spectrum_four_step_sizes_never_run(gpu, lg):
    """k_fft4_a / k_fft4_b<kSpec> at the two-launch sizes the spectrum had not
    run: ops.spectrum, seg_start 3, seg_len N - 5, odd pitch, random rows
    against float64 and an impulse at the first and at the last valid sample
    (|X[k]| = w[p] of design.hann in every bin)."""
    from dspcore import design
    N = 1 << lg
    half = N // 2 + 1
    seg_start, seg_len = 3, N - 5
    per = 2 if lg <= 19 else 1
    w = design.hann(N)
    rng = np.random.default_rng(600 + lg)
    rows, refs = [], []
    for _ in range(per):
        s = rng.uniform(-1, 1, seg_len).astype(np.float32)
        fr = np.zeros(N)
        fr[:seg_len] = s
        rows.append(s)
        refs.append(np.abs(np.fft.rfft(w * fr)))
    for p in (0, seg_len - 1):
        s = np.zeros(seg_len, dtype=np.float32)
        s[p] = 1.0
        rows.append(s)
        refs.append(np.full(half, w[p]))
    ld_x = _odd(seg_start + N + 8)
    worst = 0.0
    for r0 in range(0, len(rows), per):
        segs = torch.from_numpy(np.stack(rows[r0:r0 + per])).to(gpu)
        x = _spec_input(segs, torch.arange(segs.shape[0], device=gpu), ld_x, seg_start)
        out = _Out(gpu, segs.shape[0], half, half + 3, False)
        (got,), names = _traced(lambda: (_ops().spectrum(x, seg_start, seg_len, N, out.view),))
        assert names == ["spectrum"], names
        tag = f"four-step spectrum N=2^{lg} rows {r0}.."
        out.check(tag)
        worst = max(worst, _ratios(got.cpu().numpy().astype(np.float64),
                                   np.stack(refs[r0:r0 + per]), tag))
    _report("four-step spectrum", f"N=2^{lg}", worst)


@pytest.mark.parametrize("lg", (17, 18, 19, 21, 22))
def test_fft_real_four_step_sizes_never_run(gpu, lg):
    """k_fft4_a<kR2C> at the two-launch sizes real input had not run, padded
    pitches and sentinels, random rows against float64 numpy."""
    N = 1 << lg
    B = 2 if lg <= 19 else 1
    x = np.random.default_rng(700 + lg).uniform(-1, 1, (B, N)).astype(np.float32)
    ref = np.fft.fft(x.astype(np.float64), axis=1)
    xin = _pad_in(torch.from_numpy(x).to(gpu), N + 3)
    out = _Out(gpu, B, N, N + 5, True)
    (got,), names = _traced(lambda: (_ops().fft(xin, out.view),))
    assert names == ["fft"], names
    tag = f"four-step R2C N=2^{lg}"
    out.check(tag)
    _report("four-step R2C", f"N=2^{lg}", _ratios(got.cpu().numpy().astype(np.complex128), ref, tag))
