"""The loader, playback and conversion kernels of csrc/audio_io.hip at their
edges: k_pcm_mono, k_pcm_batch, k_scale_batch, k_absmax, k_scale, k_quantize16
and k_convert, every result BITWISE against a few lines of numpy (float64, or
numpy's own float32 arithmetic).  There is no tolerance in this module.

tests/test_gpu_audio_io.py checks the same promise at friendly shapes: at most
10 channels (the 8-accumulator block of channel_mean never ran a second
round), each decoder in one or two files, 1200 random G.711 codes, rows of at
most 5000 frames (k_scale_batch reduced at most 5 block maxima), contiguous
rows only, uniform noise through the quantiser, and assert_array_equal, which
takes -0.0 for +0.0.

Method, for every part:
  * the kernels are called through the C ABI; inputs are views into larger
    buffers whose padding holds 0xFF bytes (NaN as a float, -1 / 255 as an
    integer), outputs are views into buffers full of a sentinel bit pattern
    that must be unchanged beside and behind every row;
  * results are compared as bit patterns (uint32 views, int16 equality); where
    the reference is NaN the result must be NaN, payloads are not compared;
  * the decode is restated here in float64 from the bytes: ints / 2^(bits-1),
    (u8 - 128) / 128, s8 / 128, floats as stored, G.711 through the 256-entry
    tables of test_audio_model.py (closed form, pinned on audioop there and
    here); then numpy's .mean(axis=1) for ch > 1, .astype(float32),
    np.max(np.abs(x)) and x / peak where peak > 1e-6.  Playback is
    oracle.dsp_ref_cpu.playback_pcm16, files are oracle.dsp_ref_cpu.load_audio.

A: every (format, bits, flags) decoder x 11 channel counts; B: all 256 G.711
codes; C: peak and normalise; D: the batched loader (descriptor tables, 293
and 2048 block maxima, 65 541 rows); E: the quantiser; F: k_convert past one
grid-stride round; G: files with -0.0 frames.

Two things the inputs need that random data does not give (pcm_row,
_threshold_rows): the channel mean's summation order survives the float32 cast
only where an addition rounds by much, so the float rows carry frames in which
two huge samples cancel; and 1e-6 lies strictly between two float32 values, so
only a threshold a float32 can equal tells `>` from `>=`.

Before channel_mean added +0.0 to its multi-channel sum, 43 cases failed, all
on the all -0.0 frames (-0.0 for numpy's +0.0): A's 40 float cases with ch >= 2,
test_d_batch_every_decoder, test_d_batch_past_the_grid_row_limit and G.
"""
import ctypes
import io

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import audio_files
from test_audio_model import ALAW, ULAW, same_bits

pytestmark = pytest.mark.gpu

PCM, FLT, ALAW_T, ULAW_T, BE, S8 = 1, 3, 6, 7, 0x100, 0x200
# the 17 instantiations launch_pcm_mono lists, in its order
KEYS = {
    "u8": (PCM, 8), "s8": (PCM | S8, 8), "s8be": (PCM | S8 | BE, 8),
    "s16le": (PCM, 16), "s24le": (PCM, 24), "s32le": (PCM, 32),
    "s16be": (PCM | BE, 16), "s24be": (PCM | BE, 24), "s32be": (PCM | BE, 32),
    "f32le": (FLT, 32), "f64le": (FLT, 64), "f32be": (FLT | BE, 32), "f64be": (FLT | BE, 64),
    "ulaw": (ULAW_T, 8), "alaw": (ALAW_T, 8), "ulaw_be": (ULAW_T | BE, 8),
    "alaw_be": (ALAW_T | BE, 8),
}
CHANNELS = (1, 2, 7, 8, 9, 15, 16, 17, 24, 127, 128)
FRAMES = 1029                 # two blocks, three grid-stride rounds, a ragged end
SENT = -889262067             # int32 0xCAFEF00D: a finite float32 of magnitude 8.4e6
SENT16 = -13570               # int16 0xCAFE
THRESHOLD = 1e-6              # dsp_core.py:31
BIG = 2048 * 1024 + 1029      # past io_blocks' 2048-block cap: five rounds per thread
FLT_MAX = float(np.finfo(np.float32).max)
F32_SPECIALS = (-0.0, 0.0, 1e-45, -1e-45, FLT_MAX, -FLT_MAX)
F64_SPECIALS = F32_SPECIALS + (1e39, -1e39, 1e-40, 1.0 + 2.0 ** -24, 5e-324)
NONFINITE = (np.nan, np.inf, -np.inf)


def io_blocks(n):
    """csrc/audio_io.hip io_blocks: ~4 elements per thread of 256, 1..2048 blocks."""
    return min(2048, max(1, -(-n // 1024)))


def _abi():
    from dspcore import _lib, ops
    return _lib.load(), _lib, ops


def _ok(rc, what):
    lib, _lib, _ = _abi()
    assert rc == 0, f"{what}: status {rc}: {_lib.last_error()}"


# --------------------------------------------------------------------------- buffers
class Buf:
    """[B, n] rows at pitch ld inside a device buffer full of `fill`, GUARD
    elements of padding before the first row and after the last."""
    GUARD = 67

    def __init__(self, B, n, ld, gpu, dtype=np.float32, fill=SENT):
        self.B, self.n, self.ld, self.dtype = B, n, ld, np.dtype(dtype)
        self.raw = {2: np.int16, 4: np.int32, 8: np.int64}[self.dtype.itemsize]
        self.fill = fill
        self.host = np.full(B * ld + 2 * self.GUARD, fill, dtype=self.raw)
        self.dev = None
        self.gpu = gpu

    def _rows(self, flat):
        return flat[self.GUARD:self.GUARD + self.B * self.ld].reshape(self.B, self.ld)

    def put(self, rows):
        rows = np.ascontiguousarray(rows, dtype=self.dtype).reshape(self.B, self.n)
        self._rows(self.host)[:, :self.n] = rows.view(self.raw)
        return self

    @property
    def ptr(self):
        if self.dev is None:
            self.dev = torch.from_numpy(self.host).to(self.gpu)
        return self.dev.data_ptr() + self.GUARD * self.dtype.itemsize

    def get(self):
        """The rows, after checking that every padding element is untouched."""
        h = self.dev.cpu().numpy()
        G = self.GUARD
        assert (h[:G] == self.fill).all() and (h[-G:] == self.fill).all(), "wrote outside the rows"
        assert (self._rows(h)[:, self.n:] == self.fill).all(), "wrote behind a row"
        return np.ascontiguousarray(self._rows(h)[:, :self.n]).view(self.dtype)


def _peaks(B, gpu):
    return Buf(1, B, B + 3, gpu)


def _pcm(pieces, offsets, total, gpu):
    host = np.full(total, 0xFF, dtype=np.uint8)
    for raw, off in zip(pieces, offsets):
        host[off:off + raw.size] = raw
    return torch.from_numpy(host).to(gpu)


def _bits_ok(got, ref, what):
    ok = same_bits(got, ref)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.size} differ, first at {i}: "
                             f"got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), "
                             f"reference {ref[i]!r} ({ref.view(np.uint32)[i]:#010x})")


# --------------------------------------------------------------------------- references
def decode_ref(fmt, bits, raw):
    """Flat float64 samples of the bytes `raw`, as soundfile returns them."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    base, be = fmt & 0xFF, bool(fmt & BE)
    if base == ULAW_T:
        return ULAW[raw] / 32768.0
    if base == ALAW_T:
        return ALAW[raw] / 32768.0
    end = ">" if be else "<"
    if base == FLT:
        return raw.view(f"{end}f{bits // 8}").astype(np.float64)
    if bits == 8:
        if fmt & S8:
            return raw.view(np.int8).astype(np.float64) / 128.0
        return (raw.astype(np.float64) - 128.0) / 128.0
    if bits == 24:
        b = raw.reshape(-1, 3).astype(np.int64)
        hi, mid, lo = (b[:, 0], b[:, 1], b[:, 2]) if be else (b[:, 2], b[:, 1], b[:, 0])
        v = (hi << 16) | (mid << 8) | lo
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return v.astype(np.float64) / 8388608.0
    return raw.view(f"{end}i{bits // 8}").astype(np.float64) / float(1 << (bits - 1))


def mono_ref(fmt, bits, raw, ch):
    x = decode_ref(fmt, bits, raw).reshape(-1, ch)
    with np.errstate(all="ignore"):
        x = x.mean(axis=1) if ch > 1 else x[:, 0]
        return x.astype(np.float32)


def norm_ref(x, threshold=None):
    """(x / peak where peak > 1e-6, peak) in numpy's float32, as the loader;
    with `threshold`, the C ABI's rule: where (double)peak > threshold."""
    if x.size == 0:
        return x, np.float32(0)
    with np.errstate(all="ignore"):
        peak = np.max(np.abs(x))
        scale = peak > 1e-6 if threshold is None else float(peak) > threshold
        return (x / peak if scale else x), peak


# --------------------------------------------------------------------------- rows
def _encode(fmt, bits, v):
    base, end = fmt & 0xFF, ">" if fmt & BE else "<"
    with np.errstate(all="ignore"):
        if base in (ULAW_T, ALAW_T):
            out = v.astype(np.uint8)
        elif base == FLT:
            out = v.astype(f"{end}f{bits // 8}")
        elif bits == 8:
            out = v.astype(np.int8) if fmt & S8 else (v + 128).astype(np.uint8)
        elif bits == 24:
            return np.frombuffer((audio_files.pcm_be if fmt & BE else audio_files.pcm_le)(v, 24),
                                 dtype=np.uint8).copy()
        else:
            out = v.astype(f"{end}i{bits // 8}")
    return np.frombuffer(out.tobytes(), dtype=np.uint8).copy()


_ROWS = {}


def pcm_row(name, ch, seed=0):
    """FRAMES frames of `ch` channels in format `name` as bytes: seeded random
    samples, then
      frames 0..: one frame per special value with that value in every channel
        (floats: frame 0 all -0.0, frame 1 (+inf, -inf, ...), then the finite
        specials; ints: min, max, -1, 0, +1);
      frames 16..524: finite special j alone at channel position c of frame
        16 + (j ch + c) mod 509 (509 is prime: two specials never meet in one
        sample), so every special visits every channel position;
      frames 530..1028: NaN, +inf, -inf alone at position c of frame
        530 + (k ch + c) mod 499 (floats only; at most frame 913);
      frames 920..1019: the cancellation frames below (floats, ch > 1)."""
    key = (name, ch, seed)
    if key in _ROWS:
        return _ROWS[key]
    fmt, bits = KEYS[name]
    base = fmt & 0xFF
    rng = np.random.default_rng([seed, ch, bits, fmt])
    nonfinite = ()
    if base in (ULAW_T, ALAW_T):
        v = rng.integers(0, 256, (FRAMES, ch))
        specials = (0x00, 0x80, 0x7F, 0xFF, 0x55, 0xD5, 0x2A, 0xAA)
    elif base == FLT:
        v = rng.uniform(-1.3, 1.3, (FRAMES, ch))
        if bits == 32:
            v = v.astype(np.float32).astype(np.float64)
        specials = F32_SPECIALS if bits == 32 else F64_SPECIALS
        nonfinite = NONFINITE
    else:
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        v = rng.integers(lo, hi + 1, (FRAMES, ch))
        specials = (lo, hi, -1, 0, 1)
    c = np.arange(ch)
    for j, s in enumerate(specials):
        v[16 + (j * ch + c) % 509, c] = s
    for k, s in enumerate(nonfinite):
        v[530 + (k * ch + c) % 499, c] = s
    if base == FLT and ch > 1:
        # The summation order shows only where an addition rounds, and after
        # the float32 cast only where it rounds by much: +L and -L (2^50 and
        # up) at two random positions among samples of order 1.  L cancels
        # exactly, but every sample added while it sits in an accumulator is
        # rounded to a multiple of 2^-2, so the sum depends on which
        # accumulator each channel goes to and in which order.  (Integer PCM
        # and G.711 sums of up to 128 channels are exact in float64: no input
        # of theirs can tell two orders apart.)
        for f in range(920, 1020):
            p, q = rng.choice(ch, 2, replace=False)
            L = float(np.float32(rng.uniform(1, 2))) * 2.0 ** 50
            v[f, p], v[f, q] = L, -L
    if base == FLT:
        v[0, :] = -0.0
        v[1, :] = np.where(c % 2 == 0, np.inf, -np.inf)
        for j, s in enumerate(specials):
            v[2 + j, :] = s
    else:
        for j, s in enumerate(specials):
            v[j, :] = s
    raw = _encode(fmt, bits, v)
    assert raw.size == FRAMES * ch * (bits // 8)
    _ROWS[key] = raw
    return raw


def run_pcm_to_mono(gpu, fmt, bits, ch, rows, frames):
    """dsp_pcm_to_mono_f32 over equally long byte rows: ld_bytes = row bytes + 5
    behind a 7-byte lead, ld_out = frames + 3."""
    lib, _, ops = _abi()
    B = len(rows)
    nbytes = frames * ch * (bits // 8)
    ld_bytes = nbytes + 5
    pcm = _pcm(rows, [7 + b * ld_bytes for b in range(B)], 7 + B * ld_bytes + 16, gpu)
    out = Buf(B, frames, frames + 3, gpu)
    _ok(lib.dsp_pcm_to_mono_f32(pcm.data_ptr() + 7, fmt, bits, ch, B, frames, ld_bytes, out.ptr,
                                out.ld, ops._stream(gpu)), "dsp_pcm_to_mono_f32")
    return out.get()


def run_peak_normalize(gpu, rows, threshold=THRESHOLD):
    """dsp_peak_normalize_f32 in place at ld = n + 3: (rows, peaks)."""
    lib, _, ops = _abi()
    rows = np.asarray(rows, dtype=np.float32)
    B, n = rows.shape
    x = Buf(B, n, n + 3, gpu).put(rows)
    pk = _peaks(B, gpu)
    _ok(lib.dsp_peak_normalize_f32(x.ptr, B, n, x.ld, threshold, pk.ptr, ops._stream(gpu)),
        "dsp_peak_normalize_f32")
    return x.get(), pk.get()[0]


# --------------------------------------------------------------------------- A
@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("name", list(KEYS))
def test_a_decoder_channels(gpu, name, ch):
    """k_pcm_mono<format, bits, BE, S8> at ch channels, three rows."""
    fmt, bits = KEYS[name]
    rows = [pcm_row(name, ch, seed) for seed in range(3)]
    got = run_pcm_to_mono(gpu, fmt, bits, ch, rows, FRAMES)
    for b, raw in enumerate(rows):
        ref = mono_ref(fmt, bits, raw, ch)
        if (fmt & 0xFF) == FLT:
            # the all -0.0 frame: +0.0 from two channels up, -0.0 kept in mono
            assert ref.view(np.uint32)[0] == (0x80000000 if ch == 1 else 0)
            assert np.isnan(ref[1]) == (ch > 1)
        _bits_ok(got[b], ref, f"{name} ch={ch} row {b}")


# --------------------------------------------------------------------------- B
def test_b_g711_tables():
    import audioop
    codes = bytes(range(256))
    assert np.array_equal(ULAW, np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2"))
    assert np.array_equal(ALAW, np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2"))
    assert (ULAW[0x00], ULAW[0x80], ULAW[0x7F], ULAW[0xFF]) == (-32124, 32124, 0, 0)
    assert (ALAW[0x55], ALAW[0xD5], ALAW[0x2A], ALAW[0xAA]) == (-8, 8, -32256, 32256)


@pytest.mark.parametrize("name", ["ulaw", "alaw", "ulaw_be", "alaw_be"])
def test_b_g711_all_codes(gpu, name):
    fmt, bits = KEYS[name]
    table = ULAW if (fmt & 0xFF) == ULAW_T else ALAW
    codes = np.arange(256, dtype=np.uint8)
    got = run_pcm_to_mono(gpu, fmt, bits, 1, [codes], 256)[0]
    _bits_ok(got, (table / 32768.0).astype(np.float32), f"{name} mono")
    assert np.array_equal(got * 32768.0, table)         # every code, exactly
    pair = np.stack([codes, 255 - codes], axis=1).reshape(-1)
    got = run_pcm_to_mono(gpu, fmt, bits, 2, [pair], 256)[0]
    ref = ((table[codes] / 32768.0 + table[255 - codes] / 32768.0 + 0.0) / 2.0).astype(np.float32)
    _bits_ok(ref, mono_ref(fmt, bits, pair, 2), f"{name} reference")
    _bits_ok(got, ref, f"{name} pairs")


# --------------------------------------------------------------------------- C
def _peak_rows(n, rng):
    """name -> float32 row of length n (see test_c_peak_normalize)."""
    eps = np.float32(1e-6)
    up = np.nextafter(eps, np.float32(1))
    rows = {}

    def noise(peak, at, sign=1.0):
        x = (rng.uniform(-0.5, 0.5, n) * peak).astype(np.float32)
        x[at] = np.float32(sign * peak)
        return x
    rows["peak first"] = noise(0.8125, 0)
    rows["peak last negative"] = noise(3.25, n - 1, -1.0)
    rows["at threshold"] = noise(eps, n // 2)
    rows["above threshold"] = noise(up, n // 3)
    x = noise(up, n - 1)
    if n > 2:
        x[0], x[n // 2] = np.float32(1e-45), np.float32(-3e-39)
    rows["subnormal quotients"] = x
    x = noise(0.5, 0)
    x[n // 2] = np.nan
    rows["nan peak"] = x
    x = noise(7.0, 0)
    x[n - 1] = -np.inf
    if n > 2:
        x[1] = -0.0
    rows["inf peak"] = x
    rows["negative zeros"] = np.full(n, -0.0, dtype=np.float32)
    return rows


def _check_peak_rows(gpu, rows):
    names = list(rows)
    src = np.stack([rows[k] for k in names])
    got, peaks = run_peak_normalize(gpu, src)
    for b, k in enumerate(names):
        ref, peak = norm_ref(src[b])
        _bits_ok(peaks[b:b + 1], np.asarray([peak], dtype=np.float32), f"{k}: peak")
        _bits_ok(got[b], ref, k)
    return names, src, got, peaks


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_c_peak_normalize(gpu, n):
    """k_absmax<false> + k_scale: the peak at a row's first and last sample,
    at the threshold (float32(1e-6): not scaled) and one ulp above (scaled),
    subnormal quotients, NaN and inf peaks, an all -0.0 row."""
    rows = _peak_rows(n, np.random.default_rng(n))
    names, src, got, peaks = _check_peak_rows(gpu, rows)
    at = {k: b for b, k in enumerate(names)}
    u = lambda a: a.view(np.uint32)
    # what each row is there for, stated on the reference-checked result
    assert np.array_equal(u(got[at["at threshold"]]), u(src[at["at threshold"]]))
    b = at["above threshold"]
    assert np.max(np.abs(got[b])) == 1.0 and peaks[b] == np.nextafter(np.float32(1e-6), np.float32(1))
    assert np.array_equal(u(got[at["nan peak"]]), u(src[at["nan peak"]])) and np.isnan(peaks[at["nan peak"]])
    b = at["inf peak"]
    assert np.isnan(got[b, n - 1]) and np.isinf(peaks[b])
    if n > 2:
        # finite / inf: zeros that keep their sign (the peak is +inf)
        assert not got[b, :n - 1].any() and u(got[b, 1:2])[0] == 0x80000000
        assert np.array_equal(np.signbit(got[b, :n - 1]), np.signbit(src[b, :n - 1]))
        q, s = got[at["subnormal quotients"]], src[at["subnormal quotients"]]
        tiny = np.finfo(np.float32).tiny
        assert 0 < q[0] < tiny and 0 < -s[n // 2] < tiny and q[n // 2] < 0
    assert (u(got[at["negative zeros"]]) == 0x80000000).all() and u(peaks)[at["negative zeros"]] == 0


def test_c_peak_normalize_past_the_block_cap(gpu):
    """n = 2048 * 1024 + 1029: io_blocks at its cap, five rounds per thread."""
    assert io_blocks(BIG) == 2048 and io_blocks(2048 * 1024) == 2048 and io_blocks(2047 * 1024) == 2047
    rows = _peak_rows(BIG, np.random.default_rng(3))
    _check_peak_rows(gpu, {k: rows[k] for k in ("peak first", "peak last negative")})


def _threshold_rows():
    """Peaks at, one ulp below and one ulp above 2^-20, a threshold that a
    float32 peak can equal (1e-6 lies strictly between two float32 values, so
    with it `>` and `>=` decide alike)."""
    thr = np.float32(2.0 ** -20)
    rng = np.random.default_rng(20)
    rows = []
    for peak in (thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))):
        x = (rng.uniform(-0.5, 0.5, 300) * peak).astype(np.float32)
        x[299] = -peak
        rows.append(x)
    return float(thr), np.stack(rows)


def test_c_threshold_is_exclusive(gpu):
    """k_scale and k_scale_batch divide where (double)peak > threshold: a peak
    equal to the threshold is left alone."""
    thr, src = _threshold_rows()
    refs = [norm_ref(r, thr) for r in src]
    u = lambda a: a.view(np.uint32)
    assert np.array_equal(u(refs[0][0]), u(src[0])) and np.array_equal(u(refs[1][0]), u(src[1]))
    assert refs[2][0][299] == -1.0
    got, peaks = run_peak_normalize(gpu, src, thr)
    fmt, bits = KEYS["f32le"]
    desc, pieces, offsets, total = _table([(r.view(np.uint8), 300, fmt, bits, 1) for r in src])
    bgot, bpeaks = run_pcm_batch(gpu, _pcm(pieces, offsets, total, gpu), desc, 300, 303, thr)
    for b, (ref, peak) in enumerate(refs):
        _bits_ok(got[b], ref, f"k_scale row {b}")
        _bits_ok(bgot[b], ref, f"k_scale_batch row {b}")
        assert u(peaks)[b] == u(bpeaks)[b] == u(np.asarray([peak]))[0]


# --------------------------------------------------------------------------- D
ROW_DTYPE = np.dtype([("offset", "<i8"), ("frames", "<i8"), ("format", "<i4"), ("bits", "<i4"),
                      ("channels", "<i4"), ("reserved", "<i4")])


def run_pcm_batch(gpu, pcm, desc, width, ld_out, threshold=THRESHOLD):
    """dsp_pcm_batch_to_mono_f32 over the descriptor table `desc` (ROW_DTYPE):
    (rows [B, width], peak bits as float32 [B]); the workspace starts as 0xFF
    bytes, so a block maximum nobody wrote would read as a NaN peak."""
    lib, _lib, ops = _abi()
    assert ROW_DTYPE.itemsize == ctypes.sizeof(_lib.PcmRow)
    B = desc.shape[0]
    out = Buf(B, width, ld_out, gpu)
    pk = _peaks(B, gpu)
    nws = int(lib.dsp_pcm_batch_workspace_bytes(B, width))
    ws = torch.full((nws + 256,), 0xFF, dtype=torch.uint8, device=gpu)
    wsp = (ws.data_ptr() + 255) & ~255
    _ok(lib.dsp_pcm_batch_to_mono_f32(pcm.data_ptr(), pcm.numel(), desc.ctypes.data, B, width,
                                      out.ptr, out.ld, threshold, pk.ptr, wsp, nws,
                                      ops._stream(gpu)), "dsp_pcm_batch_to_mono_f32")
    torch.cuda.synchronize(gpu)
    return out.get(), pk.get()[0]


def _table(entries):
    """[(bytes, frames, format, bits, channels)] -> (descriptor table, pieces,
    offsets, total): row b starts at a byte offset of residue b mod 8."""
    desc = np.zeros(len(entries), dtype=ROW_DTYPE)
    pieces, offsets, off = [], [], 3
    for b, (raw, frames, fmt, bits, ch) in enumerate(entries):
        off += (b % 8 - off) % 8
        desc[b] = (off, frames, fmt, bits, ch, 0)
        pieces.append(raw)
        offsets.append(off)
        off += raw.size + 1
    return desc, pieces, offsets, off + 16


def test_d_batch_every_decoder(gpu):
    """A's rows in one k_pcm_batch launch, one per key at three channel counts
    (full rows, and 500 frames of the all-finite part, which are normalised),
    a row of no frames and rows of one frame: bitwise the numpy loader and the
    per-row kernels, zeros behind each row's frames."""
    entries = []
    for k, (name, (fmt, bits)) in enumerate(KEYS.items()):
        fb = bits // 8
        for t in range(3):
            ch = CHANNELS[(3 * k + t) % len(CHANNELS)]
            raw = pcm_row(name, ch)
            lo, hi = ((0, FRAMES), (2, 502), (16, 16 + 1 + k))[t]
            entries.append((raw[lo * ch * fb:hi * ch * fb], hi - lo, fmt, bits, ch))
    entries.append((np.zeros(0, np.uint8), 0, FLT, 32, 2))
    for name, ch in (("f32le", 2), ("f64be", 1), ("s16be", 128), ("f32be", 9)):
        fmt, bits = KEYS[name]
        entries.append((pcm_row(name, ch)[:ch * bits // 8], 1, fmt, bits, ch))   # frame 0
    desc, pieces, offsets, total = _table(entries)
    assert set(desc["offset"] % 8) == set(range(8))
    assert {0, 1, FRAMES} <= set(desc["frames"].tolist())
    pcm = _pcm(pieces, offsets, total, gpu)
    got, peaks = run_pcm_batch(gpu, pcm, desc, FRAMES, FRAMES + 3)
    scaled = 0
    for b, (raw, frames, fmt, bits, ch) in enumerate(entries):
        ref, peak = norm_ref(mono_ref(fmt, bits, raw, ch))
        scaled += bool(peak > 1e-6)
        what = f"row {b} (format {fmt:#x}/{bits}, ch {ch}, {frames} frames)"
        _bits_ok(got[b, :frames], ref, what)
        _bits_ok(peaks[b:b + 1], np.asarray([peak], dtype=np.float32), what + " peak")
        assert not got[b, frames:].view(np.uint32).any(), what + ": not +0.0 behind the frames"
        if frames:
            one = run_pcm_to_mono(gpu, fmt, bits, ch, [raw], frames)
            one, pk1 = run_peak_normalize(gpu, one)
            _bits_ok(one[0], ref, what + " per-row kernels")
            _bits_ok(got[b, :frames], np.where(np.isnan(ref), ref, one[0]), what + " batch vs per-row")
            _bits_ok(pk1, np.asarray([peak], dtype=np.float32), what + " per-row peak")
    assert scaled >= 17           # the normalising branch ran for every key


@pytest.mark.parametrize("at", [65541, 74759, 299999])
def test_d_batch_peak_in_a_late_block(gpu, at):
    """width 300 000: k_scale_batch reduces 293 block maxima, 256 in its first
    round.  The one large sample sits in block 256, in block 292 (the last), or
    is the row's last frame."""
    width = 300000
    nbx = io_blocks(width)
    assert nbx == 293 and (at % (nbx * 256)) // 256 == (256 if at == 65541 else 292)
    rng = np.random.default_rng(at)
    rows = [rng.integers(125, 132, width).astype(np.uint8) for _ in range(3)]
    for b, r in enumerate(rows):
        r[at] = (255, 0, 250)[b]
    fmt, bits = KEYS["u8"]
    desc, pieces, offsets, total = _table([(r, width, fmt, bits, 1) for r in rows])
    got, peaks = run_pcm_batch(gpu, _pcm(pieces, offsets, total, gpu), desc, width, width + 3)
    for b, r in enumerate(rows):
        ref, peak = norm_ref(mono_ref(fmt, bits, r, 1))
        assert abs(ref[at]) == 1.0 and peak == abs((int(r[at]) - 128) / 128.0)
        _bits_ok(peaks[b:b + 1], np.asarray([peak], dtype=np.float32), f"row {b} peak")
        _bits_ok(got[b], ref, f"row {b}")


def test_d_batch_past_the_block_cap(gpu):
    """width 2048 * 1024 + 1029: 2048 blocks (the cap), the peak as the last frame."""
    width = BIG
    assert io_blocks(width) == 2048
    rng = np.random.default_rng(11)
    fmt, bits = KEYS["u8"]
    rows = [rng.integers(120, 137, width).astype(np.uint8) for _ in range(2)]
    rows[0][-1], rows[1][-1] = 1, 254
    desc, pieces, offsets, total = _table([(r, width, fmt, bits, 1) for r in rows])
    got, peaks = run_pcm_batch(gpu, _pcm(pieces, offsets, total, gpu), desc, width, width + 3)
    for b, r in enumerate(rows):
        ref, peak = norm_ref(mono_ref(fmt, bits, r, 1))
        assert abs(ref[-1]) == 1.0
        _bits_ok(peaks[b:b + 1], np.asarray([peak], dtype=np.float32), f"row {b} peak")
        _bits_ok(got[b], ref, f"row {b}")


WIDE = 65541                  # 6 rows past the grid's 65 535-row split


def test_d_batch_past_the_grid_row_limit(gpu):
    """65 541 rows cycling through 17 base rows, one per key (17 is prime:
    every key meets both sides of the split), 1..5 frames at width 5."""
    entries = []
    for k, (name, (fmt, bits)) in enumerate(KEYS.items()):
        frames, ch = 1 + k % 5, (1, 2, 7, 8, 9, 16, 17)[k % 7]
        # floats: the all -0.0 frame, or the frames of one special each;
        # integers: frames with a special at one channel position
        lo = (0 if frames == 1 else 2) if (fmt & 0xFF) == FLT else 16
        fb = ch * bits // 8
        entries.append((pcm_row(name, ch)[lo * fb:(lo + frames) * fb], frames, fmt, bits, ch))
    base, pieces, offsets, total = _table(entries)
    desc = np.ascontiguousarray(base[np.arange(WIDE) % 17])
    got, peaks = run_pcm_batch(gpu, _pcm(pieces, offsets, total, gpu), desc, 5, 8)
    for b, (raw, frames, fmt, bits, ch) in enumerate(entries):
        ref, peak = norm_ref(mono_ref(fmt, bits, raw, ch))
        _bits_ok(got[b, :frames], ref, f"base row {b}")
        _bits_ok(peaks[b:b + 1], np.asarray([peak], dtype=np.float32), f"base row {b} peak")
        assert not got[b, frames:].view(np.uint32).any()
    idx = np.arange(WIDE) % 17
    bad = np.flatnonzero((got.view(np.uint32) != got.view(np.uint32)[idx]).any(axis=1)
                         | (peaks.view(np.uint32) != peaks.view(np.uint32)[idx]))
    assert bad.size == 0, f"{bad.size} rows differ from their base row, first {bad[:5]}"


def test_d_pcm_to_mono_past_the_grid_row_limit(gpu):
    fmt, bits = KEYS["s16le"]
    v = np.random.default_rng(65).integers(-32768, 32768, (WIDE, 6)).astype("<i2")
    rows = list(v.view(np.uint8).reshape(WIDE, 12))
    got = run_pcm_to_mono(gpu, fmt, bits, 2, rows, 3)
    ref = (v.astype(np.float64) / 32768.0).reshape(WIDE, 3, 2).mean(axis=2).astype(np.float32)
    _bits_ok(got, ref, "int16 stereo, 65541 rows")


# --------------------------------------------------------------------------- E
def run_quantize(gpu, z, precision):
    """dsp_quantize_pcm16 at ld_z = n + 3 (0xFF padding: NaN), ld_out = n + 5."""
    lib, _, ops = _abi()
    B, n = z.shape
    zin = Buf(B, n, n + 3, gpu, fill=-1).put(z)
    out = Buf(B, n, n + 5, gpu, dtype=np.int16, fill=SENT16)
    pk = _peaks(B, gpu)
    _ok(lib.dsp_quantize_pcm16(zin.ptr, out.ptr, B, n, zin.ld, out.ld, pk.ptr, precision,
                               ops._stream(gpu)), "dsp_quantize_pcm16")
    return out.get()


def _edge_row(peak):
    """float32(j / 32767 * peak), j = -32767..32767: after / peak * 32767 every
    sample lies next to an integer, where truncation and rounding differ."""
    j = np.arange(-32767, 32768, dtype=np.float64)
    return (j / 32767.0 * peak).astype(np.float32)


def _check_quantize(gpu, rows):
    from oracle import dsp_ref_cpu as orc
    names = list(rows)
    z = np.stack([rows[k] for k in names])
    differ = {}
    with np.errstate(all="ignore"):
        r32 = [orc.playback_pcm16(z[b]) for b in range(len(names))]
        r64 = [orc.playback_pcm16(z[b].astype(np.float64)) for b in range(len(names))]
    for precision, ref in ((32, r32), (64, r64)):
        got = run_quantize(gpu, z, precision)
        for b, k in enumerate(names):
            bad = np.flatnonzero(got[b] != ref[b])
            assert bad.size == 0, (f"{k}, float{precision}: {bad.size} differ, first at {bad[0]}: "
                                   f"z {z[b, bad[0]]!r} got {got[b, bad[0]]} ref {ref[b][bad[0]]}")
    for b, k in enumerate(names):
        differ[k] = int(np.count_nonzero(r32[b] != r64[b]))
    return differ, r32, r64


def test_e_quantize_edges(gpu):
    rng = np.random.default_rng(16)
    n = 65535
    rows = {f"edge {p}": _edge_row(p) for p in (0.73, 1.0, 3.1e-3, 1e-40)}
    x = np.zeros(n, dtype=np.float32)
    x[rng.integers(0, n, 900)] = np.float32(1e-45)
    x[rng.integers(0, n, 900)] = np.float32(-1e-45)
    x[n - 1] = np.float32(1e-45)
    rows["peak 1e-45"] = x
    x = (rng.uniform(-1, 1, n) * FLT_MAX).astype(np.float32)
    x[0] = -np.float32(FLT_MAX)
    rows["peak FLT_MAX"] = x
    for name, v in (("peak +inf", np.inf), ("peak -inf", -np.inf)):
        x = (rng.uniform(-1, 1, n) * 1e30).astype(np.float32)
        x[5], x[6], x[n - 2] = v, np.nan, np.float32(FLT_MAX)
        rows[name] = x
    rows["all NaN"] = np.full(n, np.nan, dtype=np.float32)
    rows["all -0.0"] = np.full(n, -0.0, dtype=np.float32)
    differ, r32, r64 = _check_quantize(gpu, rows)
    print("float32 vs float64 references differ at", differ)
    # the two modes stay distinguishable, and the edge row is an edge: the
    # truncated values are not the ideal j
    assert differ["edge 0.73"] > 0 and sum(differ[f"edge {p}"] for p in (1.0, 3.1e-3, 1e-40)) > 0
    ideal = np.arange(-32767, 32768)
    assert np.count_nonzero(r32[0] != ideal) > 10000 and np.count_nonzero(r64[0] != ideal) > 10000
    assert r32[4][n - 1] == 32767 and not r32[8].any() and not r32[9].any()


def test_e_quantize_past_the_block_cap(gpu):
    rng = np.random.default_rng(17)
    x = rng.uniform(-0.999, 0.999, BIG).astype(np.float32)
    x[-1] = np.float32(-1.7)
    _check_quantize(gpu, {"peak last": x})


# --------------------------------------------------------------------------- F
NCONV = 8192 * 256 + 3        # the grid's 8192 blocks of 256, then a second round


@pytest.mark.parametrize("narrow", [True, False])
def test_f_convert_second_round(gpu, narrow):
    lib, _, ops = _abi()
    rng = np.random.default_rng(19)
    src = rng.uniform(-2, 2, NCONV)
    special = np.array(F64_SPECIALS + NONFINITE + (1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24),
                                                  2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149,
                                                  float(np.float32(1e-6)), -3e-39))
    src[-64:] = np.resize(special, 64)
    if not narrow:
        with np.errstate(all="ignore"):
            src = src.astype(np.float32)
    fin = Buf(1, NCONV, NCONV + 3, gpu, dtype=src.dtype, fill=-1).put(src)
    out = Buf(1, NCONV, NCONV + 3, gpu, dtype=np.float32 if narrow else np.float64,
              fill=SENT if narrow else (SENT << 32) | 0x0BADF00D)
    fn = lib.dsp_convert_f64_f32 if narrow else lib.dsp_convert_f32_f64
    _ok(fn(fin.ptr, out.ptr, NCONV, ops._stream(gpu)), "dsp_convert")
    with np.errstate(all="ignore"):
        ref = src.astype(out.dtype)
    got = out.get()[0]
    ok = same_bits(got, ref)
    assert ok.all(), (int(np.count_nonzero(~ok)), np.flatnonzero(~ok)[:5])


# --------------------------------------------------------------------------- G
def _signed_zero_file(kind):
    rng = np.random.default_rng(23)
    x = rng.uniform(-0.9, 0.9, (700, 2)).astype(np.float32)
    x[0] = x[300] = x[699] = -0.0                    # -0.0 frames: the mean is +0.0
    x[1] = (-0.0, 0.0)
    x[2] = (np.float32(1e-45), np.float32(-1e-45))
    x[3] = (np.float32(3e-39), np.float32(1e-45))
    assert np.isfinite(x).all()
    if kind == "wav":
        buf = io.BytesIO()
        wavfile.write(buf, 48000, x)
        return buf.getvalue()
    return audio_files.aiff(x.astype(">f4").tobytes(), 2, 44100, 32, b"fl32")


def test_g_files_with_negative_zero_frames(gpu):
    from dspcore import audio_io
    from modules import dsp_core
    from oracle import dsp_ref_cpu as orc
    files = [_signed_zero_file("wav"), _signed_zero_file("aiff")]
    refs = [orc.load_audio(f) for f in files]
    for f, (ref, rfs) in zip(files, refs):
        assert ref.view(np.uint32)[0] == 0 and ref.view(np.uint32)[300] == 0 and ref[3] != 0
        x, fs = dsp_core.cargar_senal_audio(io.BytesIO(f))
        assert fs == rfs and x.dtype == np.float32
        _bits_ok(x, ref, "cargar_senal_audio")
    batch, lengths, rates = audio_io.load_batch(files, gpu)
    got = batch.cpu().numpy()
    assert lengths == [700, 700] and rates == [r[1] for r in refs]
    for b, (ref, _) in enumerate(refs):
        _bits_ok(got[b], ref, f"load_batch row {b}")
