"""The loader's two claims that need no GPU to check (csrc/audio_io.hip).

"numpy's summation order": `channel_mean` restates np.add.reduce over a
contiguous axis of 1..128 channels -- a plain loop below 8 elements, the
8-accumulator block above, the ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) combine, the
tail loop -- and numpy's reduction starts from the ufunc's identity, +0.0,
which only a frame of all -0.0 can show: its mean is +0.0.  `channel_mean_model`
is that function line by line in numpy float64 (elementwise IEEE adds); it is
compared here with `x.mean(axis=1)` of the installed numpy bit for bit, and
tests/test_gpu_audio_edges.py compares the kernels with the same call.

G.711: `ulaw_to_s16` / `alaw_to_s16` are the kernel's closed-form expansions;
all 256 codes of each law against audioop (the oracle's expansion), and the
end points as literals.
"""
import numpy as np
import pytest


def channel_mean_model(x):
    """csrc/audio_io.hip channel_mean over float64 frames x [F, ch]."""
    x = np.asarray(x, dtype=np.float64)
    ch = x.shape[1]
    if ch == 1:
        return x[:, 0].copy()          # mono: no mean is taken, -0.0 stays
    if ch < 8:
        s = x[:, 0].copy()
        for c in range(1, ch):
            s = s + x[:, c]
    else:
        r = [x[:, k].copy() for k in range(8)]
        c = 8
        while c + 8 <= ch:
            for k in range(8):
                r[k] = r[k] + x[:, c + k]
            c += 8
        s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while c < ch:
            s = s + x[:, c]
            c += 1
    return (s + 0.0) / float(ch)       # numpy's reduction starts from +0.0


def ulaw_to_s16(code):
    u = ~code & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7)
    return 0x84 - t if u & 0x80 else t - 0x84


def alaw_to_s16(code):
    a = code ^ 0x55
    t = (a & 0x0F) << 4
    seg = (a & 0x70) >> 4
    t = t + 8 if seg == 0 else (t + 0x108) << (seg - 1)
    return t if a & 0x80 else -t


ULAW = np.array([ulaw_to_s16(c) for c in range(256)], dtype=np.int64)
ALAW = np.array([alaw_to_s16(c) for c in range(256)], dtype=np.int64)


def same_bits(got, ref):
    """Elementwise: equal bit patterns, or NaN where the reference is NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape,
                                                               ref.shape)
    u = {4: np.uint32, 8: np.uint64}[ref.dtype.itemsize]
    return np.where(np.isnan(ref), np.isnan(got), got.view(u) == ref.view(u))


def _frames(kind, ch, rng, F=96):
    if kind == "int32":
        return rng.integers(-2**31, 2**31, (F, ch)).astype(np.float64) / 2147483648.0
    if kind == "float32":
        x = rng.uniform(-1, 1, (F, ch)) * 10.0 ** rng.integers(-44, 38, (F, ch))
        return x.astype(np.float32).astype(np.float64)
    if kind == "float64":
        return rng.uniform(-1, 1, (F, ch)) * 10.0 ** rng.integers(-300, 300, (F, ch))
    return np.full((F, ch), -0.0)


@pytest.mark.parametrize("kind", ["int32", "float32", "float64", "negzero"])
def test_channel_mean_model_is_numpy_mean_bitwise(kind):
    rng = np.random.default_rng(128)
    for ch in range(1, 129):
        x = np.ascontiguousarray(_frames(kind, ch, rng))
        with np.errstate(all="ignore"):
            ref = x.mean(axis=1) if ch > 1 else x[:, 0]
            got = channel_mean_model(x)
        ok = same_bits(got, ref)
        assert ok.all(), (kind, ch, int(np.count_nonzero(~ok)), got[~ok][:3], ref[~ok][:3])


def test_negative_zero_frame():
    """All channels -0.0: numpy's mean is +0.0 from two channels up, and a
    mono file (no mean taken) keeps its -0.0."""
    for ch in range(2, 129):
        m = np.full((3, ch), -0.0).mean(axis=1)
        assert not np.signbit(m).any(), ch
        assert not np.signbit(channel_mean_model(np.full((3, ch), -0.0))).any(), ch
    assert np.signbit(channel_mean_model(np.full((3, 1), -0.0))).all()
    # one +0.0 among them, at either end, changes nothing
    for ch in (2, 7, 8, 9, 17):
        for pos in (0, ch - 1):
            x = np.full((1, ch), -0.0)
            x[0, pos] = 0.0
            assert not np.signbit(channel_mean_model(x)).any()
            assert not np.signbit(x.mean(axis=1)).any()


def test_g711_closed_form_is_audioop():
    import audioop
    codes = bytes(range(256))
    assert np.array_equal(ULAW, np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2"))
    assert np.array_equal(ALAW, np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2"))
    assert (ULAW[0x00], ULAW[0x80], ULAW[0x7F], ULAW[0xFF]) == (-32124, 32124, 0, 0)
    assert (ALAW[0x55], ALAW[0xD5], ALAW[0x2A], ALAW[0xAA]) == (-8, 8, -32256, 32256)
    # both tables are odd-symmetric in the sign bit and monotone per half
    assert np.array_equal(ULAW[:128], -ULAW[128:]) and np.array_equal(ALAW[:128], -ALAW[128:])
    assert len(set(ULAW.tolist())) == 255 and len(set(ALAW.tolist())) == 256
