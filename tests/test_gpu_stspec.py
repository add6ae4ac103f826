"""The stream spectrum on the GPU (include/dspcore_stspec.h, csrc/stft_stream.hip
k_stft_stream, dspcore.stspec.StreamSpectrum), through the C ABI and the class.

Sizes N = 32, 512, 4096, 16384: Plan<log2 N - 1> packs 256, 16, 2 and 1
transforms per workgroup, so packed and single-transform workgroups run, and
16384 has the largest LDS image.  hop = N/4 + 1 everywhere, so consecutive
frames start at alternating 8-byte alignment (both loader paths) and never on a
block boundary for long.

The C-ABI harness (_stream) keeps 1.0e3 in everything the kernel must not read
(the block's padding, carry_in past carry_len, both carry buffers before the
first push) and the sentinel bits 0xCAFEF00D in the padding of the mag rows,
and checks after every call that the sentinels are intact and that
carry_out[:carry_out_len] is bitwise the stream's last samples.  The carry
pitch is N + 1 (rows at every 4-byte residue); the class has aligned rows.

One reference per size (float64 rfft of the windowed float32 samples) is
computed once and shared.  Every case prints its worst error / bound ratio.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_fft_family import AMP, IN_PAD, R, _bits, _Out, _pad_in, _ratios, _window
from test_gpu_parity import CHAIN_MAG_RTOL, FFT_RTOL, _traced

pytestmark = pytest.mark.gpu

SIZES = (32, 512, 4096, 16384)
TPB = {32: 256, 512: 16, 4096: 2, 16384: 1}     # csrc/fft_pass.h Plan<log2 N - 1>::TPB


def _hop(N):
    return N // 4 + 1


def _sizes(N):
    return [0, 1, _hop(N) - 1, N - 1, N, N + 1, 3 * N + 5]


def _total(N):
    return sum(_sizes(N))


def _parts(N):
    """name -> (blocks, column offset of block i in its buffer, pitch parity)."""
    s = _sizes(N)
    return {
        "one": ([_total(N)], lambda i: 0, 0),                 # even pitch: aligned rows
        "ragged": (s, lambda i: 0, 1),                        # odd pitch: rows alternate
        "reversed": (s[::-1], lambda i: 0, 1),
        "views": ([N + 1, 3 * N + 5, 0, N - 1, 1, _hop(N) - 1, N], lambda i: 1 + i % 3, 1),
    }


def _design():
    from dspcore import design
    return design


def _ops():
    from dspcore import ops
    return ops


@functools.lru_cache(maxsize=None)
def _base(N):
    """11 rows of _total(N) samples: impulses, two tones, seeded noise."""
    total = _total(N)
    x = np.zeros((R, total), dtype=np.float32)
    for r, p in enumerate((0, N - 1, N, total - 1)):
        x[r, p] = AMP
    j = np.arange(total, dtype=np.int64)
    x[4] = AMP * np.cos(2 * np.pi * ((3 * j) % N) / N)
    x[5] = AMP * np.cos(2 * np.pi * (((N // 2 - 1) * j) % N) / N)
    x[6:] = np.random.default_rng(N).uniform(-1, 1, (R - 6, total))
    x.setflags(write=False)
    return x


def _frames_ref(x, N, hop, w):
    """|rfft| in float64 of every zero-padded frame of the float32 rows times
    the (float32-valued) window w -> [rows, frames, N/2 + 1]."""
    rows, total = x.shape
    F = _design().stft_plan(total, N, hop).frames
    pad = np.zeros((rows, (F - 1) * hop + N))
    pad[:, :total] = x
    idx = hop * np.arange(F)[:, None] + np.arange(N)[None, :]
    return np.abs(np.fft.rfft(pad[:, idx] * np.asarray(w, dtype=np.float64), axis=-1))


@functools.lru_cache(maxsize=None)
def _hann_ref(N):
    w32 = _design().hann(N).astype(np.float32)
    ref = _frames_ref(_base(N), N, _hop(N), w32)
    ref.setflags(write=False)
    return ref


def _stream(gpu, N, hop, wdev, x, blocks, lead=lambda i: 0, odd=1, tag=""):
    """The rows of x [B, total] (device) through dsp_stspec_mag_f32 block by
    block, then the flush; returns every frame, [B, stft_plan frames, N/2 + 1]."""
    from dspcore import _lib
    design = _design()
    lib = _lib.load()
    B, total = x.shape
    assert sum(blocks) == total
    lg, half = N.bit_length() - 1, N // 2 + 1
    ldc, ldm = N + 1, half + 3
    carry = torch.full((2, B, ldc), IN_PAD, dtype=torch.float32, device=gpu)
    tw = _ops()._table("tw", N, gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    seen, cur, outs = 0, 0, []
    for i, n in enumerate(list(blocks) + [None]):
        flush = n is None
        n = 0 if flush else n
        p = design.stream_stft_plan(N, hop, seen, n, flush)
        carry[1 - cur].fill_(IN_PAD)
        ld = ((n + 4) | 1) if odd else ((n + 5) & ~1)
        blk = _pad_in(x[:, seen:seen + n], ld, lead(i)) if n else None
        out = _Out(gpu, B * p.frames, half, ldm, False)
        rc = lib.dsp_stspec_mag_f32(
            carry[cur].data_ptr(), carry[1 - cur].data_ptr(), ldc,
            blk.data_ptr() if n else None, ld if n else 0, n,
            out.view.data_ptr() if p.frames else None, ldm, B, lg, hop, seen, int(flush),
            wdev.data_ptr(), tw.data_ptr(), stream)
        assert rc == 0, (tag, i, _lib.last_error())
        out.check(f"{tag} call {i}")
        seen += n
        col = p.carry_out_len
        got = carry[1 - cur]
        assert torch.equal(_bits(got[:, :col]), _bits(x[:, seen - col:seen])), (tag, i, "carry")
        assert bool((got[:, col:] == IN_PAD).all()), (tag, i, "carry_out past carry_out_len")
        assert bool((carry[cur, :, p.carry_len:] == IN_PAD).all()), (tag, i, "carry_in written")
        cur = 1 - cur
        outs.append(out.view.reshape(B, p.frames, half).clone())
    res = torch.cat(outs, dim=1)
    assert res.shape[1] == design.stft_plan(total, N, hop).frames, tag
    return res


def _flat(a):
    return np.asarray(a, dtype=np.float64).reshape(-1, a.shape[-1])


def _report(what, N, worst):
    print(f"[stspec] {what} N={N}: worst err / bound = {worst:.3f}")


# --------------------------------------------------------------------------- load mapping
def _map_blocks(N):
    return [N + 3, _hop(N) + 2, N - 1, 5]


def _map_positions(N):
    """Stream positions relative to the second call of _map_blocks: the last
    carried sample, the block's first sample, sample 0 and N - 1 of frame 2,
    and the two samples on either side of the next block boundary."""
    hop = _hop(N)
    b = _map_blocks(N)
    s1, s2 = b[0], b[0] + b[1]
    carried = _design().stream_stft_plan(N, hop, s1, 0).carry_len
    assert carried >= 1
    return [s1 - 1, s1, 2 * hop, 2 * hop + N - 1, s2 - 1, s2]


@pytest.mark.parametrize("N", SIZES)
def test_load_mapping_sample_by_sample(gpu, N):
    """An impulse of 0.75 at stream position p gives 0.75 w[p - f hop] in every
    bin of every frame f that covers it and exact zeros elsewhere (ramp window:
    exact in float32, nowhere zero, every position 0.75 / N from the next)."""
    hop = _hop(N)
    w, w32 = _window(N)
    blocks = _map_blocks(N)
    pos = _map_positions(N)
    total = sum(blocks)
    x = np.zeros((len(pos), total), dtype=np.float32)
    x[np.arange(len(pos)), pos] = AMP
    F = _design().stft_plan(total, N, hop).frames
    i = np.asarray(pos)[:, None] - hop * np.arange(F)[None, :]           # [rows, F]
    val = np.where((i >= 0) & (i < N), AMP * w[np.clip(i, 0, N - 1)], 0.0)
    assert (val > 0).sum(1).min() >= 2                                   # several frames cover p
    ref = np.repeat(val[:, :, None], N // 2 + 1, axis=2)
    got = _stream(gpu, N, hop, torch.from_numpy(w32).to(gpu), torch.from_numpy(x).to(gpu),
                  blocks, lambda k: k % 4, tag=f"map N={N}")
    _report("load mapping", N, _ratios(_flat(got.cpu().numpy()), _flat(ref), f"map N={N}"))


# --------------------------------------------------------------------------- partitions
@pytest.mark.parametrize("N", SIZES)
def test_partition_invariance_bitwise_and_accuracy(gpu, N):
    """The 11 base rows as one block, then as ragged partitions (a 0-sample
    push, blocks as views at column offsets 1, 2, 3 of an odd-pitch buffer):
    every frame, the flush's included, bitwise the same; stft_plan's count; and
    within FFT_RTOL of float64 (Hann window)."""
    hop = _hop(N)
    wdev = _ops()._table("hann", N, gpu)
    x = torch.from_numpy(_base(N).copy()).to(gpu)
    got = {}
    for name, (blocks, lead, odd) in _parts(N).items():
        got[name] = _stream(gpu, N, hop, wdev, x, blocks, lead, odd, tag=f"{name} N={N}")
    for name, res in got.items():
        assert torch.equal(_bits(res), _bits(got["one"])), f"N={N}: partition {name} differs"
    worst = _ratios(_flat(got["one"].cpu().numpy()), _flat(_hann_ref(N)), f"accuracy N={N}")
    _report("partitions", N, worst)


@pytest.mark.parametrize("N", SIZES)
def test_class_accuracy_against_float64_and_the_one_shot_stft(gpu, N):
    """StreamSpectrum (aligned carry rows, Hann table) over the ragged
    partition: bitwise the C-ABI run's frames, within FFT_RTOL max|ref| per
    frame of float64, within 2 FFT_RTOL max|ref| per frame of
    ops.stft_magnitude on the whole signal; N = 32 also against the oracle."""
    from dspcore.stspec import StreamSpectrum
    hop, total = _hop(N), _total(N)
    x = torch.from_numpy(_base(N).copy()).to(gpu)
    ss = StreamSpectrum(N, hop, batch=R, max_block=3 * N + 5, device=gpu)
    outs, seen = [], 0
    for n in _sizes(N):
        m = ss.push(x[:, seen:seen + n])
        assert m.shape == (R, _design().stream_stft_plan(N, hop, seen, n).frames, N // 2 + 1)
        outs.append(m.clone())
        seen += n
    outs.append(ss.flush().clone())
    got = torch.cat(outs, dim=1)
    F = _design().stft_plan(total, N, hop).frames
    assert got.shape[1] == F == ss.frames_emitted and ss.samples == total
    abi = _stream(gpu, N, hop, ss.window, x, [total], odd=0, tag=f"class N={N}")
    assert torch.equal(_bits(got), _bits(abi))
    ref = _hann_ref(N)
    g = got.cpu().numpy()
    worst = _ratios(_flat(g), _flat(ref), f"class N={N}")
    one = _ops().stft_magnitude(x, N, hop, F).cpu().numpy().astype(np.float64)
    err = np.max(np.abs(g - one), axis=2)
    top = np.max(ref, axis=2)
    assert np.all(err <= 2 * FFT_RTOL * top), (N, float(np.max(err / np.maximum(top, 1e-300))))
    print(f"[stspec] vs one-shot N={N}: worst err / (2 bound) = "
          f"{float(np.max(err[top > 0] / (2 * FFT_RTOL * top[top > 0]))):.3f}")
    if N == 32:
        from oracle import dsp_ref_cpu as orc
        for r in range(R):
            rmag = orc.spectrogram(_base(N)[r].astype(np.float64), N, hop, F)
            assert np.max(np.abs(g[r] - rmag)) <= CHAIN_MAG_RTOL * np.max(rmag), r
    _report("class", N, worst)


# --------------------------------------------------------------------------- wide batch
@pytest.mark.parametrize("N", SIZES)
def test_wide_batch_is_the_base_rows_bitwise(gpu, N):
    """base[arange(B) % 11] with B x 3 frames odd and above 2 TPB (171 rows at
    N = 32): full workgroups and a last one with dead transforms; every row is
    bitwise its base row, in a push that starts from a carry too."""
    hop = _hop(N)
    B = 171 if N == 32 else 13
    assert (B * 3) % 2 == 1 and B * 3 > 2 * TPB[N]
    n1 = N + 2 * hop                                   # 3 frames
    blocks = [n1, 3 * hop, _total(N) - n1 - 3 * hop]
    assert _design().stream_stft_plan(N, hop, 0, n1).frames == 3
    assert _design().stream_stft_plan(N, hop, n1, 3 * hop).frames == 3
    wdev = _ops()._table("hann", N, gpu)
    base = torch.from_numpy(_base(N).copy()).to(gpu)
    idx = torch.arange(B, device=gpu) % R
    narrow = _stream(gpu, N, hop, wdev, base, blocks, tag=f"base N={N}")
    wide = _stream(gpu, N, hop, wdev, base[idx], blocks, tag=f"wide N={N}")
    same = (_bits(wide) == _bits(narrow)[idx]).flatten(1).all(1)
    assert bool(same.all()), f"N={N}: wide rows {torch.nonzero(~same).flatten()[:8].tolist()}"


# --------------------------------------------------------------------------- launches
def test_a_push_is_two_launches(gpu):
    from dspcore.stspec import StreamSpectrum
    ss = StreamSpectrum(512, 128, batch=3, max_block=1000, device=gpu)
    x = torch.from_numpy(_base(512)[:3, :1000].copy()).to(gpu)
    (m,), names = _traced(lambda: (ss.push(x),))
    assert names == ["stspec", "stspec_nf"], names
    assert m.shape == (3, 1 + (1000 - 512) // 128, 257)
    (m,), names = _traced(lambda: (ss.push(x[:, :7]),))
    assert names == ["stspec", "stspec_nf"] and m.shape[1] == 0, names


# --------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("N", (32, 512))
def test_non_finite_samples_get_the_reference_classes(gpu, N):
    """A NaN, a +inf and a -inf, each alone in a noise row, at the load-mapping
    positions (around the ragged partition's N-sample block) and at a frame's sample 0,
    where the Hann zero makes the windowed sample NaN.  Frames that cover the
    sample: NaN mask and +inf mask are ops.stft_magnitude's (and the oracle's at
    N = 32); frames that do not are bitwise the clean run's -- in every
    partition, which move the sample between carry and block."""
    design = _design()
    hop, total = _hop(N), _total(N)
    sz = _sizes(N)
    s1 = sum(sz[:4])                                   # before the N-sample block
    carried = design.stream_stft_plan(N, hop, s1, 0).carry_len
    assert carried >= 1
    assert s1 - carried == hop                         # frame 1 is the first that block completes
    pos = [s1 - 1, s1, 2 * hop, 2 * hop + N - 1, s1 + N - 1, s1 + N, 3 * hop]
    vals = [float("nan"), float("inf"), float("-inf")]
    clean = _base(N)[7]
    x = np.tile(clean, (1 + len(pos) * len(vals), 1))
    where = [None]
    for p in pos:
        for v in vals:
            x[len(where), p] = v
            where.append(p)
    F = design.stft_plan(total, N, hop).frames
    cover = np.zeros((x.shape[0], F), dtype=bool)
    for r, p in enumerate(where):
        if p is not None:
            f = np.arange(F)
            cover[r] = (f * hop <= p) & (p < f * hop + N)
    assert cover[1:].any(1).all()
    xd = torch.from_numpy(x).to(gpu)
    wdev = _ops()._table("hann", N, gpu)
    one = _ops().stft_magnitude(xd, N, hop, F).cpu().numpy()
    assert not np.isfinite(one[cover]).any() and np.isfinite(one[~cover]).all()
    masks = [(np.isnan(one), np.isposinf(one), "ops.stft_magnitude")]
    if N == 32:
        from oracle import dsp_ref_cpu as orc
        with np.errstate(all="ignore"):
            o = np.stack([orc.spectrogram(r.astype(np.float64), N, hop, F) for r in x])
        masks.append((np.isnan(o), np.isposinf(o), "oracle"))
    for name, (blocks, lead, odd) in _parts(N).items():
        got = _stream(gpu, N, hop, wdev, xd, blocks, lead, odd, tag=f"nf {name} N={N}").cpu().numpy()
        for nan, inf, who in masks:
            assert np.array_equal(np.isnan(got)[cover], nan[cover]), (N, name, who, "NaN mask")
            assert np.array_equal(np.isposinf(got)[cover], inf[cover]), (N, name, who, "inf mask")
        assert not np.isfinite(got[cover]).any()
        same = got.view(np.uint32) == got[0].view(np.uint32)[None]
        assert same[~cover].all(), (N, name, "a frame that does not cover the sample changed")


# --------------------------------------------------------------------------- state
def test_state_dict_reset_and_errors(gpu):
    from dspcore.stspec import StreamSpectrum
    N, hop = 512, _hop(512)
    x = torch.from_numpy(_base(N).copy()).to(gpu)
    blocks = [b for b in _sizes(N)]
    cut = 4

    def run(ss, parts, start):
        outs, seen = [], start
        for n in parts:
            outs.append(ss.push(x[:, seen:seen + n]).clone())
            seen += n
        return outs, seen

    a = StreamSpectrum(N, hop, batch=R, max_block=3 * N + 5, device=gpu)
    head, seen = run(a, blocks[:cut], 0)
    sd = a.state_dict()
    assert sd["samples"] == seen and sd["carry"].shape == (R, a.carry_len) and not sd["flushed"]
    tail_a, _ = run(a, blocks[cut:], seen)
    tail_a.append(a.flush().clone())
    b = StreamSpectrum(N, hop, batch=R, max_block=3 * N + 5, device=gpu)
    b._carry.fill_(IN_PAD)                              # nothing but the state is read
    b.load_state_dict(sd)
    assert (b.samples, b.frames_emitted) == (sd["samples"], sd["frames_emitted"])
    tail_b, _ = run(b, blocks[cut:], seen)
    tail_b.append(b.flush().clone())
    for ta, tb in zip(tail_a, tail_b):
        assert torch.equal(_bits(ta), _bits(tb))
    with pytest.raises(RuntimeError):
        b.push(x[:, :3])
    with pytest.raises(RuntimeError):
        b.flush()
    b.reset()                                           # starts over
    assert (b.samples, b.frames_emitted, b.flushed) == (0, 0, False)
    again, _ = run(b, blocks[:cut], 0)
    for ta, tb in zip(head, again):
        assert torch.equal(_bits(ta), _bits(tb))
    with pytest.raises(ValueError):
        StreamSpectrum(N, hop, batch=R - 1, max_block=64, device=gpu).load_state_dict(sd)
    for bad in (x[:R - 1, :8], x[:, :3 * N + 6], x[:, :8].double(), x[0, :8], x[:, :8].cpu()):
        with pytest.raises(ValueError):
            b.push(bad)
    for kw in (dict(n_fft=16), dict(n_fft=1 << 15), dict(n_fft=48), dict(n_fft=64, hop=0),
               dict(n_fft=64, hop=65), dict(n_fft=64, batch=0), dict(n_fft=64, max_block=0)):
        with pytest.raises(ValueError):
            StreamSpectrum(**{"batch": 2, "max_block": 64, "device": gpu, **kw})
    # an empty stream: one all-zero frame at the flush
    e = StreamSpectrum(64, 16, batch=2, max_block=64, device=gpu)
    m = e.flush()
    assert m.shape == (2, 1, 33) and not bool(m.any())
