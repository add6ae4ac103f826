"""StreamChain(..., spectrum=dict(n_fft=..., hop=...)): the running spectrogram
of z beside the stream's y and z.  y and z are bitwise those of the same chain
without a spectrum; the concatenated frames are, within 2 FFT_RTOL max|ref| per
frame, ops.stft_magnitude of the concatenated z (both are within FFT_RTOL of the
same truth), with stft_plan's frame count -- for one gains dict, per-channel
gains, the live EQ with a gain change mid-stream, and the SRC bypass."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_gains
from test_gpu_parity import FFT_RTOL

pytestmark = pytest.mark.gpu

FS, B, MAX_BLOCK = 48000, 3, 480
SPEC = dict(n_fft=512, hop=128)
BLOCKS = [480, 1, 0, 479, 333, 7, 480, 480, 64, 200, 480, 5, 91, 480, 300, 17, 480, 256, 33, 480]


def _gains():
    g = golden("eq")
    gains = golden_gains(g["gains_0"])            # config 3 (tests/golden/make_golden.py)
    assert int(g["fs_0"]) == 72000 and len(gains) == 6
    return gains


def _signal(gpu):
    rng = np.random.default_rng(2024)
    n = sum(BLOCKS)
    t = np.arange(n) / FS
    x = 0.4 * rng.uniform(-1, 1, (B, n)) + 0.5 * np.sin(2 * np.pi * 1000.0 * t)[None, :]
    return torch.from_numpy(x.astype(np.float32)).to(gpu)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(sc, x, blocks=BLOCKS, start=0, between=None, flush=True):
    """[(y, z, mag?) clones] of every push and the flush; between(i) runs
    before push i."""
    outs, seen = [], start
    for i, n in enumerate(blocks):
        if between is not None:
            between(i)
        outs.append(tuple(t.clone() for t in sc.push(x[:, seen:seen + n])))
        seen += n
    if flush:
        outs.append(tuple(t.clone() for t in sc.flush()))
    return outs


def _check(gpu, make, between=None):
    from dspcore import design, ops
    x = _signal(gpu)
    plain = _run(make(None), x, between=between)
    sc = make(SPEC)
    with_spec = _run(sc, x, between=between)
    assert len(plain) == len(with_spec) == len(BLOCKS) + 1
    for i, (p, s) in enumerate(zip(plain, with_spec)):
        assert len(p) == 2 and len(s) == 3
        assert torch.equal(_bits(p[0]), _bits(s[0])), f"y of call {i}"
        assert torch.equal(_bits(p[1]), _bits(s[1])), f"z of call {i}"
        assert s[2].shape[0] == B and s[2].shape[2] == SPEC["n_fft"] // 2 + 1
    z = torch.cat([s[1] for s in with_spec], dim=1)
    mag = torch.cat([s[2] for s in with_spec], dim=1).cpu().numpy().astype(np.float64)
    plan = design.stft_plan(z.shape[1], SPEC["n_fft"], SPEC["hop"])
    assert mag.shape[1] == plan.frames == sc.spec.frames_emitted and sc.spec.samples == z.shape[1]
    ref = ops.stft_magnitude(z, plan.n_fft, plan.hop, plan.frames).cpu().numpy().astype(np.float64)
    err = np.max(np.abs(mag - ref), axis=2)
    top = np.max(ref, axis=2)
    assert top.min() > 0
    ratio = float(np.max(err / (2 * FFT_RTOL * top)))
    print(f"[stream-spectrum] {plan.frames} frames: worst err / (2 FFT_RTOL max) = {ratio:.3f}")
    assert ratio <= 1.0, ratio
    return sc


def test_config3_stream_with_spectrum(gpu):
    from dspcore.stream import StreamChain
    sc = _check(gpu, lambda spec: StreamChain(FS, 3, 2, None, _gains(), B, MAX_BLOCK, gpu,
                                              spectrum=spec))
    assert sc.spec.max_block >= -(-MAX_BLOCK * 3 // 2)


def test_src_bypass_with_spectrum(gpu):
    from dspcore.stream import StreamChain
    _check(gpu, lambda spec: StreamChain(FS, 1, 1, None, _gains(), B, MAX_BLOCK, gpu,
                                         spectrum=spec))


def test_per_channel_gains_with_spectrum(gpu):
    from dspcore.stream import StreamChain
    g = _gains()
    per = [g, {k: -v for k, v in g.items()}, {k: 0.0 for k in g}]
    _check(gpu, lambda spec: StreamChain(FS, 3, 2, None, per, B, MAX_BLOCK, gpu, spectrum=spec))


def test_live_eq_with_a_gain_change_and_spectrum(gpu):
    """set_gains between two pushes: the reference is the STFT of that run's own z."""
    from dspcore.stream import StreamChain
    g = _gains()
    chains = []

    def make(spec):
        chains.append(StreamChain(FS, 3, 2, None, g, B, MAX_BLOCK, gpu, live=True, spectrum=spec))
        return chains[-1]

    def between(i):
        if i == 9:
            chains[-1].set_gains({k: -v for k, v in g.items()})

    _check(gpu, make, between)


def test_state_dict_round_trip_continues_bitwise(gpu):
    from dspcore.stream import StreamChain
    x = _signal(gpu)
    cut = 8
    a = StreamChain(FS, 3, 2, None, _gains(), B, MAX_BLOCK, gpu, spectrum=SPEC)
    _run(a, x, BLOCKS[:cut], flush=False)
    sd = a.state_dict()
    assert "spectrum" in sd and sd["spectrum"]["samples"] == a.produced
    seen = sum(BLOCKS[:cut])
    tail_a = _run(a, x, BLOCKS[cut:], start=seen)
    b = StreamChain(FS, 3, 2, None, _gains(), B, MAX_BLOCK, gpu, spectrum=SPEC)
    b.load_state_dict(sd)
    tail_b = _run(b, x, BLOCKS[cut:], start=seen)
    for ta, tb in zip(tail_a, tail_b):
        for u, v in zip(ta, tb):
            assert torch.equal(_bits(u), _bits(v))
    # without a spectrum the state dict has no new key, and reset() starts both over
    assert "spectrum" not in StreamChain(FS, 3, 2, None, _gains(), B, MAX_BLOCK, gpu).state_dict()
    b.reset()
    assert (b.spec.samples, b.spec.frames_emitted, b.spec.flushed) == (0, 0, False)
    first = _run(b, x, BLOCKS[:cut], flush=False)
    a.reset()
    for ta, tb in zip(_run(a, x, BLOCKS[:cut], flush=False), first):
        for u, v in zip(ta, tb):
            assert torch.equal(_bits(u), _bits(v))
