"""bench.py --dump-outputs: a plain run (no --full) writes the y, z and |X| of
its last timed step -- the same seeded channel rows of each, float32 -- and
they are bitwise what Chain.run returns for the benchmark's seeded input, from
run to run.  96 channels of the config-3 geometry: more rows than the dump
keeps, so the row sample is exercised; one process, bench.main called in it."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHANNELS = 96


def _run(tmp, capsys, monkeypatch):
    import bench
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "DSP_BENCH_DRYRUN", "DSP_BENCH_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main(["--gpus", "1", "--config", "c3", "--channels", str(CHANNELS), "--steps", "2",
                "--warmup", "1", "--dump-outputs", str(tmp)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    return json.loads(lines[0]), {n: np.load(tmp / f"{n}.npy") for n in ("y", "z", "mag")}


def test_plain_run_dumps_the_last_steps_outputs(gpu, tmp_path, capsys, monkeypatch):
    import bench
    from dspcore.chain import Chain, ChainConfig
    line, got = _run(tmp_path / "a", capsys, monkeypatch)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    # (ms_per_step is printed to 1e-4 ms: 1 % of a step of ~0.01 ms or more)
    assert line["value"] == pytest.approx(CHANNELS * 48000 / (line["ms_per_step"] * 1e-3) / 1e6,
                                          rel=1e-2)
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    # a plain run measures nothing beside the timed steps
    for k in ("roofline", "kernels_ms", "cpu_baseline", "config4", "ratio_sweep", "fft_2_28"):
        assert k not in line, k
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["mag.npy", "y.npy", "z.npy"]

    # the same rows from Chain.run on the benchmark's input (bench.measure)
    wl = bench.WORKLOADS["c3"]
    cfg = ChainConfig(wl["n_in"], wl["fs"], wl["L"], wl["M"], wl["num_taps"], bench.CONFIG3_GAINS,
                      n_fft=wl["n_fft"])
    gen = torch.Generator(device=gpu).manual_seed(1000)
    x = torch.rand((CHANNELS, wl["n_in"]), generator=gen, device=gpu, dtype=torch.float32)
    x.mul_(2).sub_(1)
    y, z, mag = Chain(cfg, CHANNELS, gpu, plan_batch=CHANNELS).run(x)
    idx = np.sort(np.random.default_rng(2024).choice(CHANNELS, 64, replace=False))
    assert len(set(idx.tolist())) == 64
    for name, ref in (("y", y), ("z", z), ("mag", mag)):
        a = got[name]
        assert a.dtype == np.float32 and a.shape == (64, ref.shape[1]), name
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
        assert np.array_equal(a, ref.cpu().numpy()[idx]), name
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # a second run with the same arguments: identical input, identical dump
    _, again = _run(tmp_path / "b", capsys, monkeypatch)
    for name in got:
        assert np.array_equal(got[name], again[name]), name
