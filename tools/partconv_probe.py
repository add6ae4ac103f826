#!/usr/bin/env python3
"""A/B of the partitioned fast convolution (ops.partconv) on one GPU against
the route the same call took before it: the direct kernel (ops.src_polyphase,
L = M = 1) above 8193 taps, overlap-save in one transform (ops.fastconv) at
8193.  np.convolve's 'same' alignment, seeded uniform noise through seeded
decaying-noise taps.

    python tools/partconv_probe.py --all [--out FILE]
        every case of CASES, each in a fresh child process under its own time
        limit; stops at the first child that fails.
    python tools/partconv_probe.py --rows 4096 --n 48000 --taps 16384 --log2n 14 --against direct
        one case: prints one CASE line.  --against none times the new path alone.

One case: both paths on the same device buffers in one process, one warm-up
call each, then `reps` timed calls alternating old, new, old, new ... (device
events around each call, a synchronise after it), reps sized from the warm-up so
that the slower path's timed calls take about --budget seconds (2 <= reps <=
100).  The new path's ring is allocated once, outside the timed calls.
Reported per path: median, min and max in ms (the box's variation is the min ..
max spread), the largest |old - new| over the outputs, and for the new path its
algorithmic bytes -- x read once, y written once, every spectrum written once
(8 N bytes a pair) and read by the S pairs after it, 16 S bytes per output --
and their rate as a fraction of the 8 TB/s HBM peak.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsp-audio-project_amd"))

SHAPES = ((4096, 48000), (1, 441000))
HBM_PEAK = 8.0e12   # bytes / s
# (rows, n, K, log2n, against)
CASES = tuple((r, n, 8193, 14, "fastconv") for r, n in SHAPES) + tuple(
    (r, n, K, lg, "direct" if lg == 14 and K <= 65536 else "none")
    for r, n in SHAPES for K in (16384, 65536, 262144) for lg in (14, 13, 12, 11))


def one_case(rows, n, K, budget, log2n, against):
    import numpy as np
    import torch

    from dspcore import design, ops
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(K)
    h = rng.standard_normal(K) * np.exp(-3.0 * np.arange(K) / K)
    h /= np.sqrt(np.sum(h * h))
    plan = design.partconv_plan(h, log2n)
    off = (K - 1) // 2
    gen = torch.Generator(device=dev)
    gen.manual_seed(rows + n)
    x = torch.rand((rows, n), generator=gen, device=dev) * 2 - 1
    yo = torch.empty_like(x)
    yn = torch.empty_like(x)
    slots = ops.partconv_slots(plan, n, off)
    ws = ops.partconv_workspace(plan, rows, slots, dev)
    tables = ops.partconv_tables(plan, dev)
    paths = []
    if against == "direct":
        src = design.SrcPlan(1, 1, K, h, off, n, n, 0)
        paths.append(("old", lambda: ops.src_polyphase(x, src, out=yo)))
    elif against == "fastconv":
        fplan = design.fastconv_plan(h)
        paths.append(("old", lambda: ops.fastconv(x, fplan, off, n, out=yo)))
    paths.append(("new", lambda: ops.partconv(x, plan, off, n, ws=ws, slots=slots, out=yn,
                                               tables=tables)))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # warm-up (code objects, tables): its time only sizes the timed window.  An
    # old path that refuses the call (a status code before any launch: the
    # direct kernel keeps its tap bank in LDS) is reported and left out.
    refused = None
    if len(paths) == 2:
        try:
            timed(paths[0][1])
        except RuntimeError as e:
            if "(status -3)" not in str(e):     # only DSP_ENOTSUP: anything else ends the case
                raise
            refused = f"{against}: {e}"
            against = "none"
            paths = paths[1:]
    first = {name: timed(fn) for name, fn in paths}
    reps = int(max(2, min(100, budget * 1e3 / max(first.values()))))
    ms = {name: [] for name, _ in paths}
    for _ in range(reps):
        for name, fn in paths:
            ms[name].append(timed(fn))
    out = {"rows": rows, "n": n, "K": K, "log2n": plan.log2n, "S": plan.S, "reps": reps,
           "against": against, "ring_bytes": ws.numel(), "refused": refused}
    for name in ms:
        v = sorted(ms[name])
        out[name] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}
    if against != "none":
        out["max_abs_diff"] = float((yo - yn).abs().max())
        out["speedup"] = out["old"]["median_ms"] / out["new"]["median_ms"]
    H = plan.P
    pairs_fwd = -(-n // H) + -(-off // H)               # transformed per row
    nbytes = rows * (2 * n * 4 + pairs_fwd * 8 * plan.n_fft + 16 * plan.S * n)
    out["new_bytes"] = nbytes
    out["new_hbm_frac"] = nbytes / (out["new"]["median_ms"] * 1e-3) / HBM_PEAK
    return out


def fmt(c):
    f = c["new"]
    s = f"{c['rows']:>5} x {c['n']:<7} K={c['K']:<7} N=2^{c['log2n']:<3} S={c['S']:<4} reps={c['reps']:<4} "
    if c["against"] != "none":
        d = c["old"]
        s += (f"{c['against']:>8} {d['median_ms']:10.4f} ms [{d['min_ms']:.4f} .. {d['max_ms']:.4f}]   ")
    s += f"partconv {f['median_ms']:9.4f} ms [{f['min_ms']:.4f} .. {f['max_ms']:.4f}]   "
    if c["against"] != "none":
        s += f"{c['against']}/partconv {c['speedup']:8.2f}   "
    s += (f"bytes {c['new_bytes'] / 1e6:10.2f} MB = {100 * c['new_hbm_frac']:5.2f} % of HBM peak   "
          f"ring {c['ring_bytes'] / 1e9:6.2f} GB")
    if c["against"] != "none":
        s += f"   max|diff| {c['max_abs_diff']:.2e}"
    if c["refused"]:
        s += f"   [{c['refused']}]"
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--n", type=int, default=48000)
    ap.add_argument("--taps", type=int, default=16384)
    ap.add_argument("--log2n", type=int)
    ap.add_argument("--against", choices=("direct", "fastconv", "none"), default="direct")
    ap.add_argument("--budget", type=float, default=2.0,
                    help="seconds of timed calls of the slower path")
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child, seconds")
    a = ap.parse_args()
    if not a.all:
        print("CASE " + json.dumps(one_case(a.rows, a.n, a.taps, a.budget, a.log2n, a.against)),
              flush=True)
        return 0
    lines = []
    for rows, n, K, lg, against in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(rows), "--n", str(n),
               "--taps", str(K), "--log2n", str(lg), "--against", against, "--budget",
               str(a.budget)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"case {rows} x {n} K={K} 2^{lg}: no answer in {a.limit} s; stopping", flush=True)
            return 1
        case = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        if r.returncode != 0 or not case:
            print(f"case {rows} x {n} K={K} 2^{lg}: exit {r.returncode}; stopping\n"
                  f"{r.stderr[-2000:]}", flush=True)
            return 1
        lines.append(fmt(json.loads(case[0][5:])))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
