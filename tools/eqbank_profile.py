"""What the EQ bank's table reads cost (manual GPU run): the single-sos
streaming cascade (k_iir_stream, coefficients and A^T in kernel arguments)
against the bank kernel (k_iir_bank, both read from the row's record) at one
shape, B x n with six stages (default 4096 x 2048), the bank with G = 1 (every
row reads one record) and with G = B distinct gain sets (every row its own
2.8 KB record).

The three are timed alternately in one process -- round r times each of them
over `reps` back-to-back calls between two device events -- so that a drift of
the machine meets all three alike.  Prints per variant the median over the
rounds, the spread (min .. max) and the rate, then one JSON line.

    python tools/eqbank_profile.py [--batch B] [--n N] [--rounds R] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "dsp-audio-project_amd"))

from dspcore import design, ops  # noqa: E402
from dspcore.eqbank import EqBank  # noqa: E402

FS = 72000
GAINS = {"Sub-Bass": 6, "Bass": -4, "Low Mids": 3, "High Mids": -3, "Presence": 5,
         "Brilliance": -6}


def timed_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    B, n = a.batch, a.n
    x = torch.rand((B, n), device=dev) * 2 - 1
    z = torch.empty_like(x)
    state = torch.zeros((B, 12), dtype=torch.float64, device=dev)
    sos = design.eq_plan(FS, GAINS).sos
    one = EqBank(FS, [GAINS] * B, n, dev)
    # B distinct settings: every slider moved by its own few hundredths of a dB
    own = [{k: v + 0.25 * (i + 1) / B for k, v in GAINS.items()} for i in range(B)]
    each = EqBank(FS, own, n, dev)
    assert one.G == 1 and each.G == B and one.max_stages == each.max_stages == 6
    variants = {
        "iir_stream": lambda: ops.biquad_cascade_state(x, sos, True, zi=state, out=z, zf=state),
        "iir_bank G=1": lambda: one.apply(x, zi=state, out=z, zf=state),
        f"iir_bank G={B}": lambda: each.apply(x, zi=state, out=z, zf=state),
    }
    for fn in variants.values():          # warm-up: code objects loaded, caches touched
        timed_ms(fn, 10)
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            state.zero_()
            ms[k].append(timed_ms(fn, a.reps))
    result = {"B": B, "n": n, "stages": 6, "rounds": a.rounds, "reps": a.reps}
    for k, v in ms.items():
        med = statistics.median(v)
        result[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v)}
        print(f"{k:>20}: median {med:.4f} ms  (min {min(v):.4f} .. max {max(v):.4f}, spread "
              f"{100 * (max(v) - min(v)) / med:.1f}%), {B * n / med / 1e6:.2f} G samples/s, "
              f"{B * n * 8 / med / 1e6:.0f} GB/s x+z", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
