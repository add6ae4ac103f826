"""What the C-ABI harnesses of test_gpu_fastconv.py and test_gpu_partconv.py
share: the sentinels, bit views, the lazily imported package modules, the
expected history and the direct kernel on the same rows."""
import numpy as np
import torch

SENT = 1.0e3
YSENT = np.array([0xCAFEF00D], dtype=np.uint32).view(np.int32)[0].item()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _design():
    from dspcore import design
    return design


def _ops():
    from dspcore import ops
    return ops


def _tail(hist, x, L):
    """The last L samples of (hist | x) per row (device tensors)."""
    if hist is None:
        hist = torch.zeros((x.shape[0], L), dtype=x.dtype, device=x.device)
    cat = torch.cat([hist, x], dim=1)
    return cat[:, cat.shape[1] - L:]


def _direct(x, taps, offset, n_out):
    """The direct kernel on the same rows: y [B, n_out]."""
    design = _design()
    n = int(x.shape[1])
    src = design.SrcPlan(1, 1, int(taps.size), np.asarray(taps, np.float64), offset, n, n_out, 0)
    return _ops().src_polyphase(x.contiguous(), src)
