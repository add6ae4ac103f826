"""A numpy model of k_fastconv's arithmetic (csrc/fft_conv.hip,
include/dspcore_fastconv.h) and the cases its tests share.

The model is the kernel's algorithm step by step -- overlap-save blocks of
V = N - (K - 1) outputs, two consecutive blocks of one row as the real and
imaginary parts of one complex transform, the product with Hf = FFT(taps) / N,
and the inverse as conj(FFT(conj(.))) -- in complex64 through scipy.fft.  It is
the CPU stand-in for the kernel (tests/test_fastconv_plan.py holds it to the
GPU test's bound at the GPU test's shapes) and its documentation; it differs
from the kernel in how the transforms round (pocketfft tables its twiddles,
the kernel forms them by powering, ~4 ulp), which the bound's margin covers.

Reference: float64 np.convolve of the float32 data.  Bound: |err| <= BOUND_REL
* ||taps||_2 * max|x| (2e-6: four times the model's worst error over uniform
noise through sinc low-passes, SRC taps and decaying-noise responses of 121 to
8193 taps, 5.0e-7).
"""
import functools

import numpy as np
import scipy.fft

BOUND_REL = 2e-6
SIZES = (64, 512, 4096, 16384)
TPB = {64: 64, 512: 8, 4096: 1, 16384: 1}       # csrc/fft_pass.h Plan<log2 N>::TPB


def tap_counts(N):
    return (1, 2, N // 4 + 1, N // 2, N // 2 + 1)


def offsets(K):
    return sorted({0, (K - 1) // 2, K - 1})


def row_lengths(N, K):
    V = N - (K - 1)
    return sorted({n for n in (1, V - 1, V, V + 1, 2 * V, 2 * V + 1, 3 * V + 5) if n >= 1})


@functools.lru_cache(maxsize=None)
def make_taps(K, zero_at=None):
    """Seeded decaying noise, float32; zero_at: one tap set to an exact zero."""
    rng = np.random.default_rng(1000 + K)
    h = rng.standard_normal(K) * np.exp(-3.0 * np.arange(K) / K)
    h = (h / np.sqrt(np.sum(h * h))).astype(np.float32)
    if K == 1:
        h[0] = np.float32(0.75)
    if zero_at is not None:
        h[zero_at] = 0.0
    h.setflags(write=False)
    return h


def impulse_positions(N, K, n):
    V = N - (K - 1)
    return [min(p, n - 1) for p in (0, K - 1, V - 1, V, n - 1)]


@functools.lru_cache(maxsize=None)
def make_rows(N, K, n):
    """9 rows of n float32 samples: impulses of amplitude 1 at 0, K - 1, V - 1,
    V and the last sample (clipped into the row), two tones, seeded noise."""
    x = np.zeros((9, n), dtype=np.float32)
    for r, p in enumerate(impulse_positions(N, K, n)):
        x[r, p] = 1.0
    j = np.arange(n, dtype=np.int64)
    x[5] = np.cos(2 * np.pi * ((3 * j) % N) / N)
    x[6] = 0.5 * np.cos(2 * np.pi * (((N // 2 - 1) * j) % N) / N)
    x[7:] = np.random.default_rng(N * 31 + K * 7 + n).uniform(-1, 1, (2, n))
    x.setflags(write=False)
    return x


def bound(taps, x):
    t = np.asarray(taps, dtype=np.float64)
    m = float(np.max(np.abs(x))) if np.size(x) else 0.0
    return BOUND_REL * float(np.sqrt(np.sum(t * t))) * m


def full_reference(x, taps, hist=None):
    """np.convolve(history | row, taps) in float64 for every row of x [B, n],
    from the row's sample 0 on: [B, n + K - 1] ('full').  A row with at most 8
    non-zero samples is summed tap set by tap set (the same float64 terms)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(taps, dtype=np.float64)
    K = h.size
    B, n = x.shape
    out = np.zeros((B, n + K - 1))
    for b in range(B):
        row = x[b] if hist is None else np.concatenate([np.asarray(hist[b], np.float64), x[b]])
        skip = 0 if hist is None else K - 1
        nz = np.flatnonzero(row)
        if nz.size <= 8 and np.all(np.isfinite(row)):
            full = np.zeros(row.size + K - 1)
            for p in nz:
                full[p:p + K] += row[p] * h
        else:
            full = np.convolve(row, h) if row.size else np.zeros(K - 1)
        out[b] = full[skip:skip + n + K - 1]
    return out


def model(x, taps, log2n, offset=0, n_out=None, hist=None):
    """The kernel's arithmetic for the rows of x [B, n] (float32) -> float32
    [B, n_out]; hist [B, K - 1] is the history before sample 0 (zeros)."""
    x = np.asarray(x, dtype=np.float32)
    t32 = np.asarray(taps, dtype=np.float32)
    B, n = x.shape
    K, N = t32.size, 1 << log2n
    V = N - (K - 1)
    n_out = n if n_out is None else n_out
    hf = (np.fft.fft(t32.astype(np.float64), N) / N).astype(np.complex64)
    pairs = -(-n_out // (2 * V))
    # the stream from index -(K - 1) on, zeros past the row
    s = np.zeros((B, (K - 1) + max(n, 2 * pairs * V + offset)), dtype=np.float32)
    if hist is not None:
        s[:, :K - 1] = hist
    s[:, K - 1:K - 1 + n] = x
    blocks = -(-n_out // V)
    y = np.zeros((B, 2 * pairs * V), dtype=np.float32)
    for q in range(pairs):
        a0 = 2 * q * V + offset              # block 2q's sample 0 in s
        z = s[:, a0:a0 + N].astype(np.complex64)
        if 2 * q + 1 < blocks:
            z = z + 1j * s[:, a0 + V:a0 + V + N].astype(np.complex64)
        A = scipy.fft.fft(z.astype(np.complex64), axis=-1)
        C = np.conj(A * hf).astype(np.complex64)
        D = scipy.fft.fft(C, axis=-1)
        y[:, 2 * q * V:(2 * q + 1) * V] = D.real[:, K - 1:]
        y[:, (2 * q + 1) * V:(2 * q + 2) * V] = -D.imag[:, K - 1:]
    return y[:, :n_out]
