"""A numpy model of the partitioned fast convolution's arithmetic
(csrc/fft_pconv.hip, include/dspcore_partconv.h) and the cases its tests share.

The model is the kernels' algorithm step by step: V = N/4, P = H = N/2, the
taps as S partitions of P, pair q of a row the complex64 transform Z_q of
z[n] = u'[q H - 3 V + n] + i u'[q H - 2 V + n] (u' the stream at absolute
positions, shifted by the offset), W_q = sum_s Z_(q-s) Hf[s] in ascending s,
D = FFT(conj(W_q)), outputs [q H, q H + V) = Re D[3 V:], [q H + V, q H + 2 V) =
-Im D[3 V:].  A call at stream position `pos` knows the samples up to its own
end only: its last, partial pair is transformed against zeros.  The model
differs from the kernels in how the transforms and the sum round (pocketfft,
numpy's complex64 product against the kernels' fused multiply-adds), which the
bound's margin covers.

Reference: float64 np.convolve of the float32 data.  Bound:
fastconv_model.BOUND_REL * ||taps||_2 * max|x|, unchanged.
"""
import functools

import numpy as np
import scipy.fft

import fastconv_model as fm

SIZES = (64, 512, 4096)
TPB = {64: 64, 512: 8, 4096: 1, 16384: 1}       # csrc/fft_pass.h Plan<log2 N>::TPB


def geometry(N, K):
    """(V, H = P, S, hist_len)."""
    V, H = N // 4, N // 2
    S = -(-K // H)
    return V, H, S, S * H + 3 * V


def tap_counts(N):
    P = N // 2
    return (P, P + 1, 2 * P, 2 * P + 1, 5 * P - 3) + ((2049,) if N == 64 else ())


def offsets(K):
    return sorted({0, (K - 1) // 2, K - 1})


def row_lengths(N):
    H = N // 2
    return (1, H - 1, H, H + 1, 2 * H + 1, 3 * H + 5)


def impulse_positions(N, n):
    return [min(p, n - 1) for p in (0, N // 2 - 1, N // 2, N // 4, n - 1)]


@functools.lru_cache(maxsize=None)
def make_rows(N, n):
    """9 rows of n float32 samples: impulses of amplitude 1 at 0, P - 1, P, V
    and the last sample (clipped into the row), two tones, seeded noise."""
    x = np.zeros((9, n), dtype=np.float32)
    for r, p in enumerate(impulse_positions(N, n)):
        x[r, p] = 1.0
    j = np.arange(n, dtype=np.int64)
    x[5] = np.cos(2 * np.pi * ((3 * j) % N) / N)
    x[6] = 0.5 * np.cos(2 * np.pi * (((N // 2 - 1) * j) % N) / N)
    x[7:] = np.random.default_rng(N * 31 + n).uniform(-1, 1, (2, n))
    x.setflags(write=False)
    return x


def hf_tables(taps, N):
    """[S, N] complex64: the float64 FFT of each float32 partition, zero-padded,
    divided by N, rounded once."""
    t32 = np.asarray(taps, dtype=np.float32)
    P = N // 2
    S = -(-t32.size // P)
    parts = np.zeros((S, P))
    parts.reshape(-1)[:t32.size] = t32
    return (np.fft.fft(parts, N, axis=-1) / N).astype(np.complex64)


def model(x, taps, log2n, offset=0, n_out=None, pos=0):
    """The kernels' arithmetic for one call at stream position `pos`.  x [B,
    pos + n_in] float32 is the stream from its sample 0 to the END OF THIS CALL
    (the call's own rows are x[:, pos:]); returns float32 [B, n_out] (default
    n_in)."""
    x = np.asarray(x, dtype=np.float32)
    B, end = x.shape
    N = 1 << log2n
    K = np.asarray(taps).size
    V, H, S, _ = geometry(N, K)
    n_out = end - pos if n_out is None else n_out
    hf = hf_tables(taps, N)
    qfirst = (-offset) // H

    def sample_block(a0):                   # u'[a0 : a0 + N]
        out = np.zeros((B, N), dtype=np.float32)
        lo = a0 + offset
        s0, s1 = max(lo, 0), min(lo + N, end)
        if s1 > s0:
            out[:, s0 - lo:s1 - lo] = x[:, s0:s1]
        return out

    spectra = {}

    def Z(q):
        if q not in spectra:
            z = sample_block(q * H - 3 * V) + 1j * sample_block(q * H - 2 * V)
            spectra[q] = scipy.fft.fft(z.astype(np.complex64), axis=-1)
        return spectra[q]

    y = np.zeros((B, n_out), dtype=np.float32)
    if n_out == 0:
        return y
    for q in range(pos // H, -(-(pos + n_out) // H)):
        W = np.zeros((B, N), dtype=np.complex64)
        for s in range(min(S, q - qfirst + 1)):
            W = (W + Z(q - s) * hf[s]).astype(np.complex64)
        D = scipy.fft.fft(np.conj(W), axis=-1)
        for blk, vals in ((0, D.real[:, 3 * V:]), (1, -D.imag[:, 3 * V:])):
            m0 = q * H + blk * V - pos
            lo, hi = max(m0, 0), min(m0 + V, n_out)
            if hi > lo:
                y[:, lo:hi] = vals[:, lo - m0:hi - m0]
    return y


def model_stream(x, taps, log2n, cuts):
    """x [B, n] through model() block by block (causal, n_out = n_in)."""
    outs, pos = [], 0
    for c in cuts:
        outs.append(model(x[:, :pos + c], taps, log2n, pos=pos))
        pos += c
    assert pos == x.shape[1]
    return np.concatenate(outs, axis=1)


make_taps, bound, full_reference = fm.make_taps, fm.bound, fm.full_reference
