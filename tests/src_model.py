"""float64 model of dsp_src_polyphase_f32 (include/dspcore.h), vectorised, and
a mirror of the generic kernel's tile planner (csrc/src_poly.hip,
launch_src_rows).  Shared by tests/test_src_model.py (CPU: the model against
tests/test_stream_plan.py's per-output loop and the oracle, the planner against
a table) and tests/test_gpu_src_edges.py (GPU).

The model is the contract read literally: zero-stuff x by L, convolve with the
K taps, keep full[m M + c] for m < n_out (0 past the end of the convolution).
The convolution is computed branch by branch -- full[phi::L] = np.convolve(x,
taps[phi::L]), the same sums without the products with the stuffed zeros
(160/147 at K = 1023 would spend 159/160 of its time on them); test_src_model
pins it to np.convolve of the zero-stuffed row.  On integer-valued taps and
samples every float64 product and partial sum is an exact integer, so the
result does not depend on the summation order."""
import numpy as np

# class codes of an output (csrc/common.h, nf_code)
FINITE, PINF, NINF, NAN_ = 0, 1, 2, 3


def full_conv(x, taps, L):
    """np.convolve(x zero-stuffed by L, taps) in float64, (n_in - 1) L + K long."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    assert x.ndim == 1 and taps.ndim == 1 and x.size >= 1 and taps.size >= 1 and L >= 1
    full = np.zeros((x.size - 1) * L + taps.size)
    for phi in range(min(L, taps.size)):
        full[phi::L] = np.convolve(x, taps[phi::L])
    return full


def src_model(x, n_out, taps, L, M, c):
    """y[m] = full[m M + c], m < n_out, for one row x [n_in] or every row of
    x [B, n_in]; float64."""
    x = np.asarray(x)
    if x.ndim == 2:
        return np.stack([src_model(r, n_out, taps, L, M, c) for r in x])
    assert n_out >= 0 and M >= 1 and c >= 0
    full = full_conv(x, taps, L)
    j = np.arange(n_out, dtype=np.int64) * M + c
    y = np.zeros(n_out)
    ok = j < full.size
    y[ok] = full[j[ok]]
    return y


def abs_model(x, n_out, taps, L, M, c):
    """sum |taps . x| per output: the scale of the float32 rounding bound."""
    return src_model(np.abs(np.asarray(x, dtype=np.float64)), n_out,
                     np.abs(np.asarray(taps, dtype=np.float64)), L, M, c)


def nf_class(x, n_out, taps, L, M, c):
    """Class (FINITE / PINF / NINF / NAN_) per output of sum_t taps[phi + L t]
    xn[q - t], xn = x with its finite samples zeroed, taps as given (the
    caller's unflushed float32 taps): NaN meets any tap -> NaN; an inf takes
    the tap's sign, and a zero tap times an inf is NaN (as fmaf gives it); infs
    of both signs in one window -> NaN.  x [n_in] or [B, n_in]."""
    x = np.asarray(x)
    if x.ndim == 2:
        return np.stack([nf_class(r, n_out, taps, L, M, c) for r in x])
    taps = np.asarray(taps)
    K = taps.size
    j = np.arange(n_out, dtype=np.int64) * M + c
    nan = np.zeros(n_out, dtype=bool)
    pos = np.zeros(n_out, dtype=bool)
    neg = np.zeros(n_out, dtype=bool)
    for p in np.flatnonzero(~np.isfinite(x)):
        k = j - int(p) * L                      # the tap that meets x[p] in output m
        hit = (k >= 0) & (k < K)
        t = np.zeros(n_out)
        t[hit] = taps[k[hit]]
        v = float(x[p])
        if v != v:
            nan |= hit
        else:
            nan |= hit & (t == 0)
            pos |= hit & ((t > 0) == (v > 0)) & (t != 0)
            neg |= hit & ((t > 0) != (v > 0)) & (t != 0)
    out = np.full(n_out, FINITE, dtype=np.int8)
    out[pos] = PINF
    out[neg] = NINF
    out[nan | (pos & neg)] = NAN_
    return out


def classify(y):
    """The same codes for the values of y."""
    y = np.asarray(y)
    out = np.full(y.shape, FINITE, dtype=np.int8)
    out[np.isposinf(y)] = PINF
    out[np.isneginf(y)] = NINF
    out[np.isnan(y)] = NAN_
    return out


# --------------------------------------------------------------------------- planner mirror
# csrc/src_poly.hip, launch_src_rows: the generic kernel's dynamic LDS is the
# tap bank, ceil4(L T) floats, and the window of a tile of t outputs,
# ceil4((t - 1) M / L + T + 2 + 8) floats; the tile halves from GEN_TILE until
# both fit in LDS_MAX bytes, and a bank that does not fit beside a GEN_TILE_MIN
# window is refused (DSP_ENOTSUP).
GEN_NT = 256                    # kGenNT
GEN_TILE = 4096                 # kGenTile
GEN_TILE_MIN = 64
LDS_MAX = 160 * 1024 - 64       # kLdsMax


def _ceil4(n):
    return (n + 3) // 4 * 4


def branch_taps(K, L):
    """T = ceil(K / L), the taps of the longest polyphase branch."""
    return -(-K // L)


def gen_lds_bytes(L, M, K, tile):
    T = branch_taps(K, L)
    return 4 * (_ceil4(L * T) + _ceil4((tile - 1) * M // L + T + 10))


def gen_tile(L, M, K):
    """The generic kernel's tile for (L, M, K); None where the call is refused."""
    tile = GEN_TILE
    while tile > GEN_TILE_MIN and gen_lds_bytes(L, M, K, tile) > LDS_MAX:
        tile >>= 1
    return tile if gen_lds_bytes(L, M, K, tile) <= LDS_MAX else None
