"""The host model of the live EQ (include/dspcore_eqlive.h), for the tests: a
channel's stream through scipy.signal.lfilter band by band, every band's `zi`
carried from block to block while the gains change.  Built on the oracle's own
designer (oracle/dsp_ref_cpu.py), not on dspcore.design."""
import numpy as np
import scipy.signal

from oracle import dsp_ref_cpu as orc


def slot_centres(fs, keys):
    """fc per slot: the reference's table, 1000 Hz for an unknown name, the
    clamp to 0.45 fs (dsp_core.py:235-246)."""
    centres = dict(orc.BANDS)
    ceiling = fs / 2.0 * 0.90
    out = []
    for name in keys:
        fc = centres.get(name, 1000)
        out.append(ceiling if fc >= ceiling else fc)
    return out


def slot_coefficients(fs, gains):
    """[(b, a)] per slot for one block's gains: the band's design when |g| > 0.1
    and fc > 10, the same design at g = 0.0 otherwise."""
    out = []
    for fc, g in zip(slot_centres(fs, gains.keys()), gains.values()):
        out.append(orc.peaking(fc, fs, g if (abs(g) > 0.1 and fc > 10) else 0.0))
    return out


def clips(gains):
    return not all(abs(g) < 0.1 for g in gains.values())


class ChannelModel:
    """One channel: state [slots][2] = scipy's zi of every band."""

    def __init__(self, slots, zi=None):
        self.s = (np.zeros((slots, 2)) if zi is None
                  else np.array(zi, dtype=np.float64).reshape(slots, 2))

    def block(self, fs, gains, x):
        """(z float32, v float64 after the clip) for one block with its gains."""
        v = np.asarray(x).astype(np.float64)
        if v.size:
            for k, (b, a) in enumerate(slot_coefficients(fs, gains)):
                v, self.s[k] = scipy.signal.lfilter(b, a, v, zi=self.s[k])
        if clips(gains):
            v = np.clip(v, -1.0, 1.0)
        return v.astype(np.float32), v

    @property
    def zi(self):
        """(s1_0, s2_0, s1_1, ...), the layout of the device state."""
        return self.s.reshape(-1).copy()


def run(fs, histories, x, lengths, zi=None):
    """B channels through the model.  histories[b][i]: row b's gains in block
    i; x float32 [B, sum(lengths)].  Returns (z float32 [B, n], zi float64
    [B, 2 * slots]) after the last block."""
    B = len(histories)
    slots = len(histories[0][0])
    z = np.empty(x.shape, dtype=np.float32)
    states = np.empty((B, 2 * slots))
    for b in range(B):
        ch = ChannelModel(slots, None if zi is None else zi[b])
        at = 0
        for i, n in enumerate(lengths):
            z[b, at:at + n], _ = ch.block(fs, histories[b][i], x[b, at:at + n])
            at += n
        states[b] = ch.zi
    return z, states
