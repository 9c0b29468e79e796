"""numpy restatement of the K = 7, rate-1/2 Viterbi decoder of the Galileo telemetry block, in the two modes of
gnsship_vit (include/gnsship.h), and of the two steps the block runs ahead of it.

REFERENCE mode restates Viterbi_Decoder::decode (telemetry_decoder/libs/viterbi_decoder.cc:47-120) as written:
  * only the first symbol of each pair enters the metric (:61 copies d_nn − 1 = 1 value, d_rec_array[1] stays 0):
    Gamma = {0, 0 + 0, 0 + r0, (0 + 0) + r0}, float sums in that order (:151-166);
  * the 64 path metrics carry over from call to call; d_prev_section[0] = 0 (:56) is the only re-initialisation,
    the rest is −1e7 only in the first call of a new object;
  * d_next_section starts at −1e7 (:102), the states are visited in ascending order with a strict `>` (:70-93): for
    next state s' the candidates come from p0 = (s' & 31) << 1, then p1 = p0 | 1, both with information bit s' >> 5
    and branch output (parity(w & g[0]) << 1) | parity(w & g[1]), w = (bit << 6) ^ p (:183-204); p0 wins a tie and an
    entry that neither candidate lifts above −1e7 is not stored;
  * the section maximum is subtracted (:96-103); the traceback starts at state 0, skips the 6 tail steps and emits
    LL bits (:107-119).
tests/test_viterbi_model.py pins this against the compiled reference (tests/golden/viterbi_ref.npz): bits and the
64 carried metrics, bit for bit.

An entry (t, s') nothing stored in this call reads here as predecessor 0, bit 0, which is what a new object holds;
the reference would read what an earlier call left there.  That case is not restated: decode() reports whether the
traceback visited such an entry, and the tests require that it did not wherever the reference is the yardstick.

FULL mode: both symbols in the metric (Gamma = {0, 0 + r1, 0 + r0, (0 + r1) + r0}) and every frame starts from
state 0 alone (metric 0, the other 63 at −1e7); nothing is carried.

deinterleave() and g2_flip() restate galileo_telemetry_decoder_gs.cc:342-351 and :362-368.  That block cannot be
compiled without GNU Radio, so these two are compared with nothing but themselves and the kernel.
"""
from __future__ import annotations

import numpy as np

REFERENCE, FULL = 0, 1
MAXLOG = np.float32(1e7)
G_GALILEO = (121, 91)
# (interleaver rows, interleaver columns, LL) of the three Galileo page types
INAV, FNAV, CNAV = (8, 30, 114), (8, 61, 238), (8, 123, 486)


def _parity(x):
    x = np.asarray(x)
    p = np.zeros_like(x)
    for k in range(7):
        p ^= (x >> k) & 1
    return p


def trellis(g=G_GALILEO):
    """p0[64], out0[64], out1[64]: per next state, its first predecessor and the branch outputs from p0 and p0 | 1."""
    s = np.arange(64)
    p0 = (s & 31) << 1
    bit = s >> 5
    outs = []
    for p in (p0, p0 | 1):
        w = (bit << 6) ^ p
        outs.append((_parity(w & g[0]) << 1) | _parity(w & g[1]))
    return p0, outs[0], outs[1]


def encode(bits, g=G_GALILEO):
    """The encoder the decoder's trellis belongs to: LL bits and 6 zero tail bits → 2·(LL + 6) symbols, +1 for a
    one and −1 for a zero (the sign the metric rewards), g[0]'s symbol first."""
    state = 0
    out = []
    for b in list(np.asarray(bits, np.int64)) + [0] * 6:
        w = (int(b) << 6) ^ state
        out.append(2 * (bin(w & g[0]).count("1") & 1) - 1)
        out.append(2 * (bin(w & g[1]).count("1") & 1) - 1)
        state = w >> 1
    return np.array(out, np.float32)


def deinterleave(rows, cols, x):
    """galileo_telemetry_decoder_gs::deinterleaver (:342-351): out[c·rows + r] = in[r·cols + c]."""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] == rows * cols
    return np.ascontiguousarray(np.swapaxes(x.reshape(x.shape[:-1] + (rows, cols)), -1, -2)).reshape(x.shape)


def g2_flip(x):
    """The NOT gate of G2 (:362-368): every second symbol negated."""
    y = np.array(x, np.float32, copy=True)
    y[..., 1::2] = -y[..., 1::2]
    return y


def prepare(x, rows=0, cols=0, invert_g2=False, negate=False):
    """What the block hands to decode(): the 180° case (:1026-1029), the de-interleaver, the G2 flip."""
    y = np.asarray(x, np.float32)
    if negate:
        y = -y
    if rows:
        y = deinterleave(rows, cols, y)
    if invert_g2:
        y = g2_flip(y)
    return y


def new_section(n=None):
    """d_prev_section of a new object (all 64 at −1e7), or n of them."""
    return np.full(64 if n is None else (n, 64), -MAXLOG, np.float32)


def decode_batch(sym, section, mode=REFERENCE, g=G_GALILEO):
    """sym float32[n, 2·(LL + 6)] (de-interleaved, flipped), section float32[n, 64] (updated in place in REFERENCE
    mode, ignored in FULL mode).  Returns (bits uint8[n, LL], unstored_visited bool[n])."""
    sym = np.asarray(sym, np.float32)
    n, frame = sym.shape
    steps = frame // 2
    LL = steps - 6
    assert frame % 2 == 0 and LL >= 1
    p0, out0, out1 = trellis(g)
    p1 = p0 | 1
    zero = np.float32(0.0)
    if mode == REFERENCE:
        prev = section
        prev[:, 0] = zero
    else:
        prev = new_section(n)
        prev[:, 0] = zero
    decision = np.zeros((steps, n, 64), bool)  # the stored predecessor is p1
    stored = np.zeros((steps, n, 64), bool)
    gamma = np.zeros((n, 4), np.float32)
    for t in range(steps):
        r0 = sym[:, 2 * t]
        rec1 = sym[:, 2 * t + 1] if mode == FULL else np.zeros(n, np.float32)
        gamma[:, 1] = zero + rec1
        gamma[:, 2] = zero + r0
        gamma[:, 3] = (zero + rec1) + r0
        m0 = prev[:, p0] + gamma[:, out0]
        m1 = prev[:, p1] + gamma[:, out1]
        cur = np.full((n, 64), -MAXLOG, np.float32)
        s0 = m0 > cur
        cur = np.where(s0, m0, cur)
        s1 = m1 > cur
        cur = np.where(s1, m1, cur)
        decision[t] = s1
        stored[t] = s0 | s1
        prev[:] = cur - cur.max(axis=1, keepdims=True)
    state = np.zeros(n, np.int64)
    rows = np.arange(n)
    visited = np.zeros(n, bool)
    bits = np.zeros((n, LL), np.uint8)
    for t in range(steps - 1, -1, -1):
        st = stored[t, rows, state]
        visited |= ~st
        if t < LL:
            bits[:, t] = np.where(st, state >> 5, 0)
        state = np.where(st, ((state & 31) << 1) | decision[t, rows, state], 0)
    return bits, visited


class ViterbiDecoder:
    """One Viterbi_Decoder object: decode() after decode() on the carried section."""

    def __init__(self, LL, g=G_GALILEO, mode=REFERENCE):
        self.LL, self.g, self.mode = LL, tuple(g), mode
        self.section = new_section()

    def decode(self, sym):
        """sym float32[2·(LL + 6)] → (bits uint8[LL], unstored_visited)."""
        sym = np.asarray(sym, np.float32)
        assert sym.shape == (2 * (self.LL + 6),)
        sec = self.section[None, :]
        bits, vis = decode_batch(sym[None, :], sec, self.mode, self.g)
        return bits[0], bool(vis[0])
