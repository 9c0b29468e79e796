"""numpy restatement of the frame handling of galileo_telemetry_decoder_gs::general_work (galileo_telemetry_decoder_gs.cc
:872-1094) for I/NAV, F/NAV and C/NAV: symbol history, preamble correlation, the three-state frame-sync machine with its
180° flag, page-part extraction, de-interleave / G2 / Viterbi (tests/viterbi_model.py), even + odd assembly, CRC-24Q, the
CRC-error counter, loss of sync and check_tlm_separation (:856-869).  One TlmDecoder object is one block object.

What is restated, per symbol and in this order: push_back into a history of capacity required + 1 (:884), the symbol
counter (:886), check_tlm_separation (:935), then the switch on d_stat (:939-1094).  In states 0 and 1 the correlation
runs only on a full history, over its P oldest entries, an entry counting as negative only when `< 0.0`.  State 2 decodes
when counter == preamble_index + period.  crc_ok is the message object's flag_CRC_test, which for I/NAV is written only
when an odd part joins a stored even part (galileo_inav_message.cc:140-197) and is cleared by nothing: after an even part
it is the previous odd part's verdict.  C/NAV decodes as with a non-zero sampling rate in the symbol (:1040).

reset() and set_satellite() restate :792-820 and :771-789.

The page builder (build_part / build_stream) is the transmitter those steps undo: CRC, six tail bits, the convolutional
code (viterbi_model.encode), the NOT gate of G2, the block interleaver and the preamble.
"""
from __future__ import annotations

import numpy as np

import viterbi_model as V

INAV, FNAV, CNAV = 1, 2, 3
CRC_ERROR_LIMIT = 6
CRC24Q_POLY = 0x1864CFB

# page flags of gnsship_tlm_page
F_CRC_OK, F_CRC_EVALUATED, F_PLL_180, F_ODD, F_FRAME_SYNC, F_SYNC_LOST = 1, 2, 4, 8, 16, 32


class Geometry:
    def __init__(self, frame_type, preamble, period, required, rows, cols, LL, max_without_valid, crc_bits):
        self.frame_type = frame_type
        self.preamble = np.array([1 if ch == "1" else -1 for ch in preamble], np.int32)
        self.P = len(preamble)
        self.period, self.required = period, required
        self.frame = period - self.P
        self.rows, self.cols, self.LL = rows, cols, LL
        self.max_without_valid = max_without_valid
        self.crc_bits = crc_bits  # bits the CRC runs over; the 24 checksum bits follow them
        assert rows * cols == self.frame == 2 * (LL + 6)


GEOMETRY = {
    INAV: Geometry(INAV, "0101100000", 250, 510, 8, 30, 114, 15000, 196),
    FNAV: Geometry(FNAV, "101101110000", 500, 512, 8, 61, 238, 2500, 214),
    CNAV: Geometry(CNAV, "1011011101110000", 1000, 1016, 8, 123, 486, 60000, 462),
}


def crc24q_bits(bits) -> int:
    """The MSB-first CRC-24Q (polynomial 0x1864CFB, zero initial value, no reflection, no final XOR) of a bit string."""
    reg = 0
    for b in np.asarray(bits, np.int64):
        reg ^= int(b) << 23
        reg <<= 1
        if reg & 0x1000000:
            reg ^= CRC24Q_POLY
    return reg & 0xFFFFFF


def crc24q_bytes(data: bytes) -> int:
    return crc24q_bits(np.unpackbits(np.frombuffer(data, np.uint8)))


def crc24q_table(n: int) -> np.ndarray:
    """table[i] = x^(n − 1 − i + 24) mod g: the remainder a one at bit i of an n-bit string contributes."""
    t = np.zeros(n, np.uint32)
    reg = 1  # x^0
    rem = []
    for _ in range(n + 24):
        rem.append(reg)
        reg <<= 1
        if reg & 0x1000000:
            reg ^= CRC24Q_POLY
        reg &= 0xFFFFFF
    for i in range(n):
        t[i] = rem[n - 1 - i + 24]
    return t


def crc24q_table_xor(bits) -> int:
    bits = np.asarray(bits, np.int64)
    t = crc24q_table(len(bits))
    return int(np.bitwise_xor.reduce(t[bits != 0])) if (bits != 0).any() else 0


def bits_value(bits) -> int:
    v = 0
    for b in np.asarray(bits, np.int64):
        v = (v << 1) | int(b)
    return v


def int_bits(v: int, n: int) -> np.ndarray:
    return np.array([(v >> (n - 1 - k)) & 1 for k in range(n)], np.uint8)


class TlmDecoder:
    """One galileo_telemetry_decoder_gs object (frame handling only)."""

    def __init__(self, frame_type: int, mode=V.REFERENCE):
        self.g = GEOMETRY[frame_type]
        self.mode = mode
        self.vit = V.ViterbiDecoder(self.g.LL, V.G_GALILEO, mode)
        self.cap = self.g.required + 1
        self.hist = []       # every symbol ever pushed (float32); the history is its last `cap` entries
        self.neg = []        # hist[i] < 0.0
        self.pre_neg = [bool(p < 0) for p in self.g.preamble]
        self.pre_pos = [not x for x in self.pre_neg]
        self.symbol_counter = 0
        self.preamble_index = 0
        self.last_valid_preamble = 0
        self.stat = 0
        self.crc_error_counter = 0
        self.pll_180 = False
        self.frame_sync = False
        self.sent_tlm_failed = False
        self.even_word_arrived = 0
        self.page_even = np.zeros(114, np.uint8)
        self.flag_crc_test = False

    # ---- channel control ----
    def reset(self):
        self.frame_sync = False
        self.stat = 0
        self.last_valid_preamble = self.symbol_counter
        self.sent_tlm_failed = False

    def set_satellite(self):
        self.last_valid_preamble = self.symbol_counter
        self.sent_tlm_failed = False

    # ---- members ----
    def history(self) -> np.ndarray:
        return np.array(self.hist[-self.cap:], np.float32)

    def state(self) -> dict:
        return dict(symbol_counter=self.symbol_counter, preamble_index=self.preamble_index, last_valid_preamble=self.last_valid_preamble,
                    stat=self.stat, crc_error_counter=self.crc_error_counter, history_size=min(len(self.hist), self.cap),
                    pll_180=int(self.pll_180), frame_sync=int(self.frame_sync), even_word_arrived=int(self.even_word_arrived),
                    flag_crc_test=int(self.flag_crc_test), sent_tlm_failed=int(self.sent_tlm_failed))

    def _corr(self):
        """0 without a hit, else the sign of corr_value (|corr_value| == P)."""
        o = len(self.neg) - self.cap
        w = self.neg[o:o + self.g.P]
        if w == self.pre_neg:
            return 1
        if w == self.pre_pos:
            return -1
        return 0

    def _page(self, bits):
        """decode_*_word after the Viterbi decoder: (a CRC was evaluated, I/NAV odd part)."""
        g = self.g
        if g.frame_type == INAV:
            if bits[0] == 0:
                self.page_even = bits.copy()
                self.even_word_arrived = 1
                return False, False
            evaluated = False
            if self.even_word_arrived == 1:
                joined = np.concatenate([self.page_even, bits, np.zeros(6, np.uint8)])
                self.flag_crc_test = crc24q_bits(joined[:196]) == bits_value(joined[196:220])
                evaluated = True
            self.even_word_arrived = 0
            return evaluated, True
        n = g.crc_bits
        self.flag_crc_test = crc24q_bits(bits[:n]) == bits_value(bits[n:n + 24])
        return True, False

    def push(self, symbol, sample_counter: int = 0):
        """One general_work call.  Returns (page or None, fault raised by this symbol)."""
        g = self.g
        s = np.float32(symbol)
        self.hist.append(s)
        self.neg.append(bool(s < 0.0))
        self.symbol_counter += 1
        fault = False
        if not self.sent_tlm_failed and self.symbol_counter - self.last_valid_preamble > g.max_without_valid:
            self.sent_tlm_failed = True
            fault = True
        page = None
        full = len(self.hist) > g.required
        if self.stat == 0:
            if full and self._corr() != 0:
                self.preamble_index = self.symbol_counter
                self.stat = 1
        elif self.stat == 1:
            c = self._corr() if full else 0
            if c != 0:
                diff = self.symbol_counter - self.preamble_index
                if diff == g.period:
                    self.preamble_index = self.symbol_counter
                    self.crc_error_counter = 0
                    self.pll_180 = c < 0
                    self.stat = 2
                elif diff > g.period:
                    self.stat = 0
        elif self.symbol_counter == self.preamble_index + g.period:
            o = len(self.hist) - self.cap
            frame = np.array(self.hist[o + g.P:o + g.P + g.frame], np.float32)
            sym = V.prepare(frame, g.rows, g.cols, invert_g2=True, negate=self.pll_180)
            bits, _ = self.vit.decode(sym)
            evaluated, odd = self._page(bits)
            crc_ok = self.flag_crc_test
            self.preamble_index = self.symbol_counter
            lost = False
            if crc_ok:
                self.crc_error_counter = 0
                self.last_valid_preamble = self.symbol_counter
                self.frame_sync = True
            else:
                self.crc_error_counter += 1
                if self.crc_error_counter > CRC_ERROR_LIMIT:
                    self.frame_sync = False
                    self.stat = 0
                    lost = True
            flags = (F_CRC_OK if crc_ok else 0) | (F_CRC_EVALUATED if evaluated else 0) | (F_PLL_180 if self.pll_180 else 0) | \
                (F_ODD if odd else 0) | (F_FRAME_SYNC if self.frame_sync else 0) | (F_SYNC_LOST if lost else 0)
            page = dict(symbol_counter=self.symbol_counter, sample_counter=int(sample_counter), flags=flags,
                        crc_error_counter=self.crc_error_counter, bits=bits)
        if len(self.hist) > 4 * self.cap:  # keep the lists short; the history is their tail
            self.hist = self.hist[-self.cap:]
            self.neg = self.neg[-self.cap:]
        return page, fault

    def run(self, symbols, sample_counters=None):
        """Push symbols in order.  Returns (pages, fault raised in this run)."""
        pages, fault = [], False
        for k, s in enumerate(np.asarray(symbols, np.float32)):
            p, f = self.push(s, 0 if sample_counters is None else sample_counters[k])
            fault |= f
            if p is not None:
                pages.append(p)
        return pages, fault


# ---- the transmitter ----------------------------------------------------------------------------------------------

def interleave(rows, cols, x):
    """The inverse of viterbi_model.deinterleave: in[r·cols + c] = x[c·rows + r]."""
    x = np.asarray(x, np.float32)
    return np.ascontiguousarray(x.reshape(cols, rows).T).reshape(-1)


def build_part(frame_type: int, bits) -> np.ndarray:
    """LL bits → one transmitted page part of `period` symbols (±1, a one positive): preamble, then the interleaved,
    G2-inverted convolutional code of the bits and six tail bits."""
    g = GEOMETRY[frame_type]
    bits = np.asarray(bits, np.uint8)
    assert bits.shape == (g.LL,)
    sym = V.g2_flip(V.encode(bits))
    return np.concatenate([g.preamble.astype(np.float32), interleave(g.rows, g.cols, sym)])


def inav_page_bits(rng):
    """(even part, odd part) of one I/NAV page with a valid CRC: 114 bits each."""
    even = rng.integers(0, 2, 114).astype(np.uint8)
    odd = rng.integers(0, 2, 114).astype(np.uint8)
    even[0], odd[0] = 0, 1
    odd[82:106] = int_bits(crc24q_bits(np.concatenate([even, odd[:82]])), 24)
    return even, odd


def page_bits(frame_type: int, rng):
    """One F/NAV or C/NAV page with a valid CRC."""
    g = GEOMETRY[frame_type]
    bits = rng.integers(0, 2, g.LL).astype(np.uint8)
    bits[g.crc_bits:] = int_bits(crc24q_bits(bits[:g.crc_bits]), 24)
    return bits


def four_parts(frame_type: int, seed: int):
    """Four page parts (I/NAV: even, odd, even, odd of two pages) with valid CRCs: a list of LL-bit arrays."""
    rng = np.random.default_rng(seed)
    if frame_type == INAV:
        a, b = inav_page_bits(rng), inav_page_bits(rng)
        return [a[0], a[1], b[0], b[1]]
    return [page_bits(frame_type, rng) for _ in range(4)]


def lead_in(frame_type: int, n: int, seed: int) -> np.ndarray:
    """n random ±1 symbols in which, followed by a preamble, no window matches the preamble or its inverse before the
    preamble itself (a false hit ahead of the first page would move the whole synchronisation)."""
    g = GEOMETRY[frame_type]
    rng = np.random.default_rng(seed)
    x = np.where(rng.integers(0, 2, n) > 0, 1.0, -1.0).astype(np.float32)
    full = np.concatenate([x, g.preamble.astype(np.float32)])
    pre = g.preamble.astype(np.float32)
    changed = True
    while changed:
        changed = False
        for k in range(n):
            w = full[k:k + g.P]
            if (w == pre).all() or (w == -pre).all():
                full[k] = -full[k]
                changed = True
    return full[:n].copy()


def build_stream(frame_type: int, parts, n_symbols: int, lead: int, seed: int = 0) -> np.ndarray:
    """lead-in, then the parts cycling, cut to n_symbols."""
    body = np.concatenate([build_part(frame_type, b) for b in parts])
    reps = max(1, -(-(n_symbols - lead) // len(body)))
    return np.concatenate([lead_in(frame_type, lead, seed)] + [body] * reps)[:n_symbols].astype(np.float32)
