"""Pure-Python restatement of gps_l1_ca_telemetry_decoder_gs (gps_l1_ca_telemetry_decoder_gs.cc) up to the time of week:
preamble seeding, the 300-symbol history, check_tlm_separation (:448-460), the two-state frame synchronisation (:463-554),
decode_subframe (:261-433) with the parity check of :191-214, the subframe ID and TOW of the HOW
(gps_navigation_message.cc:98-273) and the TOW stamping of general_work (:564-707).  One LnavDecoder is one block object.

Per symbol, in the block's order: seed the 8 preamble values into an empty history (negated under the incoming symbol's
180° flag; the counter grows by 8), push the symbol, counter++, d_flag_preamble = false, check_tlm_separation, the switch
on d_stat, then the stamping.  The block only ever asks `x < 0` and `x > 0` of a symbol, so the history holds one of three
codes per entry: 0 (zero, -0, NaN), 1 (> 0), 2 (< 0).

Kept as the block has them: state 0 clears d_prev_GPS_frame_4bytes before a decode and state 1 does not; a state-0 hit
changes the 180° flag whether the decode succeeds or not; state 0 ends every symbol with d_flag_TOW_set = false; a
subframe of good parity whose ID is not 1..5 is a failure and leaves the TOW alone; a valid subframe with TOW 0 stamps
nothing and does not even add the 20 ms; loss of sync (more than 2 consecutive failures) zeroes both TOW members and the
error counter; reset() clears the history and d_stat but not the error counter, d_flag_frame_sync, the 180° flag or the
previous word; set_satellite() is a new navigation object (TOW 0) and nothing else.

The transmitter (build_subframe / build_stream) is independent of the checker: its parities are the six equations of
IS-GPS-200 Table 20-XIV written as the ICD's XOR lists, the checker is the block's rotate-and-mask form.
"""
from __future__ import annotations

from collections import deque

import numpy as np

PREAMBLE = "10001011"
SUBFRAME_BITS = 300
CRC_ERROR_LIMIT = 2                 # "> 2" at :539
MAX_WITHOUT_VALID = 20 * SUBFRAME_BITS  # :122
BIT_PERIOD_MS = 20

# gnsship_lnav_subframe.flags
F_OK, F_PARITY_OK, F_PLL_180, F_STATE1, F_FRAME_SYNC, F_SYNC_LOST = 1, 2, 4, 8, 16, 32
# sflags
S_OUTPUT, S_PLL_180, S_SUBFRAME = 1, 2, 4

_PRE_NEG = tuple(ch == "0" for ch in PREAMBLE)  # entry i negative <=> preamble[i] is -1: corr = +8
_PRE_POS = tuple(ch == "1" for ch in PREAMBLE)  # the inverse: corr = -8


def subframes_per_run(max_rounds: int) -> int:
    """The most records one run of max_rounds symbols can emit.  Every record sets preamble_index, so the next state-1
    decode is 300 symbols later: consecutive records are at least 300 symbols apart, except a state-0 success, which may
    follow a loss of sync by one symbol.  A loss needs three consecutive state-1 failures after the last success (the
    first loss of a run may find the error counter already at 2), so losses are at least 901 symbols apart: with L
    losses, n >= 1 + 300 (R - 1 - L) + L and L <= (n - 1) / 901 + 1, which gives R <= n / 300 + n / 900 + 2."""
    return max_rounds // 300 + max_rounds // 900 + 2


def _rotl(x: int, n: int) -> int:
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def parity_check(word: int) -> bool:
    """gps_word_parityCheck (:191-214): bits 29..6 the data bits d1..d24 (already un-inverted), 5..0 the received parity,
    30 = D30*, 31 = D29*."""
    d1 = word & 0xFBFFBF00
    d2 = _rotl(word, 1) & 0x07FFBF01
    d3 = _rotl(word, 2) & 0xFC0F8100
    d4 = _rotl(word, 3) & 0xF81FFE02
    d5 = _rotl(word, 4) & 0xFC00000E
    d6 = _rotl(word, 5) & 0x07F00001
    d7 = _rotl(word, 6) & 0x00003000
    t = d1 ^ d2 ^ d3 ^ d4 ^ d5 ^ d6 ^ d7
    parity = (t ^ _rotl(t, 6) ^ _rotl(t, 12) ^ _rotl(t, 18) ^ _rotl(t, 24)) & 0x3F
    return parity == (word & 0x3F)


def _code(x) -> int:
    x = np.float32(x)
    return 1 if x > 0 else (2 if x < 0 else 0)


class LnavDecoder:
    """One gps_l1_ca_telemetry_decoder_gs object."""

    def __init__(self):
        self.hist = deque(maxlen=SUBFRAME_BITS)  # codes, oldest first
        self.symbol_counter = 0
        self.preamble_index = 0
        self.last_valid_preamble = 0
        self.subframes_tried = 0
        self.prev_word = 0
        self.tow_at_preamble_ms = 0
        self.tow_at_current_symbol_ms = 0
        self.nav_tow_s = 0
        self.stat = 0
        self.crc_error_counter = 0
        self.pll_180 = False
        self.frame_sync = False
        self.tow_set = False
        self.sent_tlm_failed = False

    # ---- channel control ----
    def reset(self):
        self.last_valid_preamble = self.symbol_counter
        self.sent_tlm_failed = False
        self.tow_set = False
        self.hist.clear()
        self.stat = 0

    def set_satellite(self):
        self.nav_tow_s = 0

    def state(self) -> dict:
        return dict(symbol_counter=self.symbol_counter, preamble_index=self.preamble_index, last_valid_preamble=self.last_valid_preamble,
                    subframes_tried=self.subframes_tried, prev_word=self.prev_word, tow_at_preamble_ms=self.tow_at_preamble_ms,
                    tow_at_current_symbol_ms=self.tow_at_current_symbol_ms, nav_tow_s=self.nav_tow_s, stat=self.stat,
                    crc_error_counter=self.crc_error_counter, history_size=len(self.hist), pll_180=int(self.pll_180),
                    frame_sync=int(self.frame_sync), tow_set=int(self.tow_set), sent_tlm_failed=int(self.sent_tlm_failed))

    def _decode(self, invert: bool):
        """decode_subframe: (returned true, words, parity_fail_mask, subframe id bits)."""
        self.subframes_tried += 1
        one = 2 if invert else 1
        words, fail, w, k = [], 0, 0, 0
        for code in self.hist:
            w = (w << 1) | (1 if code == one else 0)
            k += 1
            if k == 30:
                k = 0
                if self.prev_word & 1:
                    w |= 0x40000000
                if self.prev_word & 2:
                    w |= 0x80000000
                if w & 0x40000000:
                    w ^= 0x3FFFFFC0
                if not parity_check(w):
                    fail |= 1 << len(words)
                words.append(w)
                self.prev_word = w
                w = 0
        words += [0] * (10 - len(words))
        sid = (words[1] >> 8) & 7
        if fail == 0 and 1 <= sid <= 5:
            self.nav_tow_s = 6 * ((words[1] >> 13) & 0x1FFFF)
            return True, words, fail, sid
        return False, words, fail, sid

    def push(self, symbol, sample_counter: int = 0, flag180: bool = False):
        """One general_work call.  Returns (subframe record or None, fault raised by this symbol, tow_ms, sflags)."""
        if not self.hist:
            neg = _PRE_POS if flag180 else _PRE_NEG
            self.hist.extend(2 if n else 1 for n in neg)
            self.symbol_counter += len(PREAMBLE)
        self.hist.append(_code(symbol))
        self.symbol_counter += 1
        flag_preamble = False
        fault = False
        if not self.sent_tlm_failed and self.symbol_counter - self.last_valid_preamble > MAX_WITHOUT_VALID:
            self.sent_tlm_failed = True
            fault = True
        rec = None
        decoded = None
        lost = False
        was1 = self.stat == 1
        if self.stat == 0:
            if len(self.hist) >= SUBFRAME_BITS:
                w = tuple(self.hist[i] == 2 for i in range(len(PREAMBLE)))
                if w == _PRE_NEG or w == _PRE_POS:
                    self.preamble_index = self.symbol_counter
                    self.pll_180 = w == _PRE_POS
                    self.prev_word = 0
                    decoded = self._decode(self.pll_180)
                    if decoded[0]:
                        self.crc_error_counter = 0
                        flag_preamble = True
                        self.last_valid_preamble = self.symbol_counter
                        self.frame_sync = True
                        self.stat = 1
            self.tow_set = False
        elif self.symbol_counter >= self.preamble_index + SUBFRAME_BITS:
            self.preamble_index = self.symbol_counter
            decoded = self._decode(self.pll_180)
            if decoded[0]:
                self.crc_error_counter = 0
                flag_preamble = True
                self.last_valid_preamble = self.symbol_counter
                self.frame_sync = True
            else:
                self.crc_error_counter += 1
                if self.crc_error_counter > CRC_ERROR_LIMIT:
                    self.frame_sync = False
                    self.stat = 0
                    self.tow_at_current_symbol_ms = 0
                    self.tow_at_preamble_ms = 0
                    self.crc_error_counter = 0
                    self.tow_set = False
                    lost = True
        if flag_preamble:
            if self.nav_tow_s != 0:
                self.tow_at_current_symbol_ms = self.tow_at_preamble_ms = self.nav_tow_s * 1000
                self.tow_set = True
        elif self.tow_set:
            self.tow_at_current_symbol_ms = (self.tow_at_current_symbol_ms + BIT_PERIOD_MS) & 0xFFFFFFFF
        if decoded is not None and (decoded[0] or was1):
            ok, words, fail, sid = decoded
            flags = (F_OK if ok else 0) | (F_PARITY_OK if fail == 0 else 0) | (F_PLL_180 if self.pll_180 else 0) | \
                (F_STATE1 if was1 else 0) | (F_FRAME_SYNC if self.frame_sync else 0) | (F_SYNC_LOST if lost else 0)
            rec = dict(symbol_counter=self.symbol_counter, sample_counter=int(sample_counter), words=list(words), subframe_id=sid,
                       tow_s=self.nav_tow_s, crc_error_counter=self.crc_error_counter, parity_fail_mask=fail, flags=flags)
        sflags = (S_OUTPUT if self.tow_set else 0) | (S_PLL_180 if self.pll_180 else 0) | (S_SUBFRAME if flag_preamble else 0)
        return rec, fault, self.tow_at_current_symbol_ms, sflags

    def run(self, symbols, sample_counters=None, flags180=None):
        """Push symbols in order.  Returns (subframe records, fault raised in this run, tow_ms uint32[n], sflags uint8[n])."""
        symbols = np.asarray(symbols, np.float32)
        recs, fault = [], False
        tow, sf = np.zeros(len(symbols), np.uint32), np.zeros(len(symbols), np.uint8)
        for k, s in enumerate(symbols):
            r, f, tow[k], sf[k] = self.push(s, 0 if sample_counters is None else sample_counters[k], False if flags180 is None else bool(flags180[k]))
            fault |= f
            if r is not None:
                recs.append(r)
        assert len(recs) <= subframes_per_run(len(symbols)), (len(recs), len(symbols))
        return recs, fault, tow, sf


# ---- the transmitter: IS-GPS-200, 20.3.5.2 and Table 20-XIV -------------------------------------------------------------

# source bits d1..d24 entering D25..D30 (1-based, as the ICD lists them), and which of D29*, D30* leads each equation
_ICD = [
    (29, (1, 2, 3, 5, 6, 10, 11, 12, 13, 14, 17, 18, 20, 23)),
    (30, (2, 3, 4, 6, 7, 11, 12, 13, 14, 15, 18, 19, 21, 24)),
    (29, (1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22)),
    (30, (2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23)),
    (30, (1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24)),
    (29, (3, 5, 6, 8, 9, 10, 11, 13, 15, 19, 22, 23, 24)),
]


def icd_parity(d, d29s: int, d30s: int):
    """D25..D30 of the source bits d[0..23] = d1..d24."""
    out = []
    for lead, taps in _ICD:
        p = d29s if lead == 29 else d30s
        for t in taps:
            p ^= int(d[t - 1])
        out.append(p)
    return out


def encode_word(d, d29s: int, d30s: int, solve: bool = False):
    """24 source bits → the 30 transmitted bits D1..D30 (D1..D24 = d XOR D30*).  With solve, d23 and d24 are chosen so
    that D29 = D30 = 0 (the two non-information bits of words 2 and 10)."""
    d = [int(x) for x in d]
    if solve:
        d[22] = d[23] = 0
        p = icd_parity(d, d29s, d30s)
        d[23] = p[4]                    # of D29 and D30, d24 enters both
        d[22] = p[5] ^ d[23]            # and d23 only D30
        assert icd_parity(d, d29s, d30s)[4:] == [0, 0]
    return [b ^ d30s for b in d] + icd_parity(d, d29s, d30s)


def stored_word(bits30, d29s: int, d30s: int) -> int:
    """What decode_subframe stores for the transmitted bits D1..D30 after a word ending in D29*, D30*."""
    w = 0
    for b in bits30:
        w = (w << 1) | int(b)
    w |= (d30s << 30) | (d29s << 31)
    if d30s:
        w ^= 0x3FFFFFC0
    return w


def build_subframe(subframe_id: int, tow: int, payload, d29s: int = 0, d30s: int = 0):
    """One LNAV subframe.  tow: the 17-bit TOW count of the HOW (the block's TOW is 6 × tow seconds); payload: 208 bits —
    16 for the TLM word after the preamble, 2 for the HOW's alert and anti-spoof flags, 24 for each of words 3..9 and 22
    for word 10.  Returns (bits uint8[300] as transmitted, the ten words as the block stores them)."""
    payload = [int(b) for b in payload]
    assert len(payload) == 208 and 0 <= tow < (1 << 17) and 0 <= subframe_id < 8
    src = [[int(ch) for ch in PREAMBLE] + payload[:16]]
    how = [(tow >> (16 - k)) & 1 for k in range(17)] + payload[16:18] + [(subframe_id >> (2 - k)) & 1 for k in range(3)] + [0, 0]
    src.append(how)
    for i in range(7):
        src.append(payload[18 + 24 * i:18 + 24 * (i + 1)])
    src.append(payload[186:208] + [0, 0])
    bits, words = [], []
    for i, d in enumerate(src):
        w = encode_word(d, d29s, d30s, solve=i in (1, 9))
        words.append(stored_word(w, d29s, d30s))
        bits += w
        d29s, d30s = w[28], w[29]
    return np.array(bits, np.uint8), words


def symbols_of(bits) -> np.ndarray:
    """A one is +1, a zero -1."""
    return np.where(np.asarray(bits) != 0, 1.0, -1.0).astype(np.float32)


def build_stream(subframes, n_symbols: int, lead: int, seed: int = 0) -> np.ndarray:
    """`lead` random ±1 symbols, then the subframes (bit arrays) cycling, cut to n_symbols."""
    rng = np.random.default_rng(seed)
    head = np.where(rng.integers(0, 2, lead) > 0, 1.0, -1.0).astype(np.float32)
    body = np.concatenate([symbols_of(b) for b in subframes])
    reps = max(1, -(-(n_symbols - lead) // len(body)))
    return np.concatenate([head] + [body] * reps)[:n_symbols].astype(np.float32)


def five_subframes(seed: int, tow0: int = 1000, ids=(1, 2, 3, 4, 5)):
    """Consecutive subframes (TOW count rising by one) with random payloads: (list of bit arrays, list of stored words)."""
    rng = np.random.default_rng(seed)
    out_bits, out_words = [], []
    for k, sid in enumerate(ids):
        b, w = build_subframe(sid, tow0 + k, rng.integers(0, 2, 208))
        out_bits.append(b)
        out_words.append(w)
    return out_bits, out_words
