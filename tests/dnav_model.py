"""The yardstick for the device BeiDou D1/D2 telemetry (gnsship_dnav_*): beidou_b1i_telemetry_decoder_gs and
beidou_b3i_telemetry_decoder_gs restated symbol by symbol in their own order and integer types, with the ID / Pnum / SOW /
flag logic of Beidou_Dnav_Navigation_Message::d1_subframe_decoder and d2_subframe_decoder, and a transmitter built from
the ICD's BCH(15,11,1) encoder and interleaver.  Restated, not repaired: see include/gnsship.h for the list of properties.

A symbol is a Python float (from a float32): `x < 0` and `x > 0` are asked of it as the block asks them, so +0, -0 and NaN
behave as there."""
from __future__ import annotations

from collections import deque

import numpy as np

B1I, B3I = 0, 1
PREAMBLE = [1 if ch == "1" else -1 for ch in "11100010010"]  # BEIDOU_DNAV_PREAMBLE as d_preamble_samples
N_PRE, PERIOD, REQUIRED = 11, 300, 311
LEAP = 14  # BEIDOU_DNAV_BDT2GPST_LEAP_SEC_OFFSET
ERRIND = [14, 13, 10, 12, 6, 9, 4, 11, 0, 5, 7, 8, 1, 3, 2]

# record flags (GNSSHIP_DNAV_*), sflags (GNSSHIP_DNAV_S_*)
F_INVERTED, F_STATE1, F_NEW_SOW, F_D2_DECODER, F_D2_TIMING, F_TOW_ZEROED = 1, 2, 4, 8, 16, 32
S_VALID_WORD, S_SUBFRAME, S_INVERTED = 1, 2, 4


def subframes_per_run(max_rounds: int) -> int:
    return max_rounds // 300 + 1


# ------------------------------------------------------------------ the blocks' decoder -----------------------------
def decode_bch15_11_01(bits):
    """decode_bch15_11_01 (:164-197) on fifteen +1 / -1 integers."""
    dec = list(bits)
    reg = [-1, -1, -1, -1]
    for i in range(15):
        bit = reg[3]
        reg[3] = reg[2]
        reg[2] = reg[1]
        reg[1] = reg[0]
        reg[0] = bits[i] * bit
        reg[1] *= bit
    reg = [(r + 1) // 2 for r in reg]
    err = reg[0] + reg[1] * 2 + reg[2] * 4 + reg[3] * 8
    if 0 < err < 16:
        dec[ERRIND[err - 1]] *= -1
    return dec, err


def decode_word(word_counter, enc):
    """decode_word (:200-241) on thirty floats: thirty +1 / -1 integers, and the two rows' syndromes."""
    if word_counter == 1:
        return [1 if x > 0 else -1 for x in enc], (0, 0)
    rows = [[1 if enc[c * 2 + r] > 0 else -1 for c in range(15)] for r in range(2)]
    (first, e1), (second, e2) = decode_bch15_11_01(rows[0]), decode_bch15_11_01(rows[1])
    return first[:11] + second[:11] + first[11:] + second[11:], (e1, e2)


def read_unsigned(bits, fields):
    """read_navigation_unsigned: bit N of the ICD (1-based, N = 1 first) is bits[N - 1]."""
    v = 0
    for first, n in fields:
        for j in range(n):
            v = (v << 1) | bits[first - 1 + j]
    return v


class NavMessage:
    """What the blocks use of Beidou_Dnav_Navigation_Message."""

    def __init__(self):
        self.sow = 0            # d_SOW, a double in the source; every value it takes is an integer below 2^20
        self.new_sow = False    # flag_new_SOW_available
        self.crc = False        # flag_crc_test

    def d1_subframe_decoder(self, bits):
        fra_id = read_unsigned(bits, [(16, 3)])
        self.crc = True  # "Perform crc computation (tbd)"
        if 1 <= fra_id <= 5:
            self.sow = read_unsigned(bits, [(19, 8), (31, 12)])
            self.new_sow = True
        return fra_id

    def d2_subframe_decoder(self, bits):
        fra_id = read_unsigned(bits, [(16, 3)])
        page = read_unsigned(bits, [(43, 4)])
        self.crc = True
        if fra_id == 1 and 1 <= page <= 10:
            self.sow = read_unsigned(bits, [(19, 8), (31, 12)])
            self.new_sow = True
        return fra_id


def is_d2_timing(prn):
    return 0 < prn < 6 or prn > 58


def is_d2_decoder(signal, prn):
    return 0 < prn < 6 or (signal == B1I and prn > 58)


class Decoder:
    """One block object.  `signal` picks the block (B1I / B3I); the satellite is given as the constructor and
    set_satellite() are given it."""

    def __init__(self, signal, prn=0, channel=0):
        self.signal, self.channel = signal, channel
        self.history = deque(maxlen=REQUIRED)
        self.symbol_counter = 0
        self.preamble_index = 0
        self.last_valid_preamble = 0
        self.tow_at_preamble_ms = 0
        self.tow_at_current_symbol_ms = 0
        self.stat = 0
        self.crc_error_counter = 0
        self.sow_set = self.frame_sync = self.valid_word = self.sent_tlm_failed = False
        self.nav = NavMessage()
        self.prn = 0
        self.symbol_duration_ms = 20
        self.set_satellite(prn)

    def set_satellite(self, prn):
        self.prn = prn
        self.symbol_duration_ms = 2 if is_d2_timing(prn) else 20

    def reset(self):
        self.last_valid_preamble = self.symbol_counter
        self.tow_at_current_symbol_ms = 0
        self.sent_tlm_failed = False
        self.valid_word = False

    def state(self):
        return dict(symbol_counter=self.symbol_counter, preamble_index=self.preamble_index, last_valid_preamble=self.last_valid_preamble,
                    tow_at_preamble_ms=self.tow_at_preamble_ms, tow_at_current_symbol_ms=self.tow_at_current_symbol_ms, sow=self.nav.sow,
                    symbol_duration_ms=self.symbol_duration_ms, stat=self.stat, crc_error_counter=self.crc_error_counter,
                    history_size=len(self.history), prn=self.prn, sow_set=int(self.sow_set), frame_sync=int(self.frame_sync),
                    valid_word=int(self.valid_word), new_sow_available=int(self.nav.new_sow), sent_tlm_failed=int(self.sent_tlm_failed),
                    d2_decoder=int(is_d2_decoder(self.signal, self.prn)), d2_timing=int(is_d2_timing(self.prn)))

    def _decode(self, corr, state1, sample_counter):
        inverted = not corr > 0
        h = self.history
        frame = [-h[i] for i in range(PERIOD)] if inverted else [h[i] for i in range(PERIOD)]
        bits, mask = [], 0
        for w in range(10):
            dec, errs = decode_word(w + 1, frame[30 * w:30 * w + 30])
            bits += [1 if b > 0 else 0 for b in dec]
            if w:
                mask |= (1 if errs[0] else 0) << (2 * w - 2) | (1 if errs[1] else 0) << (2 * w - 1)
        d2 = is_d2_decoder(self.signal, self.prn)
        fra_id = self.nav.d2_subframe_decoder(bits) if d2 else self.nav.d1_subframe_decoder(bits)
        words = [read_unsigned(bits, [(30 * w + 1, 30)]) for w in range(10)]
        pnum = read_unsigned(bits, [(43, 4)]) if d2 else read_unsigned(bits, [(44, 7)])
        flags = (F_INVERTED if inverted else 0) | (F_STATE1 if state1 else 0) | (F_D2_DECODER if d2 else 0) | \
            (F_D2_TIMING if is_d2_timing(self.prn) else 0)
        rec = dict(symbol_counter=self.symbol_counter, sample_counter=sample_counter, channel=self.channel, words=words, fra_id=fra_id,
                   pnum=pnum, sow=0, corrected_mask=mask, tow_at_current_symbol_ms=0, flags=flags)
        # get_flag_CRC_test() is always true: the other branch (d_CRC_error_counter++, loss of sync) is unreachable
        self.crc_error_counter = 0
        self.preamble_index = self.symbol_counter
        self.frame_sync = True
        return rec

    def work(self, x, out_valid=True, sample_counter=0):
        """general_work (:468-711) on one symbol: (tow_ms, sflags, record or None)."""
        self.history.append(x)
        self.symbol_counter += 1
        flag_preamble = False
        corr = 0
        h = self.history
        if len(h) >= REQUIRED:
            for i in range(N_PRE):
                if h[i] < 0:
                    corr -= PREAMBLE[i]
                else:
                    corr += PREAMBLE[i]
        rec = None
        if self.stat == 0:
            if abs(corr) >= N_PRE:
                self.preamble_index = self.symbol_counter
                self.stat = 1
        elif self.stat == 1:
            if abs(corr) >= N_PRE:
                diff = ((self.symbol_counter - self.preamble_index + (1 << 31)) % (1 << 32)) - (1 << 31)  # static_cast<int32_t>
                if abs(diff - PERIOD) == 0:
                    self.preamble_index = self.symbol_counter
                    self.stat = 2
                    rec = self._decode(corr, True, sample_counter)
                    flag_preamble = True
                elif diff > PERIOD:
                    self.stat = 0
        elif self.stat == 2:
            if self.symbol_counter == self.preamble_index + PERIOD:
                rec = self._decode(corr, False, sample_counter)
                flag_preamble = True
        d = self.symbol_duration_ms
        if flag_preamble and self.nav.new_sow:
            self.tow_at_preamble_ms = ((self.nav.sow + LEAP) * 1000) & 0xFFFFFFFF
            last = self.tow_at_current_symbol_ms
            self.tow_at_current_symbol_ms = (self.tow_at_preamble_ms + REQUIRED * d) & 0xFFFFFFFF
            self.sow_set = True
            self.nav.new_sow = False
            rec["flags"] |= F_NEW_SOW
            if last != 0 and abs(self.tow_at_current_symbol_ms - last) > d:
                self.tow_at_current_symbol_ms = 0
                self.valid_word = False
                rec["flags"] |= F_TOW_ZEROED
            else:
                self.last_valid_preamble = self.symbol_counter
                self.valid_word = True
        elif self.valid_word:
            self.tow_at_current_symbol_ms = (self.tow_at_current_symbol_ms + d) & 0xFFFFFFFF
            if not out_valid:
                self.valid_word = False
        sflags = (S_VALID_WORD if self.valid_word else 0)
        if rec is not None:
            rec["sow"] = self.nav.sow
            rec["tow_at_current_symbol_ms"] = self.tow_at_current_symbol_ms
            sflags |= S_SUBFRAME | (S_INVERTED if rec["flags"] & F_INVERTED else 0)
        return self.tow_at_current_symbol_ms, sflags, rec


def run(decoders, symbols, valid=None, out_valid=None, sample_counters=None):
    """One device run over symbols[n_rounds, channels] on a list of Decoder objects: (records per channel, tow_ms, sflags)
    as the device lays them out; entries that are no symbols give 0 / 0."""
    symbols = np.asarray(symbols, np.float32)
    n, nc = symbols.shape
    tow, sf = np.zeros((n, nc), np.uint32), np.zeros((n, nc), np.uint8)
    records = []
    for c, dec in enumerate(decoders):
        col = symbols[:, c].tolist()
        v = [True] * n if valid is None else np.asarray(valid)[:, c].astype(bool).tolist()
        ov = [True] * n if out_valid is None else np.asarray(out_valid)[:, c].astype(bool).tolist()
        sc = [0] * n if sample_counters is None else np.asarray(sample_counters)[:, c].tolist()
        recs = []
        for r in range(n):
            if not v[r]:
                continue
            t, s, rec = dec.work(col[r], ov[r], sc[r])
            tow[r, c], sf[r, c] = t, s
            if rec is not None:
                recs.append(rec)
        records.append(recs)
    return records, tow, sf


# ------------------------------------------------------------------ the transmitter ---------------------------------
def bch_parity(info):
    """The ICD's BCH(15,11,1) encoder, g(x) = x^4 + x + 1, systematic: four parity bits of eleven information bits."""
    reg = [0, 0, 0, 0]  # d0..d3
    for b in info:
        fb = b ^ reg[3]
        reg = [fb, reg[0] ^ fb, reg[1], reg[2]]
    return [reg[3], reg[2], reg[1], reg[0]]


def bch_encode(info):
    return list(info) + bch_parity(info)


def int_bits(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def build_subframe(d2, fra_id, pnum, sow, payload):
    """(the 300 bits as the decoders should restore them, the 300 bits on the air).  payload: at least 182 bits, consumed as
    needed.  Word 1: preamble, four reserved bits, FraID, the SOW's upper 8 bits, BCH parity over bits 16..26.  Word 2: the
    SOW's lower 12 bits, then Pnum in bits 43..46 (D2) or 44..50 (D1).  Words 2..10: two BCH codewords, interleaved."""
    payload = [int(b) for b in payload]
    head = int_bits(fra_id, 3) + int_bits(sow >> 12, 8)
    plain = [1 if p > 0 else 0 for p in PREAMBLE] + [0, 0, 0, 0] + head + bch_parity(head)
    air = list(plain)
    if d2:
        info2 = int_bits(sow & 0xFFF, 12) + int_bits(pnum, 4) + payload[:6]
        rest = payload[6:]
    else:
        info2 = int_bits(sow & 0xFFF, 12) + payload[:1] + int_bits(pnum, 7) + payload[1:3]
        rest = payload[3:]
    infos = [info2] + [rest[22 * k:22 * k + 22] for k in range(8)]
    for info in infos:
        a, b = bch_encode(info[:11]), bch_encode(info[11:])
        plain += a[:11] + b[:11] + a[11:] + b[11:]
        for c in range(15):
            air += [a[c], b[c]]
    return plain, air


def symbols_of(air_bits, inverted=False, amplitude=1.0):
    s = np.where(np.asarray(air_bits) > 0, 1.0, -1.0).astype(np.float32) * np.float32(amplitude)
    return -s if inverted else s


def stream(subframes, lead=0, inverted=False, rng=None, tail=0):
    """`lead` random symbols (free of preamble look-alikes is not promised; use a seed that the test checks), the
    subframes' air bits, `tail` symbols of +1."""
    parts = []
    if lead:
        parts.append(np.where(rng.integers(0, 2, lead) > 0, 1.0, -1.0).astype(np.float32))
    for air in subframes:
        parts.append(symbols_of(air, inverted))
    if tail:
        parts.append(np.ones(tail, np.float32))
    return np.concatenate(parts)
