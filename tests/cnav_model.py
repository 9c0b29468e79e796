"""A plain-Python restatement of the reference's GPS CNAV chain, the model the device (gnsship_cnav_*) is tested against:
libswiftcnav (cnav_msg.c, viterbi27.c, bits.c, edc.c) member for member, and on top of it the general_work and reset of
gps_l2c_telemetry_decoder_gs and gps_l5_telemetry_decoder_gs.  Properties a clean-room decoder would not have are kept,
not repaired (include/gnsship.h, the gnsship_cnav_* section, lists them).  Every branch of interest counts itself in
``Decoder.br``.  The transmitter at the end builds the test streams."""
from __future__ import annotations

import math

import numpy as np

L2C, L5 = 0, 1
POLY_A, POLY_B = 0x4F, 0x6D
PREAMBLE1, PREAMBLE2 = 0x8B, 0x74
PREAMBLE_LEN, MSG_LEN, CRC_LEN = 8, 300, 24
DATA_LEN = MSG_LEN - CRC_LEN
MAX_CRC_FAILS = 10
INIT_BITS = DECODE_BITS = DELAY_BITS = 32
HISTORY = 64
NORM_LIMIT = 1 << 30
U32, U64 = 0xFFFFFFFF, (1 << 64) - 1

# gnsship_cnav_message.flags and the sflags of an entry
F_CRC_OK, F_INVERTED, F_LOCK = 1, 2, 4
S_VALID_WORD, S_PLL_180, S_MESSAGE = 1, 2, 4

WATCHDOG = {L2C: MSG_LEN * 2 * 5, L5: MSG_LEN * 2 * 10}
L2_PERIOD_S, L5_PERIOD_MS = 0.02, 10

BRANCHES = ("rescan_hit", "rescan_miss", "retry_crc_no_lock", "lock_lost", "flush_part1", "flush_part2", "norm_taken",
            "norm_skipped_above", "lock_acquired", "locked_crc_fail", "disposed_ok", "disposed_bad")


def parity(x: int) -> int:
    return bin(x & U32).count("1") & 1


# v27_poly_init over {0x4F, 0x6D}: both coefficients are positive
C0 = np.array([255 if parity((2 * s) & POLY_A) else 0 for s in range(32)], np.uint32)
C1 = np.array([255 if parity((2 * s) & POLY_B) else 0 for s in range(32)], np.uint32)


def _crc24q_table():
    tab = []
    for b in range(256):
        crc = b << 16
        for _ in range(8):
            crc <<= 1
            if crc & 0x1000000:
                crc ^= 0x1864CFB
        tab.append(crc & 0xFFFFFF)
    return tab


CRC24Q = _crc24q_table()


def crc24q_bits(crc: int, buf, n_bits: int, invert: bool) -> int:
    """edc.c crc24q_bits: the message left-aligned in buf, as if prepended with zero bits up to a byte boundary."""
    acc, shift = 0, 8 - n_bits % 8
    for i in range(n_bits // 8 + 1):
        acc = ((acc << 8) | buf[i]) & 0xFFFF
        if invert:
            acc ^= 0xFF
        b = (acc >> shift) & 0xFF
        crc = ((crc << 8) & 0xFFFFFF) ^ CRC24Q[((crc >> 16) ^ b) & 0xFF]
    return crc


def getbitu(buf, pos: int, n: int) -> int:
    bits = 0
    for i in range(pos, pos + n):
        bits = (bits << 1) + ((buf[i // 8] >> (7 - i % 8)) & 1)
    return bits


def setbitu(buf, pos: int, n: int, data: int):
    mask = 1 << (n - 1)
    for i in range(pos, pos + n):
        if data & mask:
            buf[i // 8] |= 1 << (7 - i % 8)
        else:
            buf[i // 8] &= ~(1 << (7 - i % 8)) & 0xFF
        mask >>= 1


def bitshl(buf, shift: int):
    """bits.c bitshl on the whole buffer: an MSB-first left shift with zero fill."""
    size = len(buf)
    if shift > size * 8:
        buf[:] = bytes(size)
        return
    v = (int.from_bytes(bytes(buf), "big") << shift) & ((1 << (size * 8)) - 1)
    buf[:] = v.to_bytes(size, "big")


class Part:
    """cnav_v27_part_t with its v27_t.  metrics[0] / metrics[1] are metrics1 / metrics2; ``old`` says which of them
    old_metrics points at, new_metrics is the other."""

    SCALARS = ("n_symbols", "n_decoded", "preamble_seen", "invert", "message_lock", "crc_ok", "n_crc_fail", "init",
               "decisions_index", "old")

    def __init__(self, br):
        self.br = br
        self.metrics = [np.full(64, 63, np.uint32), np.zeros(64, np.uint32)]
        self.metrics[0][0] = 0
        self.old = 0
        self.decisions = np.zeros((HISTORY, 2), np.uint32)
        self.decisions_index = 0
        self.symbols = bytearray(2 * (INIT_BITS + DECODE_BITS))
        self.n_symbols = 0
        self.decoded = bytearray(DECODE_BITS + DELAY_BITS)
        self.n_decoded = 0
        self.preamble_seen = self.invert = self.message_lock = self.crc_ok = False
        self.n_crc_fail = 0
        self.init = True

    # ---- viterbi27.c ----
    def v27_update(self, nbits: int):
        for b in range(nbits):
            s0, s1 = np.uint32(self.symbols[2 * b]), np.uint32(self.symbols[2 * b + 1])
            old, new = self.metrics[self.old], self.metrics[self.old ^ 1]
            metric = (C0 ^ s0) + (C1 ^ s1)
            m0 = old[:32] + metric
            m1 = old[32:] + (np.uint32(510) - metric)
            d0 = (m0 - m1).view(np.int32) > 0
            new[0::2] = np.where(d0, m1, m0)
            t = metric + metric - np.uint32(510)
            m0 = m0 - t
            m1 = m1 + t
            d1 = (m0 - m1).view(np.int32) > 0
            new[1::2] = np.where(d1, m1, m0)
            dec = np.zeros(64, np.uint64)
            dec[0::2], dec[1::2] = d0, d1
            word = int((dec << np.arange(64, dtype=np.uint64)).sum())
            self.decisions[self.decisions_index] = (word & U32, word >> 32)
            if int(new[0]) > NORM_LIMIT:  # state 0 alone is tested
                self.br["norm_taken"] += 1
                new -= np.uint32(min(1 << 31, int(new.min())))
            elif int(new.max()) > NORM_LIMIT:
                self.br["norm_skipped_above"] += 1
            self.decisions_index = (self.decisions_index + 1) % HISTORY
            self.old ^= 1  # the swap: new_metrics now names the buffer the step read from

    def v27_chainback_likely(self, nbits: int) -> bytearray:
        stale = self.metrics[self.old ^ 1]  # new_metrics after the swap: the metrics of the step before the last
        best = int(np.argmin(stale))  # the first minimum
        data = bytearray((nbits + 7) // 8)
        final_state = (best % 64) << 2
        idx = self.decisions_index
        while nbits != 0:
            nbits -= 1
            idx = HISTORY - 1 if idx == 0 else idx - 1
            s = final_state >> 2
            k = (int(self.decisions[idx][s // 32]) >> (s % 32)) & 1
            final_state = ((final_state >> 1) | (k << 7)) & 0xFF
            data[nbits >> 3] = final_state
        return data

    # ---- cnav_msg.c ----
    def rescan_preamble(self):
        self.preamble_seen = False
        if self.n_decoded > PREAMBLE_LEN + 1:
            for i in range(1, self.n_decoded - PREAMBLE_LEN):
                c = getbitu(self.decoded, i, PREAMBLE_LEN)
                if c in (PREAMBLE1, PREAMBLE2):
                    self.preamble_seen = True
                    self.invert = c == PREAMBLE2
                    bitshl(self.decoded, i)
                    self.n_decoded -= i
                    self.br["rescan_hit"] += 1
                    break
        if not self.preamble_seen and self.n_decoded >= PREAMBLE_LEN:
            bitshl(self.decoded, self.n_decoded - PREAMBLE_LEN + 1)
            self.n_decoded = PREAMBLE_LEN - 1
            self.br["rescan_miss"] += 1

    def add_symbol(self, ch: int):
        self.symbols[self.n_symbols] = ch
        self.n_symbols += 1
        if self.init:
            if self.n_symbols < (INIT_BITS + DECODE_BITS) * 2:
                return
            self.init = False
        elif self.n_symbols < DECODE_BITS * 2:
            return
        self.v27_update(self.n_symbols // 2)
        self.n_symbols = 0
        tmp = self.v27_chainback_likely(DECODE_BITS + DELAY_BITS)
        setbitu(self.decoded, self.n_decoded, DECODE_BITS, getbitu(tmp, 0, DECODE_BITS))
        self.n_decoded += DECODE_BITS
        retry = True
        while retry:
            retry = False
            if not self.preamble_seen:
                self.rescan_preamble()
            if self.preamble_seen and MSG_LEN <= self.n_decoded:
                crc = crc24q_bits(0, self.decoded, DATA_LEN, self.invert)
                crc2 = getbitu(self.decoded, DATA_LEN, CRC_LEN) ^ (0xFFFFFF if self.invert else 0)
                if self.message_lock:
                    self.crc_ok = crc == crc2
                    if self.crc_ok:
                        self.n_crc_fail = 0
                    else:
                        self.br["locked_crc_fail"] += 1
                        self.n_crc_fail += 1
                        if self.n_crc_fail > MAX_CRC_FAILS:
                            self.n_crc_fail = 0
                            self.message_lock = False
                            self.preamble_seen = False
                            self.br["lock_lost"] += 1
                            retry = True
                elif crc == crc2:
                    self.message_lock = True
                    self.crc_ok = True
                    self.n_crc_fail = 0
                    self.br["lock_acquired"] += 1
                else:
                    self.crc_ok = False
                    self.preamble_seen = False
                    self.br["retry_crc_no_lock"] += 1
                    retry = True

    def msg_decode(self):
        """cnav_msg_decode_: (res, record) — record is None when fewer than 300 bits are held, else what the buffer was
        disposed of as, CRC good or not (the fields are read from the un-inverted copy either way)."""
        if self.n_decoded < MSG_LEN:
            return False, None
        raw = bytes(b ^ 0xFF for b in self.decoded) if self.invert else bytes(self.decoded)
        rec = dict(prn=getbitu(raw, 8, 6), msg_id=getbitu(raw, 14, 6), tow=getbitu(raw, 20, 17), alert=getbitu(raw, 37, 1), raw=raw,
                   delay=(self.n_decoded - MSG_LEN + DELAY_BITS) * 2 + self.n_symbols, crc_ok=bool(self.crc_ok), invert=bool(self.invert))
        res = bool(self.crc_ok)
        self.br["disposed_ok" if res else "disposed_bad"] += 1
        bitshl(self.decoded, MSG_LEN)
        self.n_decoded -= MSG_LEN
        rec["lock"] = bool(self.message_lock)
        return res, rec

    def scalars(self):
        return [int(getattr(self, n)) for n in self.SCALARS]


class Decoder:
    """cnav_msg_decoder_t: cnav_msg_decoder_init, then cnav_msg_decoder_add_symbol per symbol."""

    def __init__(self):
        self.br = {k: 0 for k in BRANCHES}
        self.part1, self.part2 = Part(self.br), Part(self.br)
        self.part2.add_symbol(0x80)

    @property
    def parts(self):
        return (self.part1, self.part2)

    def add_symbol(self, symbol: int):
        """(res, record): res is the library's return value, record every disposal (part 0 / 1 in record['part'])."""
        self.part1.add_symbol(symbol)
        self.part2.add_symbol(symbol)
        for k, (p, other) in enumerate(((self.part1, self.part2), (self.part2, self.part1))):
            if p.message_lock:
                if other.n_decoded or other.n_symbols > 1:
                    self.br["flush_part2" if k == 0 else "flush_part1"] += 1
                other.n_decoded = 0
                other.n_symbols = 0
                res, rec = p.msg_decode()
                if rec is not None:
                    rec["part"] = k
                return res, rec
        return False, None

    def add_metrics(self, bias: int):
        """What tests/golden/cnav_ref_shim.c's ref_cnav_add_metrics does: bias every metric of both buffers of both parts."""
        for p in self.parts:
            for m in p.metrics:
                m += np.uint32(bias)


def _round_ms(x: float) -> int:
    """round(x) as uint32 for the non-negative x the block has; half away from zero."""
    if not x == x or x <= 0:
        return 0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return min(int(r), U32)


class CnavBlock:
    """gps_l2c_telemetry_decoder_gs (mode L2C) or gps_l5_telemetry_decoder_gs (mode L5): a new object, general_work per
    symbol, reset()."""

    def __init__(self, mode: int):
        self.mode = mode
        self.dec = Decoder()
        self.symbol_counter = 0
        self.last_valid_preamble = 0
        self.tow_s = 0.0          # L2C d_TOW_at_current_symbol
        self.tow_ms = 0           # L5 d_TOW_at_current_symbol_ms
        self.tow_at_preamble = 0  # L2C msg.tow, L5 msg.tow * 6000
        self.pll_180 = self.valid_word = self.sent_tlm_failed = False
        self.tow_inconsistent = 0

    def reset(self):
        self.last_valid_preamble = self.symbol_counter
        self.sent_tlm_failed = False
        if self.mode == L5:
            self.tow_ms = 0
            self.valid_word = False

    def work(self, x, out_valid=True, sample_counter=0, channel=0):
        """One symbol: (record or None, fault fired here, tow_ms, sflags)."""
        symbol = 255 if x > 0 else 0
        fired = False
        res, rec = self.dec.add_symbol(symbol)
        self.symbol_counter = (self.symbol_counter + 1) & U64
        if not self.sent_tlm_failed and ((self.symbol_counter - self.last_valid_preamble) & U64) > WATCHDOG[self.mode]:
            self.sent_tlm_failed = fired = True
        if res:
            self.pll_180 = self.dec.part1.invert or self.dec.part2.invert
            if self.mode == L2C:
                self.tow_at_preamble = rec["tow"]
                self.last_valid_preamble = self.symbol_counter
                self.tow_s = float(rec["tow"]) * 6.0 + float(rec["delay"]) * L2_PERIOD_S + 12 * L2_PERIOD_S
                self.valid_word = True
            else:
                self.tow_at_preamble = (rec["tow"] * 6000) & U32
                last = self.tow_ms
                self.tow_ms = (rec["tow"] * 6000 + (rec["delay"] + 12) * L5_PERIOD_MS) & U32
                if last != 0 and abs(self.tow_ms - last) > L5_PERIOD_MS:
                    self.tow_ms = 0
                    self.valid_word = False
                    self.tow_inconsistent += 1
                else:
                    self.last_valid_preamble = self.symbol_counter
                    self.valid_word = True
        elif self.mode == L2C:
            self.tow_s += L2_PERIOD_S
            if not out_valid:
                self.valid_word = False
        elif self.valid_word:
            self.tow_ms = (self.tow_ms + L5_PERIOD_MS) & U32
            if not out_valid:
                self.valid_word = False
        if self.mode == L2C:
            tow, sf = _round_ms(self.tow_s * 1000.0), (S_VALID_WORD if self.valid_word else 0) | (S_PLL_180 if self.pll_180 else 0)
        elif self.valid_word:
            tow, sf = self.tow_ms, S_VALID_WORD | (S_PLL_180 if self.pll_180 else 0)
        else:
            tow, sf = 0, 0
        if res:
            sf |= S_MESSAGE
        if rec is not None:
            rec = dict(rec, symbol_counter=self.symbol_counter, sample_counter=sample_counter, channel=channel,
                       flags=(F_CRC_OK if rec["crc_ok"] else 0) | (F_INVERTED if rec["invert"] else 0) | (F_LOCK if rec["lock"] else 0))
        return rec, fired, tow, sf

    def run(self, symbols, valid=None, out_valid=None, sample_counters=None, channel=0):
        """Entries in order: (records, fault, tow_ms uint32[n], sflags uint8[n]); entries that are no symbols give 0, 0."""
        n = len(symbols)
        tow, sf = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        recs, fault = [], False
        for k in range(n):
            if valid is not None and not valid[k]:
                continue
            rec, fired, tow[k], sf[k] = self.work(symbols[k], True if out_valid is None else bool(out_valid[k]),
                                                  0 if sample_counters is None else int(sample_counters[k]), channel)
            fault |= fired
            if rec is not None:
                recs.append(rec)
        assert len(recs) <= messages_per_run(n)
        return recs, fault, tow, sf

    def state(self) -> dict:
        """Every member, under the names of gnsship_cnav_state (parts as lists of two)."""
        st = {}
        for k, p in enumerate(self.dec.parts):
            st[f"part{k}"] = dict(metrics=np.stack(p.metrics).copy(), decisions=p.decisions.copy(),
                                  symbols=np.frombuffer(bytes(p.symbols), np.uint8).copy(), decoded=np.frombuffer(bytes(p.decoded), np.uint8).copy(),
                                  n_symbols=p.n_symbols, n_decoded=p.n_decoded, n_crc_fail=p.n_crc_fail, decisions_index=p.decisions_index,
                                  old_is_metrics2=p.old, preamble_seen=int(p.preamble_seen), invert=int(p.invert),
                                  message_lock=int(p.message_lock), crc_ok=int(p.crc_ok), init=int(p.init))
        st.update(symbol_counter=self.symbol_counter, last_valid_preamble=self.last_valid_preamble, tow_s=self.tow_s, tow_ms=self.tow_ms,
                  tow_at_preamble=self.tow_at_preamble, pll_180=int(self.pll_180), valid_word=int(self.valid_word),
                  sent_tlm_failed=int(self.sent_tlm_failed))
        return st

    def set_state(self, st: dict):
        for k, p in enumerate(self.dec.parts):
            s = st[f"part{k}"]
            p.metrics = [np.array(s["metrics"][0], np.uint32), np.array(s["metrics"][1], np.uint32)]
            p.decisions = np.array(s["decisions"], np.uint32).reshape(HISTORY, 2)
            p.symbols = bytearray(np.asarray(s["symbols"], np.uint8).tobytes())
            p.decoded = bytearray(np.asarray(s["decoded"], np.uint8).tobytes())
            p.n_symbols, p.n_decoded, p.n_crc_fail, p.decisions_index = (int(s[n]) for n in ("n_symbols", "n_decoded", "n_crc_fail", "decisions_index"))
            p.old = int(s["old_is_metrics2"])
            p.preamble_seen, p.invert, p.message_lock, p.crc_ok, p.init = (bool(s[n]) for n in ("preamble_seen", "invert", "message_lock", "crc_ok", "init"))
        self.symbol_counter, self.last_valid_preamble = int(st["symbol_counter"]), int(st["last_valid_preamble"])
        self.tow_s, self.tow_ms, self.tow_at_preamble = float(st["tow_s"]), int(st["tow_ms"]), int(st["tow_at_preamble"])
        self.pll_180, self.valid_word, self.sent_tlm_failed = bool(st["pll_180"]), bool(st["valid_word"]), bool(st["sent_tlm_failed"])


def messages_per_run(max_rounds: int) -> int:
    """GNSSHIP_CNAV_MESSAGES_PER_RUN."""
    return max_rounds // 300 + 4


# ---------------------------------------------------------------- the transmitter ----
def crc24q_of_bits(bits) -> int:
    crc = 0
    for b in bits:
        crc ^= int(b) << 23
        crc <<= 1
        if crc & 0x1000000:
            crc ^= 0x1864CFB
    return crc & 0xFFFFFF


def build_message(prn: int, msg_id: int, tow: int, body) -> np.ndarray:
    """300 bits: preamble 0x8B, 6-bit PRN, 6-bit ID, 17-bit TOW, 239 body bits (the alert flag first), CRC-24Q over 276."""
    body = [int(b) & 1 for b in body]
    assert len(body) == DATA_LEN - 37
    bits = [(PREAMBLE1 >> (7 - k)) & 1 for k in range(8)] + [(prn >> (5 - k)) & 1 for k in range(6)] + \
        [(msg_id >> (5 - k)) & 1 for k in range(6)] + [(tow >> (16 - k)) & 1 for k in range(17)] + body
    crc = crc24q_of_bits(bits)
    return np.array(bits + [(crc >> (23 - k)) & 1 for k in range(24)], np.uint8)


def encode(bits, sr: int = 0):
    """The K=7 rate-1/2 encoder, taps 0x4F / 0x6D, newest bit in bit 0: (symbols as bits, two per data bit; the register)."""
    out = []
    for b in bits:
        sr = ((sr << 1) | int(b)) & 0x7F
        out += [parity(sr & POLY_A), parity(sr & POLY_B)]
    return np.array(out, np.uint8), sr


def messages(n: int, seed: int, tow0: int = 1000, tow_step: int = 1, prn: int = 7):
    rng = np.random.default_rng(seed)
    return [build_message(prn, 10 + k % 5, tow0 + tow_step * k, rng.integers(0, 2, DATA_LEN - 37)) for k in range(n)]


def stream(msgs, lead: int = 0, seed: int = 0, invert: bool = False) -> np.ndarray:
    """Symbol bits (0 / 1): ``lead`` random symbols, then the encoded messages."""
    rng = np.random.default_rng(1000 + seed)
    sym, _ = encode(np.concatenate(msgs))
    out = np.concatenate([rng.integers(0, 2, lead).astype(np.uint8), sym])
    return out ^ 1 if invert else out


def to_float(sym_bits) -> np.ndarray:
    return np.where(np.asarray(sym_bits) > 0, 1.0, -1.0).astype(np.float32)


def ruined(msg) -> np.ndarray:
    """The message with one body bit inverted: the preamble stands, the CRC fails."""
    bad = msg.copy()
    bad[100] ^= 1
    return bad


NORM_BIAS = NORM_LIMIT - 300


def golden_streams() -> dict:
    """name -> (symbol bits, metric bias before the first symbol): the streams of tests/golden/cnav_ref.npz."""
    out = {}
    for lead in (0, 1, 37):
        for inv in (False, True):
            out[f"lead{lead}_{'neg' if inv else 'pos'}"] = (stream(messages(4, 11 + lead), lead, lead, inv), 0)
    s = stream(messages(5, 21), 5, 21)
    s[np.arange(40, len(s), 53)] ^= 1  # scattered flips, well inside what the code corrects
    out["flips"] = (s, 0)
    m = messages(17, 31)
    out["lossy"] = (stream(m[:2] + [ruined(x) for x in m[2:14]] + m[14:], 0, 31), 0)
    m = messages(4, 41)
    body = np.random.default_rng(41).integers(0, 2, DATA_LEN - 37)
    body[120:128] = [(PREAMBLE1 >> (7 - k)) & 1 for k in range(8)]
    m[0] = build_message(7, 10, 1000, body)
    out["lookalike"] = (stream(m, 0, 41)[100:], 0)  # from after the first preamble: the look-alike is met first
    out["norm_state0"] = (stream(messages(3, 51), 0, 51), NORM_BIAS)
    out["norm_others"] = (np.zeros(400, np.uint8), NORM_BIAS)
    return out
