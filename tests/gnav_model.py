"""A numpy / Python restatement of glonass_l1_ca_telemetry_decoder_gs (and its L2 twin, the same algorithm) with what it
uses of Glonass_Gnav_Navigation_Message (CRC_test, string_decoder, have_new_ephemeris, have_new_utc_model) and of
Glonass_Gnav_Ephemeris::glot_to_gpst, and a transmitter beside it.  Written from the blocks' behaviour, oddities included
(include/gnsship.h lists them); tests/golden/gnav_ref.npz pins the navigation-object part to the reference itself.

The decoder keeps the symbols as doubles and decodes a string from the history in one go, as the block does; the device
accumulates half-bits as symbols stream in.  The calendar here is Python's datetime; the device counts days itself.
The correlation is computed on integers, for a whole run at once, and looked at only where a state needs it."""
from __future__ import annotations

import datetime

import numpy as np

L1CA, L2CA = 0, 1
RING, PRE, DATA = 2000, 300, 1700
CRC_ERROR_LIMIT = 6
MARK = [int(ch) for ch in "111110001101110101000010010110"]  # the time mark, first bit first
MARK_SYMBOLS = np.repeat(np.where(np.array(MARK) == 1, 1, -1), 10).astype(np.int32)
# record flags, entry flags
CRC_OK, CORRECTED, INVERTED, NEW_TOW, SLOT_UPDATED, NEW_EPHEMERIS, NEW_UTC_MODEL = 1, 2, 4, 8, 16, 32, 64
S_VALID_WORD, S_STRING, S_INVERTED = 1, 2, 4

# The Hamming code of the ICD over bits[0..84] (bits[n - 1] is the ICD's bit n): bits[0..6] are beta_1..beta_7, bits[7] the
# overall parity, and information bit bits[8 + i] carries the i-th syndrome that is no power of two.
SYNDROME_OF = [1 << k for k in range(7)] + [0] + [s for s in range(3, 128) if s & (s - 1)][:77]
LOCATOR = [0] * 85  # GLONASS_GNAV_ECC_LOCATOR: syndrome -> bit
for _b, _s in enumerate(SYNDROME_OF):
    if _b != 7 and _s < 85:
        LOCATOR[_s] = _b
LEAP = [(datetime.datetime(y, m, 1), s) for y, m, s in
        [(2017, 1, 18), (2015, 7, 17), (2012, 7, 16), (2009, 1, 15), (2006, 1, 14), (1999, 1, 13), (1997, 7, 12), (1996, 1, 11), (1994, 7, 10),
         (1993, 7, 9), (1992, 7, 8), (1991, 1, 7), (1990, 1, 6), (1988, 1, 5), (1985, 7, 4), (1983, 7, 3), (1982, 7, 2), (1981, 7, 1)]]
GPS_EPOCH = datetime.date(1980, 1, 6)
# string fields as (first character, 1-based; length)
F_STRING_ID, F_TK_HR, F_TK_MIN, F_TK_SEC, F_TB = (2, 4), (10, 5), (15, 6), (21, 1), (10, 7)
F_NT, F_N, F_TAU_C, F_N4, F_TAU_GPS, F_NA = (60, 11), (71, 5), (17, 32), (50, 5), (55, 22), (9, 5)


def strings_per_run(max_rounds: int) -> int:
    return max_rounds // 2000 + 1


# ------------------------------------------------------------------------------------------------ the navigation object
def field(bits, f):
    """read_navigation_unsigned: bits is the bitset (bits[84 - i] is character i)."""
    v = 0
    for j in range(f[1]):
        v = (v << 1) | bits[85 - f[0] - j]
    return v


def signed_field(bits, f):
    """read_navigation_signed: sign and magnitude."""
    v = field(bits, (f[0] + 1, f[1] - 1))
    return -v if bits[85 - f[0]] else v


def crc_test(bits):
    """CRC_test on the bitset (a list of 85 ints, changed in place): (accepted, flipped bit or -1)."""
    c = [0] * 7
    for k in range(7):
        c[k] = sum(bits[b] for b in range(85) if b != 7 and (SYNDROME_OF[b] >> k) & 1) & 1
    q = sum(bits[8:]) & 1            # sum_bits as the C_Sigma computation leaves it
    c_sigma = (sum(bits[:8]) & 1) ^ q
    if sum(c) + c_sigma == 0:
        return True, -1
    if c_sigma == 1 and sum(c) == 1:
        return True, -1
    if c_sigma and q:
        syndrome = sum(c[k] << k for k in range(7))
        if syndrome < 85:
            bits[LOCATOR[syndrome]] ^= 1
            return True, LOCATOR[syndrome]
        return False, -1
    return False, -1


def glot_to_gpst(n_4, n_t, tod_offset, tau_c, tau_gps):
    """(d_WN, d_TOW) of glot_to_gpst(tod_offset, tau_c, tau_gps) with d_N_T = n_t and the year string 5 derives from N_4."""
    return glot_to_gpst_from(1996 + 4 * (n_4 - 1), n_t, tod_offset, tau_c, tau_gps)


def glot_to_gpst_from(year, n_t, tod_offset, tau_c, tau_gps):
    """The same from the year the day count starts in (d_yr - J + 1); the offset's seconds are truncated to an integer."""
    utc = datetime.datetime(int(year), 1, 1) + datetime.timedelta(days=int(n_t) - 1, seconds=int(tod_offset - 10800))
    gps = None
    for when, leap in LEAP:
        if utc >= when:
            gps = utc + datetime.timedelta(seconds=leap)
            break
    days = float((utc.date() - GPS_EPOCH).days)
    sec_of_day = float(gps.hour * 3600 + gps.minute * 60 + gps.second)
    total = days * 86400 + sec_of_day
    wn = int(np.floor(total / 604800))
    tow = total - 604800 * np.floor(total / 604800)
    tow = float(tow) + (tau_c + tau_gps)
    return wn, tow


class NavMessage:
    """What Glonass_Gnav_Navigation_Message keeps that reaches the time of week."""

    def __init__(self):
        self.crc = False
        self.bits = [0] * 85   # after the last CRC_test
        self.flipped = -1
        self.string_id = 0
        self.e = [False] * 4   # flag_ephemeris_str_1..4
        self.utc5 = False
        self.tow_set = self.tow_new = self.update_slot = False
        self.t_k = self.t_b = self.previous_tb = 0
        self.n_t = self.n = self.n_4 = 0
        self.tau_c = self.tau_gps = 0.0
        self.tow, self.wn = 0.0, 0

    def string_decoder(self, chars) -> int:
        """chars: 85 ints, character 0 first.  Returns what string_decoder returns."""
        bits = [int(chars[84 - i]) for i in range(85)]
        self.crc, self.flipped = crc_test(bits)
        self.bits = bits
        if not self.crc:
            return 0
        sid = self.string_id = field(bits, F_STRING_ID)
        if sid == 1:
            self.t_k = field(bits, F_TK_HR) * 3600 + field(bits, F_TK_MIN) * 60 + field(bits, F_TK_SEC) * 30
            self.e[0] = True
        elif sid == 2:
            if self.e[0]:
                self.t_b = field(bits, F_TB) * 900
                self.e[1] = True
        elif sid == 3:
            if self.e[1]:
                self.e[2] = True
        elif sid == 4:
            if self.e[2]:
                self.n_t, self.n = field(bits, F_NT), field(bits, F_N)
                self.update_slot = True
                self.e[3] = True
        elif sid == 5:
            if self.e[3]:
                self.tau_c = float(signed_field(bits, F_TAU_C)) * 2.0 ** -31
                self.n_4 = field(bits, F_N4)
                self.tau_gps = float(signed_field(bits, F_TAU_GPS)) * 2.0 ** -30
                self.utc5 = True
                if self.e[0]:
                    self.wn, self.tow = glot_to_gpst(self.n_4, self.n_t, self.t_k + 10, self.tau_c, self.tau_gps)
                    self.tow_set = self.tow_new = True
        elif sid in (6, 8, 10, 12, 14):  # the almanac strings return 0 on a slot number outside 1..24 (d_frame_ID is 0 at string 14)
            if not 1 <= field(bits, F_NA) <= 24:
                return 0
        return sid

    def have_new_ephemeris(self) -> bool:
        if all(self.e) and self.utc5 and self.previous_tb != self.t_b:
            self.e = [False] * 4
            self.previous_tb = self.t_b
            return True
        return False

    def have_new_utc_model(self) -> bool:
        if self.utc5:
            self.utc5 = False
            return True
        return False


# ------------------------------------------------------------------------------------------------ the block
def round_half_away(x: float) -> int:
    """C's round() of a finite double, as an int."""
    a = abs(x)
    r = int(np.floor(a))
    if a - r >= 0.5:
        r += 1
    return -r if x < 0 else r


def pack_bits(bits):
    """The bitset as three uint32."""
    return [sum(int(bits[32 * w + b]) << b for b in range(32) if 32 * w + b < 85) for w in range(3)]


class Decoder:
    """One block object on one channel."""

    def __init__(self, prn: int = 0, channel: int = 0):
        self.prn, self.channel = prn, channel
        self.counter = self.preamble_index = 0
        self.stat = self.crc_error_counter = 0
        self.frame_sync = False
        self.tow_cur = 0.0
        self.hist = np.zeros(0, np.float64)  # the last <= 2000 symbols, oldest first
        self.nav = NavMessage()

    def set_satellite(self, prn: int):
        self.prn = prn

    def decode_string(self, sym):
        """decode_string over the 1700 symbols (already under the polarity): the 85 characters."""
        sums = np.cumsum(sym.reshape(170, 10), axis=1)[:, -1]  # in order; 0.0 + x is x but for -0.0, which tests as 0.0 does
        half = sums > 0
        rel = half[0::2] & ~half[1::2]
        return [0] + [int(rel[i - 1] ^ rel[i]) for i in range(1, 85)]

    def run(self, symbols, valid=None, sample_counters=None):
        """symbols[n] (any float type, taken as doubles), valid[n] or None, sample_counters[n] or None: the records (dicts),
        tow_ms uint32[n], sflags uint8[n]."""
        x_all = np.asarray(symbols, np.float64).reshape(-1)
        n = len(x_all)
        idx = np.arange(n) if valid is None else np.nonzero(np.asarray(valid).reshape(-1))[0]
        x = x_all[idx]
        tow_ms, sflags, recs = np.zeros(n, np.uint32), np.zeros(n, np.uint8), []
        had = len(self.hist)
        everything = np.concatenate([self.hist, x])
        sgn = c_all = None

        def corr_at(j):
            """corr_value at new symbol j: the mark against the 300 oldest entries, 0 while there are fewer."""
            nonlocal sgn, c_all
            held = min(had + 1 + j, RING)
            if held < PRE:
                return 0
            start = had + 1 + j - held
            if sgn is None:
                sgn = np.where(everything < 0.0, -1, 1).astype(np.int32)
            if c_all is None:
                if len(x) - j <= 8:
                    return int(np.dot(sgn[start:start + PRE], MARK_SYMBOLS))
                c_all = np.correlate(sgn, MARK_SYMBOLS, "valid")  # c_all[k]: the mark against entries k .. k + 299
            return int(c_all[start])

        nav = self.nav
        for j in range(len(x)):
            self.counter += 1
            due = self.stat == 2 and self.counter == self.preamble_index + RING
            corr_value = corr_at(j) if self.stat != 2 or due else 0  # state 2 looks at it on the due symbol only
            hit = abs(corr_value) >= PRE
            flag_preamble = decoded = inverted = False
            if self.stat == 0:
                if hit:
                    self.preamble_index, self.stat = self.counter, 1
            elif self.stat == 1:
                if hit:
                    diff = self.counter - self.preamble_index
                    if diff == RING:
                        self.preamble_index, self.stat = self.counter, 2
                    elif diff > RING:
                        self.stat = 0
            elif due:
                decoded, inverted = True, not corr_value > 0
                end = had + j + 1
                sym = everything[end - DATA:end]  # history entries 300..1999
                ret = nav.string_decoder(self.decode_string(-sym if inverted else sym))
                new_eph, new_utc = nav.have_new_ephemeris(), nav.have_new_utc_model()
                slot = nav.update_slot
                if slot:
                    self.prn, nav.update_slot = nav.n, False
                self.preamble_index = self.counter
                if nav.crc:
                    self.crc_error_counter, flag_preamble, self.frame_sync = 0, True, True
                else:
                    self.crc_error_counter += 1
                    if self.crc_error_counter > CRC_ERROR_LIMIT:
                        self.frame_sync, self.stat = False, 0
                del ret
            stamped = flag_preamble and nav.tow_new
            if stamped:
                self.tow_cur = float(np.floor((nav.tow - 0.3) * 1000) / 1000)
                nav.tow_new = False
            else:
                self.tow_cur = self.tow_cur + 0.001
            out = round_half_away(self.tow_cur * 1000.0) & 0xFFFFFFFF
            tow_ms[idx[j]] = out
            sflags[idx[j]] = (S_VALID_WORD if self.frame_sync and nav.tow_set else 0) | (S_STRING if decoded else 0) | (S_INVERTED if decoded and inverted else 0)
            if decoded:
                recs.append(dict(symbol_counter=self.counter, sample_counter=0 if sample_counters is None else int(np.asarray(sample_counters).reshape(-1)[idx[j]]),
                                 tow=nav.tow, bits=pack_bits(nav.bits), channel=self.channel, prn=self.prn, string_id=field(nav.bits, F_STRING_ID),
                                 flipped_bit=nav.flipped, tow_at_current_symbol_ms=out,
                                 flags=(CRC_OK if nav.crc else 0) | (CORRECTED if nav.flipped >= 0 else 0) | (INVERTED if inverted else 0) |
                                 (NEW_TOW if stamped else 0) | (SLOT_UPDATED if slot else 0) | (NEW_EPHEMERIS if new_eph else 0) |
                                 (NEW_UTC_MODEL if new_utc else 0)))
        self.hist = everything[-RING:] if len(everything) > RING else everything
        return recs, tow_ms, sflags

    def state(self) -> dict:
        """The members gnsship_gnav_state names, under its field names."""
        nav, size = self.nav, len(self.hist)
        history = np.zeros(64, np.uint32)
        p = (self.counter - size + 1 + np.nonzero(self.hist < 0.0)[0]) % RING
        np.bitwise_or.at(history, p >> 5, (1 << (p & 31)).astype(np.uint32))
        half_pos, half_neg, acc = np.zeros(6, np.uint32), np.zeros(6, np.uint32), 0.0
        if self.stat == 2:
            got = min(max(self.counter - self.preamble_index - PRE, 0), DATA)  # data symbols of the string in flight
            sym = self.hist[size - got:]
            full = got // 10
            if full:
                sums = np.cumsum(sym[:10 * full].reshape(full, 10), axis=1)[:, -1]
                for out, which in ((half_pos, sums > 0), (half_neg, sums < 0)):
                    h = np.nonzero(which)[0]
                    np.bitwise_or.at(out, h >> 5, (1 << (h & 31)).astype(np.uint32))
            for v in sym[10 * full:]:
                acc = acc + float(v)
        return dict(symbol_counter=self.counter, preamble_index=self.preamble_index, tow_at_current_symbol=self.tow_cur, tow=nav.tow, tau_c=nav.tau_c,
                    tau_gps=nav.tau_gps, chip_acc=acc, stat=self.stat, crc_error_counter=self.crc_error_counter, history_size=size, prn=self.prn,
                    wn=nav.wn, t_k=nav.t_k, t_b=nav.t_b, previous_tb=nav.previous_tb, n_t=nav.n_t, n=nav.n, n_4=nav.n_4,
                    frame_sync=int(self.frame_sync), ephemeris_str=[int(f) for f in nav.e], utc_model_str_5=int(nav.utc5), tow_set=int(nav.tow_set),
                    tow_new=int(nav.tow_new), half_pos=half_pos.tolist(), half_neg=half_neg.tolist(), history=history.tolist())


def run(decoders, symbols, valid=None, sample_counters=None):
    """symbols[n_rounds, C] over C decoders: per channel the records, and tow_ms / sflags [n_rounds, C]."""
    symbols = np.asarray(symbols)
    n, C = symbols.shape
    tow, sf, recs = np.zeros((n, C), np.uint32), np.zeros((n, C), np.uint8), []
    for c, d in enumerate(decoders):
        r, tow[:, c], sf[:, c] = d.run(symbols[:, c], None if valid is None else np.asarray(valid)[:, c],
                                       None if sample_counters is None else np.asarray(sample_counters)[:, c])
        recs.append(r)
    return recs, tow, sf


# ------------------------------------------------------------------------------------------------ the transmitter
def build_string(string_id: int, fields=(), payload=None):
    """The 85 characters of a string, character 0 first: the idle bit, the string number, `payload` (72 ints or None for
    zeros) overlaid with fields [((first, length), value), ...], and the ICD's Hamming bits."""
    ch = [0] * 85
    if payload is not None:
        ch[5:77] = [int(b) & 1 for b in payload]
    for (first, length), value in [(F_STRING_ID, string_id)] + list(fields):
        for j in range(length):
            ch[first - 1 + j] = (int(value) >> (length - 1 - j)) & 1
    bits = [ch[84 - i] for i in range(85)]
    for k in range(8):
        bits[k] = 0
    for k in range(7):
        bits[k] = sum(bits[b] for b in range(8, 85) if (SYNDROME_OF[b] >> k) & 1) & 1
    bits[7] = sum(bits) & 1
    return [bits[84 - i] for i in range(85)]


def sign_magnitude(value: int, length: int) -> int:
    return (1 << (length - 1)) | -value if value < 0 else value


def frame_strings(t_k_raw=0, t_b_raw=1, n_t=1, n=1, n_4=1, tau_c=0, tau_gps=0, rng=None, ids=(1, 2, 3, 4, 5)):
    """Strings `ids` of one frame: t_k_raw the 12 raw bits of t_k, t_b_raw 7 bits, tau_c / tau_gps signed integers in units
    of 2^-31 / 2^-30.  Random payloads around the fields when rng is given."""
    per = {1: [((10, 12), t_k_raw)], 2: [(F_TB, t_b_raw)], 3: [], 4: [(F_NT, n_t), (F_N, n)],
           5: [(F_TAU_C, sign_magnitude(tau_c, 32)), (F_N4, n_4), (F_TAU_GPS, sign_magnitude(tau_gps, 22))]}
    return [build_string(i, per.get(i, []), None if rng is None else rng.integers(0, 2, 72)) for i in ids]


def string_symbols(chars):
    """Relative code, meander half-bits at 10 symbols each, then the time mark: 2000 symbols of +-1, the time mark last."""
    rel, half = 0, []
    for i, b in enumerate(chars):
        rel = 0 if i == 0 else rel ^ int(b)
        half += [1, -1] if rel else [-1, 1]
    return np.concatenate([np.repeat(np.array(half, np.int32), 10), MARK_SYMBOLS]).astype(np.float32)


def stream(strings, lead=0, inverted=False, amplitude=1.0):
    """`lead` symbols of +1, one time mark, then the strings: each string's data follow a time mark, as the block wants."""
    x = np.concatenate([np.ones(lead, np.float32), MARK_SYMBOLS.astype(np.float32)] + [string_symbols(s) for s in strings])
    return (x * np.float32(-amplitude if inverted else amplitude)).astype(np.float32)
