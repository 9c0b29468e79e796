"""tests/gnav_model.py — the yardstick of the device GLONASS GNAV decoder — against the reference's own navigation object
(tests/golden/gnav_ref.npz, made by tests/golden/make_gnav_golden.py) and against the blocks' behaviour restated as cases.

The golden's time of week rests on a stand-in calendar, not on Boost (see make_gnav_golden.py, which checks that stand-in
against Python's datetime on every date it uses); everything else in it is the reference's code alone."""
import copy
import datetime
import os

import numpy as np
import pytest

import gnav_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gnav_ref.npz")
ORDER = (4, 5, 1, 2, 3, 4, 5, 1)


def bits_of(x) -> int:
    return int(np.float64(x).view(np.uint64))


def primed_model():
    """A model one symbol before the decode of a string 5 whose bits 8..84 have even parity, with strings 1..4 of its frame
    decoded: (model, the stream's remaining symbols, the string's characters)."""
    rng = np.random.default_rng(11)
    while True:
        strings = M.frame_strings(t_k_raw=0b01100_101010_1, t_b_raw=37, n_t=500, n=7, n_4=6, tau_c=-12345, tau_gps=777, rng=rng, ids=ORDER)
        if sum(strings[6][:77]) % 2 == 0:
            break
    x = M.stream(strings + strings[2:7], lead=3)
    m = M.Decoder(0, 0)
    m.run(x[:14002])
    assert m.stat == 2 and m.counter + 1 == m.preamble_index + 2000 and m.nav.e == [True] * 4 and not m.nav.tow_set
    return m, x[14002:], strings[6]


def with_string(template, chars):
    """A copy of the primed model whose history holds the data symbols of `chars` (the last of them still to come): the
    copy and that last symbol."""
    m = copy.deepcopy(template)
    sym = M.string_symbols(chars)[:1700].astype(np.float64)
    m.hist = m.hist.copy()
    m.hist[-1699:] = sym[:1699]
    return m, np.float32(sym[1699])


def whole_tow(n_4, n_t, t_k):
    """The whole seconds of week of glot_to_gpst(t_k + 10), by integer arithmetic on the days since 6 January 1980."""
    day = (datetime.date(1992 + 4 * n_4, 1, 1) - datetime.date(1980, 1, 6)).days + n_t - 1
    utc = day * 86400 + t_k + 10 - 10800
    leap = next(s for when, s in M.LEAP if utc >= (when.date() - datetime.date(1980, 1, 6)).days * 86400)
    return (utc // 86400 * 86400 + (utc + leap) % 86400) % 604800


@pytest.fixture(scope="module")
def primed():
    return primed_model()


def test_model_equals_the_reference_navigation_object():
    """Every call of every sequence: the return value, the CRC flag, the bits after CRC_test, the TOW flags, d_TOW (by its
    bits), d_WN, d_n, and what have_new_ephemeris / have_new_utc_model returned."""
    g = np.load(GOLDEN)
    nav, seq = None, -1
    seen = set()
    for k in range(len(g["ret"])):
        if g["seq"][k] != seq:
            nav, seq = M.NavMessage(), g["seq"][k]
        ret = nav.string_decoder(g["chars"][k].tolist())
        flags = [nav.crc, nav.tow_set, nav.tow_new, nav.have_new_ephemeris(), nav.have_new_utc_model(), nav.update_slot]
        nav.update_slot = False
        if nav.crc and nav.tow_new:
            nav.tow_new = False
        assert ret == g["ret"][k] and [int(f) for f in flags] == g["flags"][k].tolist(), (k, ret, flags, g["ret"][k], g["flags"][k])
        assert nav.bits == g["bits"][k].tolist(), k
        assert bits_of(nav.tow) == bits_of(g["tow"][k]) and nav.wn == g["wn"][k] and float(nav.n) == g["n"][k], (k, nav.tow, g["tow"][k])
        seen.add((ret, tuple(int(f) for f in flags)))
    assert len(g["ret"]) > 700 and len(seen) > 12  # the golden is not all one case
    assert g["flags"][:, 3].sum() >= 8 and (g["ret"] == 0).sum() > 100 and (g["tow"] != 0).any()


def test_model_equals_the_reference_glot_to_gpst():
    """Direct calls, among them negative and more-than-a-day offsets and leap additions that cross midnight (a day short,
    as in the source: the days come from the UTC date)."""
    g = np.load(GOLDEN)["glot"]
    crossed = 0
    for yr, n_t, tod, tc, tg, wn, tow in g:
        j = 1 if 1 <= n_t <= 366 else 2 if 367 <= n_t <= 731 else 3 if 732 <= n_t <= 1096 else 4 if 1097 <= n_t <= 1461 else 0
        got = M.glot_to_gpst_from(yr - j + 1, n_t, tod, tc, tg)
        assert (got[0], bits_of(got[1])) == (int(wn), bits_of(tow)), (yr, n_t, tod, got, wn, tow)
        crossed += (tod - 10800) % 86400 >= 86400 - 18
    assert crossed >= 2


def test_transmitter_strings_pass_the_check_uncorrected():
    rng = np.random.default_rng(1)
    for sid in range(16):
        for _ in range(20):
            ch = M.build_string(sid, (), rng.integers(0, 2, 72))
            bits = [ch[84 - i] for i in range(85)]
            assert M.crc_test(bits) == (True, -1) and bits == [ch[84 - i] for i in range(85)] and M.field(bits, M.F_STRING_ID) == sid


def test_single_bit_errors():
    """The block's third branch wants odd parity over bits 8..84 of the word AS RECEIVED.  A string whose information bits
    have even parity: an error in an information bit is corrected, one in beta_1..beta_7 is accepted as it is, the one in
    the overall parity bit is rejected.  A string with odd parity there: every information-bit error is rejected, and the
    parity-bit error is "corrected" by flipping bit 0.  No string has all 85 single errors accepted."""
    rng = np.random.default_rng(2)
    done = set()
    while len(done) < 2:
        ch = M.build_string(int(rng.integers(1, 16)), (), rng.integers(0, 2, 72))
        clean = [ch[84 - i] for i in range(85)]
        odd = sum(clean[8:]) & 1
        done.add(odd)
        for b in range(85):
            bits = list(clean)
            bits[b] ^= 1
            ok, flipped = M.crc_test(bits)
            if b < 7:
                assert (ok, flipped) == (True, -1) and bits[b] != clean[b]
            elif b == 7:
                assert (ok, flipped) == ((True, 0) if odd else (False, -1))
            else:
                assert (ok, flipped) == ((False, -1) if odd else (True, b))
                assert odd or bits == clean


def test_crc_branches_in_order():
    """Syndromes of one bit are taken by the second branch, so the locator entries 1, 2, 4, ... are never used; a syndrome
    of 85 or more with odd parity is rejected; an even overall parity with a non-zero syndrome is rejected."""
    ch = M.build_string(3, (), np.zeros(72, int))
    clean = [ch[84 - i] for i in range(85)]
    assert sum(clean[8:]) & 1 == 0
    bits = list(clean)
    bits[8] ^= 1
    bits[9] ^= 1  # two errors: C_Sigma 0, syndrome 3 ^ 5 = 6
    assert M.crc_test(bits) == (False, -1)
    bits = list(clean)
    for b in (8, 9, 84):  # three errors, C_Sigma 1, parity over 8..84 odd: syndrome 3 ^ 5 ^ 84 = 82, "corrects" a fourth bit
        bits[b] ^= 1
    assert M.SYNDROME_OF[84] == 84 and M.crc_test(bits) == (True, M.LOCATOR[82])
    bits = list(clean)
    for b in (0, 10, 84):  # syndrome 1 ^ 6 ^ 84 = 83... with one check bit among the three the parity over 8..84 is even: rejected
        bits[b] ^= 1
    assert M.crc_test(bits) == (False, -1)
    big = [b for b in range(8, 85) if M.SYNDROME_OF[b] ^ M.SYNDROME_OF[84] ^ M.SYNDROME_OF[83] >= 85][0]
    bits = list(clean)
    for b in (big, 83, 84):
        bits[b] ^= 1
    assert M.crc_test(bits) == (False, -1)  # syndrome >= 85
    assert [M.LOCATOR[1 << k] for k in range(7)] == list(range(7)) and M.LOCATOR[0] == 0 and M.LOCATOR[3] == 8 and M.LOCATOR[84] == 84


def test_the_filling_ring_and_state_1():
    """A stream whose first 300 symbols are a time mark: a hit on symbol 300 and on every symbol to 2000, because the
    correlation runs over the first 300 symbols until the ring is full (state 1 from 300; the later hits are less than 2000
    after it and change nothing).  The next mark is seen at 4000, more than 2000 after 300: back to state 0, the hit thrown
    away.  Then 6000 gives state 1 and 8000, exactly 2000 later, state 2; the first decode is at 10 000."""
    rng = np.random.default_rng(8)
    x = M.stream(M.frame_strings(rng=rng, ids=(1, 2, 3, 4, 5)), lead=0)
    m = M.Decoder()
    for end, want in ((299, (0, 0)), (300, (1, 300)), (2000, (1, 300)), (3999, (1, 300)), (4000, (0, 300)), (5999, (0, 300)), (6000, (1, 6000)),
                      (7999, (1, 6000)), (8000, (2, 8000)), (9999, (2, 8000))):
        recs, _, _ = m.run(x[m.counter:end])
        assert (m.stat, m.preamble_index) == want and not recs, end
    recs, _, sf = m.run(x[9999:10001])
    assert len(recs) == 1 and recs[0]["symbol_counter"] == 10000 and recs[0]["string_id"] == 5 and sf.tolist() == [M.S_STRING, 0]
    # a hit before 2000 in state 1 changes nothing: a second mark 1000 symbols after the first
    y = np.concatenate([M.stream([], lead=7), np.ones(700, np.float32), M.MARK_SYMBOLS.astype(np.float32), np.ones(3000, np.float32)])
    m = M.Decoder()
    m.run(y[:2307])
    assert (m.stat, m.preamble_index) == (1, 2007)   # the first mark, seen when it is the oldest
    m.run(y[2307:3307])
    assert (m.stat, m.preamble_index) == (1, 2007)   # the second, 1000 later: nothing
    m.run(y[3307:])
    assert (m.stat, m.preamble_index) == (1, 2007)   # and state 1 never times out


def test_state_2_decodes_whatever_the_correlation(primed):
    """In state 2 a time mark that is more than half wrong is no hit and has corr <= 0: the string is decoded all the same,
    under the inverted polarity.  The relative code makes the data bits the same under both polarities (every relative bit
    is complemented, their XORs are not), so the string still passes its check and sets the time of week."""
    template, rest, chars = primed
    m = copy.deepcopy(template)
    m.hist = m.hist.copy()
    m.hist[1:161] = -m.hist[1:161]  # the window at the decode is entries 1..300 of the history now
    recs, tow, sf = m.run(rest[:1])
    assert len(recs) == 1 and recs[0]["flags"] & (M.INVERTED | M.CRC_OK | M.NEW_TOW | M.CORRECTED) == M.INVERTED | M.CRC_OK | M.NEW_TOW
    assert sf[0] == M.S_STRING | M.S_INVERTED | M.S_VALID_WORD and recs[0]["bits"] == M.pack_bits([chars[84 - i] for i in range(85)])
    assert m.stat == 2 and m.preamble_index == m.counter and m.crc_error_counter == 0 and m.nav.tow_set
    m = copy.deepcopy(template)
    m.hist = m.hist.copy()
    m.hist[1:151] = -m.hist[1:151]  # corr exactly 0: inverted as well
    recs, _, _ = m.run(rest[:1])
    assert recs[0]["flags"] & M.INVERTED
    m = copy.deepcopy(template)
    m.hist = m.hist.copy()
    m.hist[1:150] = -m.hist[1:150]  # corr +2: no hit, normal polarity, a good string
    recs, _, sf = m.run(rest[:1])
    assert recs[0]["flags"] & (M.INVERTED | M.CRC_OK | M.NEW_TOW) == M.CRC_OK | M.NEW_TOW and sf[0] == M.S_STRING | M.S_VALID_WORD


def test_seven_bad_strings_in_a_row(primed):
    """Six bad strings count; the seventh drops frame sync and returns to state 0 with the counter at 7; a good string in
    between zeroes the counter.  valid_word needs frame sync and the TOW flag."""
    template, rest, chars = primed
    m = copy.deepcopy(template)
    recs, _, sf = m.run(rest[:1])
    assert recs[0]["flags"] & M.CRC_OK and m.frame_sync and sf[0] & M.S_VALID_WORD
    bad = list(chars)
    bad[20] ^= 1
    bad[33] ^= 1  # two information bits: C_Sigma 0 with a syndrome, rejected
    noise = M.stream([bad] * 7)
    recs, _, sf = m.run(noise[:7 * 2000])
    assert len(recs) == 7 and not any(r["flags"] & M.CRC_OK for r in recs)
    assert (sf[:6 * 2000 + 1999] & M.S_VALID_WORD).all() and not sf[-1] & M.S_VALID_WORD
    assert m.stat == 0 and not m.frame_sync and m.crc_error_counter == 7 and m.nav.tow_set
    m = copy.deepcopy(template)
    m.run(rest[:1])
    m.run(noise[:7 * 2000 - 1])  # one symbol before the seventh
    assert m.crc_error_counter == 6 and m.stat == 2
    good, last = with_string(m, chars)
    good.run([last])
    assert good.crc_error_counter == 0 and good.stat == 2 and good.frame_sync


def test_nav_chain_and_tb():
    """Strings 2..5 are read only behind the string before; t_b == 0 never clears the flags; a t_b change does."""
    rng = np.random.default_rng(6)
    nav = M.NavMessage()
    for ch in M.frame_strings(rng=rng, ids=(2, 3, 4, 5)):
        nav.string_decoder(ch)
    assert nav.e == [False] * 4 and not nav.tow_set and not nav.utc5
    nav = M.NavMessage()
    for ch in M.frame_strings(t_b_raw=0, rng=rng):
        nav.string_decoder(ch)
        new_eph = nav.have_new_ephemeris()
        nav.have_new_utc_model()
    assert not new_eph and nav.e == [True] * 4 and nav.tow_set
    for t_b, want in ((5, True), (5, False), (6, True)):
        for ch in M.frame_strings(t_b_raw=t_b, rng=rng):
            nav.string_decoder(ch)
            new_eph = nav.have_new_ephemeris()
            nav.have_new_utc_model()
        assert new_eph == want and nav.e == ([False] * 4 if want else [True] * 4)


def test_stamp_slices(primed):
    """d_TOW over all 4096 raw t_k (N_T 500, N_4 6), all 2048 N_T (t_k 02:59:20, which rolls the date back) and all 32 N_4
    (N_T 60 and 1461: both sides of 29 February 2100), each with random signed tau_c and tau_gps — not the full product —
    against plain day counting; then the block's stamp on 400 of them through a decode: floor((d_TOW - 0.3) * 1000) / 1000,
    round(x * 1000) and + 0.001 on the symbols after it, in doubles."""
    template, rest, _ = primed
    rng = np.random.default_rng(5)
    t_k_of = lambda raw: (raw >> 7) * 3600 + ((raw >> 1) & 63) * 60 + (raw & 1) * 30
    specs = [(raw, 500, 6) for raw in range(4096)] + [((2 << 7) | (59 << 1), n_t, 6) for n_t in range(2048)]
    specs += [(100, n_t, n_4) for n_4 in range(32) for n_t in (60, 1461)]
    for raw, n_t, n_4 in specs:
        tc, tg = int(rng.integers(-2 ** 31 + 1, 2 ** 31)), int(rng.integers(-2 ** 21 + 1, 2 ** 21))
        wn, tow = M.glot_to_gpst(n_4, n_t, t_k_of(raw) + 10, tc * 2.0 ** -31, tg * 2.0 ** -30)
        assert tow == float(whole_tow(n_4, n_t, t_k_of(raw))) + (tc * 2.0 ** -31 + tg * 2.0 ** -30), (raw, n_t, n_4)
        assert 17 <= whole_tow(n_4, n_t, t_k_of(raw)) < 604800
    for k in rng.choice(len(specs), 400, replace=False):
        raw, n_t, n_4 = specs[k]
        tc, tg = int(rng.integers(-2 ** 31 + 1, 2 ** 31)), int(rng.integers(-2 ** 21 + 1, 2 ** 21))
        m, last = with_string(template, M.frame_strings(n_4=n_4, tau_c=tc, tau_gps=tg, rng=rng, ids=(5,))[0])
        m.nav.t_k, m.nav.n_t = t_k_of(raw), n_t
        recs, tow_ms, sf = m.run(np.concatenate([[last], rest[1:4]]))
        tow = float(whole_tow(n_4, n_t, t_k_of(raw))) + (tc * 2.0 ** -31 + tg * 2.0 ** -30)
        assert recs[0]["flags"] & M.NEW_TOW and recs[0]["tow"] == tow
        x = float(np.floor((tow - 0.3) * 1000) / 1000)
        want = []
        for _ in range(4):
            want.append(M.round_half_away(x * 1000.0) & 0xFFFFFFFF)
            x = x + 0.001
        assert tow_ms.tolist() == want and (sf & M.S_VALID_WORD).all()
    assert M.round_half_away(-550.0) & 0xFFFFFFFF == 2 ** 32 - 550 and M.round_half_away(2.5) == 3 and M.round_half_away(-2.5) == -3


def test_decode_string_sums_in_order_and_zero_sums():
    """A half-bit is `sum > 0` of ten doubles added in order from 0.0: 3e30 + 1 - 3e30 - 0.5 is -0.5 in order (0.5 exactly);
    a sum that cancels to 0 and a NaN sum are '0' under both polarities."""
    d = M.Decoder()
    sym = np.tile(np.array([-1.0] * 10 + [1.0] * 10), 85)  # all pairs "01": relative 0, data 0
    assert d.decode_string(sym) == [0] * 85
    sym[10:20] = -1.0                                       # the first pair is now "?0": data bit 1 is the first half-bit
    sym[0:10] = [3e30, 1, -3e30, 1, 0, 0, 0, 0, 0, 0]       # in order: 1
    assert d.decode_string(sym)[:3] == [0, 1, 0]
    sym[0:10] = [3e30, 1, -3e30, -0.5, 0, 0, 0, 0, 0, 0]    # in order: -0.5, although the exact sum is positive
    assert d.decode_string(sym)[:3] == [0, 0, 0]
    for zero in ([0.75, -0.75] * 5, [np.nan] + [1.0] * 9, [0.0, -0.0] * 5):
        sym[0:10] = zero                                    # '0' under both polarities: "00", and negated "01"
        assert d.decode_string(sym)[:3] == [0, 0, 0] and d.decode_string(-sym)[:3] == [0, 1, 0]
