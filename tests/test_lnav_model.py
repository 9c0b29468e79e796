"""tests/lnav_model.py against itself and the ICD: the transmitter's parities are the six equations of IS-GPS-200
Table 20-XIV as XOR lists, the checker is the block's rotate-and-mask form (gps_l1_ca_telemetry_decoder_gs.cc:191-214),
two independent derivations; then every property of the block that a clean-room LNAV decoder would not have, each
pinned by a case built to hit it (the GPU tests run the same cases on the device)."""
import os

import numpy as np
import pytest

import lnav_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lnav_ref.npz")


def test_icd_encoder_passes_the_mask_checker():
    rng = np.random.default_rng(1)
    for d29s in (0, 1):
        for d30s in (0, 1):
            for _ in range(500):
                w = M.encode_word(rng.integers(0, 2, 24), d29s, d30s)
                assert M.parity_check(M.stored_word(w, d29s, d30s))
            w = M.encode_word(rng.integers(0, 2, 24), d29s, d30s, solve=True)
            assert w[28:] == [0, 0] and M.parity_check(M.stored_word(w, d29s, d30s))


def test_any_single_flipped_bit_fails():
    rng = np.random.default_rng(2)
    for d29s, d30s in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for _ in range(20):
            w = M.encode_word(rng.integers(0, 2, 24), d29s, d30s)
            for k in range(30):
                bad = list(w)
                bad[k] ^= 1
                assert not M.parity_check(M.stored_word(bad, d29s, d30s)), (d29s, d30s, k)


def test_built_subframe_fields():
    rng = np.random.default_rng(3)
    bits, words = M.build_subframe(3, 0x1ABCD, rng.integers(0, 2, 208))
    assert bits.shape == (300,) and "".join(map(str, bits[:8])) == M.PREAMBLE
    assert all(M.parity_check(w) for w in words)
    assert (words[1] >> 8) & 7 == 3 and (words[1] >> 13) & 0x1FFFF == 0x1ABCD
    assert words[1] & 3 == 0 and words[9] & 3 == 0  # D29 = D30 = 0: the next word starts from zeros


def tracked(bits_list, n, sign=1.0):
    """What a tracker that aligned on the first preamble hands over: the stream from the symbol after it."""
    return np.float32(sign) * M.build_stream(bits_list, n + 8, 0)[8:]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_seeding_decodes_the_first_subframe_at_300(sign):
    bits, words = M.five_subframes(5)
    m = M.LnavDecoder()
    flags = np.full(700, sign < 0)
    recs, fault, tow, sf = m.run(tracked(bits, 700, sign), flags180=flags)
    assert [r["symbol_counter"] for r in recs] == [300, 600] and not fault
    assert all(r["flags"] & M.F_OK for r in recs) and recs[0]["words"] == words[0] and recs[1]["words"] == words[1]
    assert all(bool(r["flags"] & M.F_PLL_180) == (sign < 0) for r in recs)
    assert not recs[0]["flags"] & M.F_STATE1 and recs[1]["flags"] & M.F_STATE1
    # without the flag the seeded preamble has the wrong sign and the first subframe is lost
    recs, _, _, _ = M.LnavDecoder().run(tracked(bits, 700, sign), flags180=np.full(700, sign > 0))
    assert [r["symbol_counter"] for r in recs] == [600]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_behind_a_lead_in(sign):
    bits, _ = M.five_subframes(5)
    m = M.LnavDecoder()
    recs, _, tow, sf = m.run(np.float32(sign) * M.build_stream(bits, 1000, 37, 1))
    assert [r["symbol_counter"] for r in recs] == [345, 645, 945]
    assert [r["tow_s"] for r in recs] == [6000, 6006, 6012]
    # +20 ms per symbol from the stamp; silent before it
    k = 345 - 8 - 1  # the run's index of the symbol at counter 345
    assert not (sf[:k] & M.S_OUTPUT).any() and sf[k] == (M.S_OUTPUT | M.S_SUBFRAME | (M.S_PLL_180 if sign < 0 else 0))
    assert tow[k] == 6000000 and np.array_equal(tow[k:k + 300], 6000000 + 20 * np.arange(300))
    assert tow[k + 300] == 6006000 and (sf[k:] & M.S_OUTPUT).all()


def test_reset_seeds_again():
    bits, _ = M.five_subframes(5)
    x = tracked(bits, 1500)
    m = M.LnavDecoder()
    m.run(x[:450])
    m.crc_error_counter = 1
    before = m.state()
    m.reset()
    st = m.state()
    assert st["history_size"] == 0 and st["stat"] == 0 and st["tow_set"] == 0 and st["last_valid_preamble"] == 458
    for f in ("crc_error_counter", "frame_sync", "pll_180", "prev_word", "symbol_counter", "nav_tow_s", "tow_at_current_symbol_ms"):
        assert st[f] == before[f]
    # the tracker aligns again: the next symbol is the one after the third subframe's preamble
    recs, _, _, _ = m.run(x[600:1200])
    assert m.symbol_counter == 458 + 8 + 600 and [r["symbol_counter"] for r in recs] == [458 + 300, 458 + 600]


def test_failed_state0_attempt_changes_the_180_flag():
    rng = np.random.default_rng(7)
    x = np.where(rng.integers(0, 2, 400) > 0, 1.0, -1.0).astype(np.float32)
    x[100:108] = -M.symbols_of([int(c) for c in M.PREAMBLE])  # an inverted preamble, oldest at counter 8 + 100 + 300
    m = M.LnavDecoder()
    m.run(x[:399])
    tried = m.subframes_tried
    m.pll_180 = False
    recs, _, _, _ = m.run(x[399:400])
    assert m.symbol_counter == 408 and m.subframes_tried == tried + 1 and not recs
    assert m.pll_180 and m.stat == 0 and m.preamble_index == 408 and m.prev_word != 0


def corrupted_word10():
    """Subframe 2's word 10 with its last two bits inverted: its parity fails, and D29* / D30* as stored become 1, 1."""
    bits, words = M.five_subframes(5)
    bad = [b.copy() for b in bits]
    bad[1][298:300] ^= 1
    return bad, words


def test_previous_word_cleared_in_state0_and_carried_in_state1():
    bad, _ = corrupted_word10()
    m = M.LnavDecoder()
    recs, _, _, _ = m.run(tracked(bad, 1300))
    assert [r["symbol_counter"] for r in recs] == [300, 600, 900, 1200]
    assert [r["parity_fail_mask"] for r in recs] == [0, 1 << 9, 1 << 0, 0]  # the clean third subframe fails in its word 1
    assert [r["crc_error_counter"] for r in recs] == [0, 1, 2, 0]
    # the same third subframe found in state 0 decodes: there the previous word is cleared
    m0 = M.LnavDecoder()
    recs0, _, _, _ = m0.run(tracked(bad, 1300)[600:])
    assert recs0[0]["symbol_counter"] == 300 and recs0[0]["flags"] & M.F_OK and recs0[0]["subframe_id"] == 3


def lose_and_regain():
    """Subframes 2, 3, 4 each with one data bit flipped (word 5), then clean."""
    bits, _ = M.five_subframes(5)
    bad = [b.copy() for b in bits]
    for k in (1, 2, 3):
        bad[k][4 * 30 + 7] ^= 1
    return bad


def test_sync_is_lost_at_the_third_failure():
    m = M.LnavDecoder()
    recs, _, tow, sf = m.run(tracked(lose_and_regain(), 2200))
    at = {r["symbol_counter"]: r for r in recs}
    assert [r["crc_error_counter"] for r in recs[:4]] == [0, 1, 2, 0]
    assert not at[900]["flags"] & M.F_SYNC_LOST and at[900]["flags"] & M.F_FRAME_SYNC
    assert at[1200]["flags"] & M.F_SYNC_LOST and not at[1200]["flags"] & M.F_FRAME_SYNC
    # in state 0 the stream is silent, until the next subframe is found there
    later = [r for r in recs if r["symbol_counter"] > 1200]
    assert later and later[0]["symbol_counter"] == 1500 and not later[0]["flags"] & M.F_STATE1 and later[0]["flags"] & M.F_OK
    assert not (sf[1200 - 9:1500 - 9] & M.S_OUTPUT).any() and (tow[1200 - 9:1500 - 9] == 0).all()
    assert sf[1500 - 9] & M.S_OUTPUT and tow[1500 - 9] == 1000 * later[0]["tow_s"]


def test_id0_with_good_parity_is_a_failure_and_leaves_the_tow():
    rng = np.random.default_rng(9)
    subs = [M.build_subframe(sid, 500 + k, rng.integers(0, 2, 208))[0] for k, sid in enumerate((1, 0, 7, 6, 2))]
    m = M.LnavDecoder()
    recs, _, tow, _ = m.run(tracked(subs, 1600))
    assert [r["subframe_id"] for r in recs[:2]] == [1, 0]
    assert recs[1]["flags"] & M.F_PARITY_OK and not recs[1]["flags"] & M.F_OK and recs[1]["tow_s"] == 3000 and recs[1]["crc_error_counter"] == 1
    assert recs[2]["subframe_id"] == 7 and recs[2]["crc_error_counter"] == 2 and recs[3]["flags"] & M.F_SYNC_LOST
    assert tow[599 - 8] == 3000000 + 20 * 300  # the failure still adds its 20 ms


def tow0_case():
    rng = np.random.default_rng(11)
    return [M.build_subframe(sid, t, rng.integers(0, 2, 208))[0] for sid, t in ((1, 100800 - 1), (2, 0), (3, 1))]


def test_tow0_subframe_leaves_a_stale_stamp():
    m = M.LnavDecoder()
    recs, _, tow, sf = m.run(tracked(tow0_case(), 950))
    assert [r["tow_s"] for r in recs] == [604794, 0, 6] and all(r["flags"] & M.F_OK for r in recs)
    k = 600 - 9
    assert tow[k - 1] == 604794000 + 20 * 299 and tow[k] == tow[k - 1] and tow[k + 1] == tow[k] + 20  # no stamp, no increment
    assert sf[k] == (M.S_OUTPUT | M.S_SUBFRAME)
    # found in state 0 the same subframe outputs nothing
    m0 = M.LnavDecoder()
    recs0, _, _, sf0 = m0.run(tracked(tow0_case(), 950)[300:])
    assert recs0[0]["tow_s"] == 0 and recs0[0]["flags"] & M.F_OK and sf0[300 - 9] == M.S_SUBFRAME and not (sf0[:600 - 9] & M.S_OUTPUT).any()


def test_fault_fires_once_and_again_only_after_reset():
    m = M.LnavDecoder()
    ones = np.ones(6000, np.float32)
    assert not m.run(ones[:6000 - 8])[1]  # the seeding counts
    assert m.run(ones[:1])[1]
    assert not m.run(ones)[1] and not m.run(ones)[1]
    m.set_satellite()
    assert not m.run(ones)[1]
    m.reset()
    assert not m.run(ones[:6000 - 8])[1]
    assert m.run(ones[:1])[1]


def test_zeros_and_nans_are_zero_bits():
    bits, words = M.five_subframes(5)
    for sign in (1.0, -1.0):
        x = tracked(bits, 700, sign)
        clean = M.LnavDecoder().run(x, flags180=np.full(700, sign < 0))[0]
        y = x.copy()
        zero_bits = np.nonzero(np.concatenate(bits)[8:708] == 0)[0]
        y[zero_bits[0::3]] = 0.0
        y[zero_bits[1::3]] = -0.0
        y[zero_bits[2::3]] = np.nan
        got = M.LnavDecoder().run(y, flags180=np.full(700, sign < 0))[0]
        assert [r["words"] for r in got] == [r["words"] for r in clean] and len(got) == 2
        z = x.copy()
        one_bits = np.nonzero(np.concatenate(bits)[8:708] == 1)[0]
        z[one_bits[5]] = np.nan  # a one turned into a NaN is a zero bit: the parity fails
        assert len(M.LnavDecoder().run(z[:300], flags180=np.full(300, sign < 0))[0]) == 0
    # in the correlation a NaN counts as positive: the preamble's first symbol ('1') as a NaN is still a hit, and then a 0 bit
    x = tracked(bits, 700)
    x[292] = np.nan
    m = M.LnavDecoder()
    recs = m.run(x[250:592])[0]  # a new object from mid-subframe: the second subframe's preamble is the oldest at counter 350
    assert not recs and m.symbol_counter == m.preamble_index == 350 and m.prev_word == words[1][9] and m.stat == 0
    assert M._code(np.nan) == 0 and M._code(-0.0) == 0 and M._code(0.0) == 0 and M._code(-1e-45) == 2


def test_noise_decodes_nothing():
    rng = np.random.default_rng(13)
    m = M.LnavDecoder()
    recs, fault, _, sf = m.run(rng.standard_normal(20000))
    assert not recs and fault and m.subframes_tried >= 100 and not (sf & M.S_OUTPUT).any()


def densest_stream(n_cycles: int) -> np.ndarray:
    """A stream whose records are as dense as the block allows, as a tracker hands it over: a good subframe, then 601
    random symbols, and again.  The good one decodes; the windows due 300, 600 and 900 symbols later fail, the third with
    loss of sync; the window one symbol after that is the next good subframe, found in state 0.  Records at counters 300,
    600, 900, 1200, 1201, 1501, 1801, 2101, 2102, ..."""
    bits, _ = M.five_subframes(5)
    rng = np.random.default_rng(17)
    cycle = np.concatenate([M.symbols_of(bits[0]), np.where(rng.integers(0, 2, 601) > 0, 1.0, -1.0).astype(np.float32)])
    return np.concatenate([cycle] * n_cycles)[8:]


def test_subframes_per_run_bound():
    assert M.subframes_per_run(899) == 899 // 300 + 2 and M.subframes_per_run(903) == 6
    x = densest_stream(4)
    m = M.LnavDecoder()
    recs, _, _, _ = m.run(x[:1199 - 8])
    assert [r["symbol_counter"] for r in recs] == [300, 600, 900] and m.crc_error_counter == 2
    n = 903 + 901
    recs, _, _, _ = m.run(x[1199 - 8:1199 - 8 + n])  # run() itself asserts the bound; the first symbol is the loss
    assert [r["symbol_counter"] - 1199 for r in recs] == [1, 2, 302, 602, 902, 903, 1203, 1503, 1803, 1804]
    assert len(recs) == M.subframes_per_run(n) == 10 > n // 300 + 2
    # the counting argument on those record times for every run length
    for n in range(1, 6000, 7):
        times, t = [], 1
        while t <= n:
            times += [u for u in (t, t + 1, t + 301, t + 601) if u <= n]
            t += 901
        assert len(times) <= M.subframes_per_run(n), n


def test_reference_fixture():
    """tests/golden/lnav_ref.npz: the reference's Gps_Navigation_Message::subframe_decoder on 64 built subframes given to one
    object in turn (tests/golden/make_lnav_golden.py): the returned ID and get_TOW() after each call, against the model's
    decode_subframe fed the same subframes as symbols — the ID bits, the TOW for IDs 1..5, the TOW left alone otherwise."""
    g = np.load(GOLD)
    ids, tows = g["ids"].tolist(), g["tows"].tolist()
    assert len(ids) == 64 and {0, 6, 7} <= set(ids) and 0 in tows
    m = M.LnavDecoder()
    for sub, sid, tow in zip(g["subframes"], ids, tows):
        words = [int(w) for w in np.frombuffer(sub.tobytes(), "<u4")]
        sent = []
        for w in words:  # the transmitted bits: D1..D24 carry the data bits XOR D30*
            d30s = (w >> 30) & 1
            sent += [((w >> (29 - k)) & 1) ^ (d30s if k < 24 else 0) for k in range(30)]
        m.hist.clear()
        m.hist.extend(M._code(v) for v in M.symbols_of(sent))
        m.prev_word = 0
        ok, got, fail, got_id = m._decode(False)
        assert got == words and fail == 0 and got_id == sid and ok == (1 <= sid <= 5)
        assert m.nav_tow_s == tow
