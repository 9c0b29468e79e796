"""tests/dnav_model.py against the reference's Beidou_Dnav_Navigation_Message (tests/golden/dnav_ref.npz, written by
tests/golden/make_dnav_golden.py), its BCH decoder against the ICD encoder of its transmitter, and the sync timing of the
restated blocks.  No GPU."""
from __future__ import annotations

import hashlib
import os

import numpy as np
import pytest

import dnav_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dnav_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("d2", [0, 1])
def test_model_equals_reference_navigation_message(golden, d2):
    nav = M.NavMessage()
    n = golden["bits"].shape[1]
    assert n == 64
    seen_ids, seen_flags = set(), set()
    for k in range(n):
        bits = np.unpackbits(golden["bits"][d2, k])[:300].tolist()
        fra_id = nav.d2_subframe_decoder(bits) if d2 else nav.d1_subframe_decoder(bits)
        assert fra_id == golden["ids"][d2, k]
        assert float(nav.sow) == golden["sows"][d2, k]
        assert int(nav.crc) == golden["crc"][d2, k] == 1
        assert int(nav.new_sow) == golden["new_sow"][d2, k]
        seen_ids.add(fra_id)
        seen_flags.add(int(nav.new_sow))
        nav.new_sow = False  # as the block does
    assert seen_ids == set(range(8)) and seen_flags == {0, 1}
    assert 0.0 in golden["sows"][d2] and float((1 << 20) - 1) in golden["sows"][d2]


def test_transmitter_restores_what_it_was_given(golden):
    # the plain bits of build_subframe read back as the fields they were built from, under both layouts
    rng = np.random.default_rng(5)
    for d2 in (False, True):
        plain, air = M.build_subframe(d2, 5, 9, 0xABCDE, rng.integers(0, 2, 182))
        assert len(plain) == len(air) == 300
        assert M.read_unsigned(plain, [(16, 3)]) == 5
        assert M.read_unsigned(plain, [(19, 8), (31, 12)]) == 0xABCDE
        assert M.read_unsigned(plain, [(43, 4)] if d2 else [(44, 7)]) == 9
        dec = M.Decoder(M.B1I, 3 if d2 else 20)
        dec.history.extend(M.symbols_of(air).tolist() + [1.0] * 11)
        rec = dec._decode(11, False, 0)
        assert rec["words"] == [M.read_unsigned(plain, [(30 * w + 1, 30)]) for w in range(10)] and rec["corrected_mask"] == 0


def pm(bits):
    return [1 if b else -1 for b in bits]


def test_bch_identity_on_codewords_and_all_single_errors():
    for complemented in (False, True):
        for v in range(2048):
            cw = M.bch_encode(M.int_bits(v, 11))
            sent = pm([1 - b for b in cw]) if complemented else pm(cw)
            dec, err = M.decode_bch15_11_01(sent)
            assert dec == sent and err == 0
            for k in range(15):
                got = list(sent)
                got[k] *= -1
                dec, err = M.decode_bch15_11_01(got)
                assert dec == sent and err != 0


def test_bch_on_every_input_is_pinned():
    h = hashlib.sha256()
    touched = 0
    for w in range(1 << 15):
        dec, err = M.decode_bch15_11_01(pm(M.int_bits(w, 15)))
        out = sum((1 if b > 0 else 0) << (14 - i) for i, b in enumerate(dec))
        h.update(out.to_bytes(2, "little") + bytes([err]))
        touched += err != 0
    assert touched == 32768 - 2048  # a perfect code: every word is a codeword or one bit from one
    assert h.hexdigest() == BCH_DIGEST


BCH_DIGEST = "8387856558f278e0ef3db5ceafc3ab6d1e6c5dbcdd58f161ef5e4e454ab91426"


def d1_stream(lead, n_sub, sow0, inverted=False, seed=1):
    rng = np.random.default_rng(seed)
    subs = [M.build_subframe(False, 1 + k % 5, 0, sow0 + 6 * k, rng.integers(0, 2, 182))[1] for k in range(n_sub)]
    return np.concatenate([np.ones(lead, np.float32), M.stream(subs, inverted=inverted), np.ones(11, np.float32)])


def d2_stream(lead, n_sub, sow0, inverted=False, seed=1):
    # FraID 1 every fifth subframe, 3 s apart; subframe 1 (the first one decoded) is a FraID 1 page
    rng = np.random.default_rng(seed)
    subs = [M.build_subframe(True, 1 + (k + 4) % 5, 1 + k % 10, sow0 + 3 * ((k + 4) // 5), rng.integers(0, 2, 182))[1] for k in range(n_sub)]
    return np.concatenate([np.ones(lead, np.float32), M.stream(subs, inverted=inverted), np.ones(11, np.float32)])


@pytest.mark.parametrize("signal", [M.B1I, M.B3I])
@pytest.mark.parametrize("lead", [0, 37])
@pytest.mark.parametrize("prn,d", [(20, 20), (3, 2)])
def test_sync_timing_on_a_clean_stream(signal, lead, prn, d):
    sow0 = 345600
    s = (d2_stream if d == 2 else d1_stream)(lead, 4, sow0)
    dec = M.Decoder(signal, prn)
    first_hit, recs, tows = None, [], {}
    for i, x in enumerate(s.tolist()):
        before = dec.stat
        tow, sf, rec = dec.work(x)
        if before == 0 and dec.stat == 1 and first_hit is None:
            first_hit = dec.symbol_counter
        if rec is not None:
            recs.append(rec)
            tows[rec["symbol_counter"]] = tow
    assert first_hit == 311 + lead
    assert [r["symbol_counter"] for r in recs] == [611 + lead, 911 + lead, 1211 + lead]
    assert recs[0]["flags"] & M.F_STATE1 and not recs[1]["flags"] & M.F_STATE1
    sow1 = sow0 + (3 if d == 2 else 6)  # the SOW of subframe 1, the first one decoded
    assert recs[0]["sow"] == sow1
    assert tows[611 + lead] == (sow1 + 14) * 1000 + 311 * d
    assert dec.valid_word and dec.stat == 2
    # the clock then runs by d per symbol and every later stamp agrees with it
    assert dec.tow_at_current_symbol_ms == (sow1 + 14) * 1000 + 311 * d + d * (len(s) - 611 - lead)
    assert not any(r["flags"] & (M.F_TOW_ZEROED | M.F_INVERTED) for r in recs)


def plant(s, at):
    """A look-alike preamble whose first symbol is s[at]."""
    s = s.copy()
    s[at:at + 11] = np.array(M.PREAMBLE, np.float32)
    return s


def test_look_alike_before_the_true_preamble_diff_below_300_is_ignored():
    # look-alike at 5, true preambles at 100, 400, 700: in state 1 since 316, the hits at 411 (diff 95) and 711 (diff 395)
    s = plant(d1_stream(100, 3, 1000), 5)
    dec = M.Decoder(M.B1I, 20)
    stats = []
    for x in s.tolist():
        dec.work(x)
        stats.append(dec.stat)
    assert stats[316 - 2] == 0 and stats[316 - 1] == 1
    assert set(stats[316 - 1:711 - 1]) == {1}    # 411, diff 95 < 300: nothing happens
    assert set(stats[711 - 1:1011 - 1]) == {0}   # 711, diff 395 > 300: state 0, and the hit is thrown away
    assert len(s) == 1011 and stats[-1] == 1 and dec.preamble_index == 1011  # the last preamble is a state-0 hit again


def test_look_alike_then_true_preamble_diff_above_300_drops_the_hit():
    # look-alike at 0 (hit at 311), true preambles at 320, 620, 920: 631 has diff 320 > 300 → state 0, hit dropped;
    # 931 is then a state-0 hit and 1231, the stream's last symbol, the first decode — 300 symbols later than without
    # the look-alike
    s = plant(d1_stream(320, 3, 1000), 0)
    dec = M.Decoder(M.B1I, 20)
    stats, recs = [], []
    for x in s.tolist():
        recs.append(dec.work(x)[2])
        stats.append(dec.stat)
    assert stats[311 - 1] == 1 and stats[631 - 2] == 1 and stats[631 - 1] == 0
    assert stats[931 - 2] == 0 and stats[931 - 1] == 1 and stats[1231 - 2] == 1
    assert len(s) == 1231 and [k + 1 for k, r in enumerate(recs) if r is not None] == [1231] and dec.preamble_index == 1231


def test_b3i_prn_above_58_takes_the_d1_decoder_with_d2_timing():
    assert M.is_d2_decoder(M.B1I, 60) and M.is_d2_timing(60)
    assert not M.is_d2_decoder(M.B3I, 60)
    assert M.Decoder(M.B3I, 60).symbol_duration_ms == 2 and M.Decoder(M.B3I, 20).symbol_duration_ms == 20
    assert M.is_d2_decoder(M.B3I, 5) and not M.is_d2_decoder(M.B3I, 6) and not M.is_d2_decoder(M.B1I, 58)


def test_state2_subframe_with_a_broken_preamble_is_decoded_inverted():
    s = d1_stream(0, 3, 2000)
    s[600:606] = -s[600:606]  # six of the eleven symbols of subframe 2's preamble wrong: corr -1 at counter 911
    dec = M.Decoder(M.B1I, 20)
    recs = [r for r in (dec.work(x)[2] for x in s.tolist()) if r is not None]
    assert [r["symbol_counter"] for r in recs] == [611, 911]
    assert not recs[0]["flags"] & M.F_INVERTED and recs[1]["flags"] & M.F_INVERTED


def test_record_bound():
    assert M.subframes_per_run(601) == 3 and M.subframes_per_run(299) == 1
