"""tests/cnav_model.py against the reference's libswiftcnav as recorded in tests/golden/cnav_ref.npz (every stored quantity,
exactly), the branches the golden inputs reach, and the block level of gps_l2c_telemetry_decoder_gs /
gps_l5_telemetry_decoder_gs: the TOW stamps, the L5 TOW-consistency branch, the out_valid drop, both watchdogs at their
exact symbol and both resets.  The GPU tests run the device against this model."""
import os

import numpy as np
import pytest

import cnav_model as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnav_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def golden_runs(gold):
    """Every golden stream through the model's Decoder once: name -> (decoder, events, raws, snapshots)."""
    runs = {}
    for name, (bits, bias) in M.golden_streams().items():
        d = M.Decoder()
        if bias:
            d.add_metrics(bias)
        ev, raws, snaps = [], [], []
        for k, b in enumerate(bits):
            res, rec = d.add_symbol(255 if b else 0)
            if res:
                ev.append([k, rec["delay"], rec["tow"], rec["msg_id"], rec["prn"], rec["alert"]])
                raws.append(np.frombuffer(rec["raw"], np.uint8))
            if (k + 1) % 64 == 0 or k + 1 == len(bits):
                snaps.append([k + 1] + d.part1.scalars() + d.part2.scalars())
        runs[name] = (d, ev, raws, snaps)
    return runs


def test_streams_are_the_stored_ones(gold):
    streams = M.golden_streams()
    assert {k[:-4] for k in gold.files if k.endswith("_sym")} == set(streams)
    for name, (bits, bias) in streams.items():
        n = int(gold[name + "_n"])
        assert n == len(bits) and int(gold[name + "_bias"]) == bias
        assert np.array_equal(np.unpackbits(gold[name + "_sym"])[:n], bits)


def test_model_equals_the_reference(gold, golden_runs):
    for name, (d, ev, raws, snaps) in golden_runs.items():
        assert np.array_equal(np.array(ev, np.int32).reshape(-1, 6), gold[name + "_ev"]), name
        assert np.array_equal(np.array(raws, np.uint8).reshape(-1, 64), gold[name + "_raw"]), name
        assert np.array_equal(np.array(snaps, np.int32), gold[name + "_snap"]), name
        for k, p in enumerate(d.parts):
            assert np.array_equal(np.stack(p.metrics), gold[name + "_metrics"][k]), name
            assert np.array_equal(p.decisions, gold[name + "_decisions"][k]), name
            assert bytes(p.symbols) == gold[name + "_symbols"][k].tobytes(), name
            assert bytes(p.decoded) == gold[name + "_decoded"][k].tobytes(), name


def test_the_expected_messages_come_out(gold):
    assert gold["lead0_pos_ev"][:, 0].tolist() == [703, 1279, 1919] and gold["lead1_pos_ev"][:, 0].tolist() == [702, 1278, 1918]
    for name in ("lead0_pos", "lead0_neg", "lead37_pos", "flips", "lookalike"):
        ev = gold[name + "_ev"]
        assert len(ev) >= 2 and (ev[:, 4] == 7).all() and (np.diff(ev[:, 2]) == 1).all(), name
    assert (np.diff(gold["lossy_ev"][:, 0]) > 7000).any()  # lock lost over the ruined messages, found again


def test_branches_hit(golden_runs):
    total = {k: sum(r[0].br[k] for r in golden_runs.values()) for k in M.BRANCHES}
    for k in ("rescan_hit", "rescan_miss", "retry_crc_no_lock", "lock_lost", "flush_part1", "flush_part2", "norm_taken", "norm_skipped_above"):
        assert total[k] >= 1, (k, total)
    assert golden_runs["lossy"][0].br["lock_lost"] >= 1 and golden_runs["lookalike"][0].br["retry_crc_no_lock"] >= 1
    assert golden_runs["norm_state0"][0].br["norm_taken"] >= 1
    assert golden_runs["norm_others"][0].br["norm_taken"] == 0 and golden_runs["norm_others"][0].br["norm_skipped_above"] >= 1
    assert golden_runs["lead1_pos"][0].br["flush_part1"] >= 1 and golden_runs["lead0_pos"][0].br["flush_part2"] >= 1


def test_polarity_only_changes_the_flag(gold):
    for lead in (0, 1, 37):
        a, b = gold[f"lead{lead}_pos_ev"], gold[f"lead{lead}_neg_ev"]
        assert np.array_equal(a, b) and np.array_equal(gold[f"lead{lead}_pos_raw"][:, :37], gold[f"lead{lead}_neg_raw"][:, :37])


@pytest.mark.parametrize("mode", [M.L2C, M.L5])
def test_block_stamps_every_symbol(mode):
    bits, _ = M.golden_streams()["lead0_neg"]
    blk = M.CnavBlock(mode)
    recs, fault, tow, sf = blk.run(M.to_float(bits))
    assert [r["symbol_counter"] for r in recs] == [704, 1280, 1920] and not fault
    assert all(r["flags"] == (M.F_CRC_OK | M.F_INVERTED | M.F_LOCK) and r["part"] == 0 and r["prn"] == 7 for r in recs)
    k = 703
    period = 20 if mode == M.L2C else 10
    stamp = recs[0]["tow"] * 6000 + (recs[0]["delay"] + 12) * period
    assert tow[k] == stamp and sf[k] == (M.S_VALID_WORD | M.S_PLL_180 | M.S_MESSAGE)
    assert np.array_equal(tow[k:1279], stamp + period * np.arange(1279 - k)) and (sf[k + 1:1279] == (M.S_VALID_WORD | M.S_PLL_180)).all()
    assert not (sf[:k] & M.S_VALID_WORD).any()
    if mode == M.L2C:  # the double counts from 0 before the first message, one addition per symbol
        t, want = 0.0, []
        for _ in range(k):
            t += 0.02
            want.append(M._round_ms(t * 1000.0))
        assert tow[:k].tolist() == want
    else:
        assert not tow[:k].any()
        assert tow[1279] == tow[1278] + 10 and blk.tow_inconsistent == 0  # consecutive TOWs agree with the symbol count


def test_l5_tow_inconsistency():
    """TOW steps of 2 between messages: the second message's stamp is 6 s from the counted one, so TOW and valid_word
    become 0; the third then finds a zero previous value and stamps again."""
    x = M.to_float(M.stream(M.messages(4, 61, tow_step=2), 0, 61))
    blk = M.CnavBlock(M.L5)
    recs, _, tow, sf = blk.run(x)
    assert [r["symbol_counter"] for r in recs] == [704, 1280, 1920] and blk.tow_inconsistent == 1
    assert sf[1279] == M.S_MESSAGE and tow[1279] == 0 and not sf[1280:1919].any() and not tow[1280:1919].any()
    # (the 180° flag may be set on this clean stream: it takes in the stale `invert` of the part that is not locked)
    assert int(sf[1919]) & ~M.S_PLL_180 == (M.S_VALID_WORD | M.S_MESSAGE) and tow[1919] == recs[2]["tow"] * 6000 + (recs[2]["delay"] + 12) * 10
    assert blk.last_valid_preamble == 1920
    # the L2C block has no such test
    l2 = M.CnavBlock(M.L2C)
    _, _, tow2, sf2 = l2.run(x)
    assert (sf2[703:] & M.S_VALID_WORD).all() and tow2[1279] == recs[1]["tow"] * 6000 + (recs[1]["delay"] + 12) * 20


@pytest.mark.parametrize("mode", [M.L2C, M.L5])
def test_out_valid_drops_the_word(mode):
    x = M.to_float(M.golden_streams()["lead0_pos"][0])
    ov = np.ones(len(x), np.uint8)
    ov[900] = 0
    ov[703] = 0  # on the message's own symbol the flag is not looked at
    blk = M.CnavBlock(mode)
    _, _, tow, sf = blk.run(x, out_valid=ov)
    assert (sf[703:900] & M.S_VALID_WORD).all() and not (sf[900:1279] & M.S_VALID_WORD).any()
    if mode == M.L2C:
        assert tow[900] == tow[899] + 20 and tow[901] == tow[900] + 20  # the double goes on counting
        assert sf[1279] & M.S_VALID_WORD
    else:
        assert not tow[900:1279].any()  # the output is silent; the member froze after the 10 ms of symbol 900


def test_l5_out_valid_drop_then_inconsistency():
    """After the drop the L5 member stands still and is non-zero, so the next message's stamp is refused as inconsistent
    and only the one after it stamps."""
    x = M.to_float(M.golden_streams()["lead0_pos"][0])
    ov = np.ones(len(x), np.uint8)
    ov[900] = 0
    blk = M.CnavBlock(M.L5)
    recs, _, tow, sf = blk.run(x, out_valid=ov)
    frozen = recs[0]["tow"] * 6000 + (recs[0]["delay"] + 12) * 10 + 10 * (900 - 703)
    assert blk.tow_inconsistent == 1 and sf[1279] == M.S_MESSAGE and int(sf[1919]) & ~M.S_PLL_180 == (M.S_VALID_WORD | M.S_MESSAGE)
    assert tow[899] == frozen - 10 and tow[900] == 0


@pytest.mark.parametrize("mode", [M.L2C, M.L5])
def test_watchdog_at_its_exact_symbol_and_reset(mode):
    limit = M.WATCHDOG[mode]
    assert limit == (3000 if mode == M.L2C else 6000)
    blk = M.CnavBlock(mode)
    zeros = np.zeros(limit, np.float32)
    assert not blk.run(zeros)[1] and not blk.sent_tlm_failed
    assert blk.run(zeros[:1])[1] and blk.sent_tlm_failed and blk.symbol_counter == limit + 1
    assert not blk.run(zeros)[1]  # once, until reset
    blk.valid_word, blk.tow_ms, blk.tow_s = True, 5000, 7.0
    before = blk.state()
    blk.reset()
    st = blk.state()
    assert st["last_valid_preamble"] == st["symbol_counter"] == 2 * limit + 1 and not st["sent_tlm_failed"]
    if mode == M.L2C:
        assert st["valid_word"] == 1 and st["tow_s"] == 7.0 and st["tow_ms"] == 5000
    else:
        assert st["valid_word"] == 0 and st["tow_ms"] == 0 and st["tow_s"] == 7.0
    for k in range(2):  # neither reset touches the CNAV decoder
        for f, v in st[f"part{k}"].items():
            assert np.array_equal(v, before[f"part{k}"][f]), f
    assert not blk.run(zeros)[1]
    assert blk.run(zeros[:1])[1]


def test_nan_and_zero_are_zero_symbols():
    bits = M.golden_streams()["lead0_pos"][0]
    x = M.to_float(bits)
    y = x.copy()
    z = np.nonzero(bits == 0)[0]
    y[z[0::4]], y[z[1::4]], y[z[2::4]], y[z[3::4]] = 0.0, -0.0, np.nan, -1e-45
    y[np.nonzero(bits == 1)[0][::2]] = 1e-45
    a, b = M.CnavBlock(M.L2C).run(x), M.CnavBlock(M.L2C).run(y)
    assert [r["raw"] for r in a[0]] == [r["raw"] for r in b[0]] and np.array_equal(a[2], b[2]) and len(a[0]) == 3


def test_state_round_trip_continues_identically():
    x = M.to_float(M.golden_streams()["lead1_neg"][0])
    a = M.CnavBlock(M.L5)
    a.run(x[:1000])
    b = M.CnavBlock(M.L5)
    b.set_state(a.state())
    ra, rb = a.run(x[1000:]), b.run(x[1000:])
    assert [r["raw"] for r in ra[0]] == [r["raw"] for r in rb[0]] and np.array_equal(ra[2], rb[2]) and np.array_equal(ra[3], rb[3])
    sa, sb = a.state(), b.state()
    assert all(np.array_equal(sa["part0"][f], sb["part0"][f]) and np.array_equal(sa["part1"][f], sb["part1"][f]) for f in sa["part0"])


def test_messages_per_run_bound():
    """Every record disposes of 300 decoded bits; a part gains 32 bits per decode, decodes are 64 symbols apart (the first
    may be due at once, with up to 127 symbols held), and state_set admits at most 480 held bits per part."""
    for n in range(1, 5000, 13):
        bits = 2 * (480 + 32 * (n // 64 + 2))
        assert bits // 300 <= M.messages_per_run(n), n
