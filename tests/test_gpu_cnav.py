"""The device GPS CNAV telemetry decoder (tlm_gps_cnav.hip, gnsship_cnav_*) against the restatement of libswiftcnav and of
gps_l2c_telemetry_decoder_gs / gps_l5_telemetry_decoder_gs in tests/cnav_model.py, which tests/test_cnav_model.py holds
against the reference's own output.

Contract: exact equality, no tolerance anywhere — every field of every message record, every tow_ms / sflags entry,
counts, faults and every member of gnsship_cnav_state (both metric buffers, the 64 decision words, both buffers of both
parts, every counter and flag, the block's members) — for both signals, both polarities, any lead, any cut of a stream
into runs, any number of channels, validity and output-valid masks, tracking records (host, device, in place), zeros,
NaNs and denormals, and states written with state_set."""
import numpy as np
import pytest

import cnav_model as M
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

MSG_FIELDS = ["symbol_counter", "sample_counter", "channel", "tow", "delay", "prn", "msg_id", "alert", "part", "flags"]
PART_SCALARS = ["n_symbols", "n_decoded", "n_crc_fail", "decisions_index", "old_is_metrics2", "preamble_seen", "invert", "message_lock",
                "crc_ok", "init"]
PART_ARRAYS = ["metrics", "decisions", "symbols", "decoded"]
BLOCK_FIELDS = ["symbol_counter", "last_valid_preamble", "tow_ms", "tow_at_preamble", "pll_180", "valid_word", "sent_tlm_failed"]
MODES = [M.L2C, M.L5]


def assert_state(got, want, label=""):
    """got: abi.CNAV_STATE_DTYPE record from the device; want: CnavBlock.state()."""
    for k in range(2):
        g, w = got["part"][k], want[f"part{k}"]
        for f in PART_SCALARS:
            assert int(g[f]) == int(w[f]), (label, k, f, int(g[f]), int(w[f]))
        for f in PART_ARRAYS:
            assert np.array_equal(g[f], w[f]), (label, k, f)
    for f in BLOCK_FIELDS:
        assert int(got[f]) == int(want[f]), (label, f, int(got[f]), int(want[f]))
    assert np.float64(got["tow_s"]).tobytes() == np.float64(want["tow_s"]).tobytes(), (label, "tow_s", float(got["tow_s"]), want["tow_s"])


def state_record(st: dict) -> np.ndarray:
    """CnavBlock.state() as an abi.CNAV_STATE_DTYPE record."""
    rec = np.zeros((), abi.CNAV_STATE_DTYPE)
    for k in range(2):
        for f in PART_SCALARS + PART_ARRAYS:
            rec["part"][k][f] = st[f"part{k}"][f]
    for f in BLOCK_FIELDS + ["tow_s"]:
        rec[f] = st[f]
    return rec


class Pair:
    """A device decoder and one model block per channel, fed the same runs and compared after each."""

    def __init__(self, ctx, mode, channels, max_rounds):
        self.C, self.mode = channels, mode
        self.dev = engine.GpsCnavTelemetryDecoder(ctx, mode, channels, max_rounds)
        assert self.dev.messages_per_run == M.messages_per_run(max_rounds) == abi.cnav_messages_per_run(max_rounds)
        self.mod = [M.CnavBlock(mode) for _ in range(channels)]
        self.msgs = [[] for _ in range(channels)]
        self.out = [[] for _ in range(channels)]

    def close(self):
        self.dev.close()

    def expect(self, sym, valid=None, out_valid=None, sample_counters=None):
        sym = np.asarray(sym).reshape(-1, self.C)
        out = []
        for c, m in enumerate(self.mod):
            recs, fault, tow, sf = m.run(sym[:, c], None if valid is None else valid[:, c], None if out_valid is None else out_valid[:, c],
                                         None if sample_counters is None else sample_counters[:, c], c)
            out.append((recs, fault, tow, sf))
        return out

    def check(self, res, exp, label=""):
        assert res.counts.tolist() == [len(e[0]) for e in exp], (label, res.counts.tolist(), [len(e[0]) for e in exp])
        assert res.faults.tolist() == [int(e[1]) for e in exp], (label, res.faults.tolist())
        for c, (recs, _, tow, sf) in enumerate(exp):
            assert len(recs) <= self.dev.messages_per_run
            for k, r in enumerate(recs):
                got = res.messages[c, k]
                have = tuple(int(got[f]) for f in MSG_FIELDS) + (got["raw"].tobytes(), int(got["reserved"]))
                want = tuple(int(r[f]) for f in MSG_FIELDS) + (r["raw"][:38], 0)
                assert have == want, (label, c, k, have, want)
                self.msgs[c].append(have)
            assert np.array_equal(res.tow_ms[:, c], tow), (label, c, np.nonzero(res.tow_ms[:, c] != tow)[0][:5])
            assert np.array_equal(res.sflags[:, c], sf), (label, c, np.nonzero(res.sflags[:, c] != sf)[0][:5])
            self.out[c].append((tow.copy(), sf.copy()))
        self.check_state(label)

    def check_state(self, label=""):
        for c in range(self.C):
            assert_state(self.dev.state(c), self.mod[c].state(), (label, c))

    def run(self, sym, valid=None, out_valid=None, label=""):
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        res = self.dev.run_symbols(sym, valid, out_valid)
        self.check(res, self.expect(sym, valid, out_valid), label)
        return res


def test_new_object_is_decoder_init(ctx):
    for mode in MODES:
        p = Pair(ctx, mode, 2, 10)
        p.check_state("new")
        st = p.dev.state(1)
        assert st["part"][1]["n_symbols"] == 1 and st["part"][1]["symbols"][0] == 0x80 and st["part"][0]["metrics"][0, :2].tolist() == [0, 63]
        p.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["lead0_pos", "lead0_neg", "lead1_pos", "lead1_neg", "lead37_pos", "lead37_neg"])
def test_device_equals_model(ctx, mode, name):
    """Leads 0, 1 and 37 in both polarities: part 1, part 2 and part 2 again find the messages (2000 symbols each)."""
    bits = M.golden_streams()[name][0][:2000]
    p = Pair(ctx, mode, 1, len(bits))
    res = p.run(M.to_float(bits), label=name)
    want = {"lead0": [704, 1280, 1920], "lead1": [703, 1279, 1919], "lead37": [1343, 1919]}[name.split("_")[0]]
    assert res.messages[0]["symbol_counter"][:res.counts[0]].tolist() == want
    assert (res.messages[0]["flags"][:res.counts[0]] & abi.CNAV_CRC_OK).all() and (res.messages[0]["prn"][:res.counts[0]] == 7).all()
    assert bool(res.messages[0]["flags"][0] & abi.CNAV_INVERTED) == name.endswith("neg")
    assert res.sflags[-1, 0] & abi.CNAV_S_VALID_WORD and res.tow_ms[-1, 0] > 6000000
    p.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cut", [1, 63, 64, 65, 127, 128, 129, 600])
def test_cuts_give_identical_outputs(ctx, mode, cut):
    """The same stream in runs of `cut` symbols, with a reset at a cut: the 64-entry chunk boundary and both decode
    thresholds fall on, before and after a run boundary."""
    n = 900 if cut == 1 else 2000
    x = M.to_float(M.golden_streams()["lead1_neg"][0][:n])
    reset_at = 800 // cut * cut if cut <= 800 else cut
    whole = Pair(ctx, mode, 1, n)
    whole.run(x[:reset_at])
    whole.dev.reset_channel(0)
    whole.mod[0].reset()
    whole.run(x[reset_at:])
    p = Pair(ctx, mode, 1, cut)
    for k in range(0, n, cut):
        if k == reset_at:
            p.dev.reset_channel(0)
            p.mod[0].reset()
        res = p.dev.run_symbols(x[k:k + cut].reshape(-1, 1))
        exp = p.expect(x[k:k + cut].reshape(-1, 1))
        if cut > 1 or k % 97 == 0 or exp[0][0]:
            p.check(res, exp, (cut, k))  # every run, but for cut 1 the state only now and then (it is 2.5 kB a read)
        else:
            assert res.counts[0] == 0 and res.tow_ms[0, 0] == exp[0][2][0] and res.sflags[0, 0] == exp[0][3][0]
    p.check_state("end")
    if cut > 1:
        assert p.msgs[0] == whole.msgs[0] and len(p.msgs[0]) == 3
        assert np.array_equal(np.concatenate([t for t, _ in p.out[0]]), np.concatenate([t for t, _ in whole.out[0]]))
    for h in (p, whole):
        h.close()


@pytest.mark.parametrize("mode", MODES)
def test_three_channels_masks_and_odd_symbols(ctx, mode):
    """Three channels with different streams, a validity mask with gaps (a whole chunk without an entry among them), an
    output-valid mask, and symbols that are NaN, +0, -0 and denormal: (x > 0) * 255 exactly."""
    rng = np.random.default_rng(3)
    g = M.golden_streams()
    streams = [g["lead0_pos"][0][:1500], g["lead37_neg"][0][:1500], g["flips"][0][:1500]]
    Cn, n = 3, 1500
    rounds = 2 * n
    valid = np.zeros((rounds, Cn), np.uint8)
    sym = (rng.standard_normal((rounds, Cn)) * 9.0).astype(np.float32)  # what sits in invalid entries must not matter
    for c in range(Cn):
        rows = np.sort(rng.choice(rounds, n, replace=False)) if c else np.arange(n)  # channel 0: nothing in the second half
        valid[rows, c] = 1
        x = M.to_float(streams[c]) * np.float32(1.0 + 0.5 * c)
        zeros, ones = np.nonzero(streams[c] == 0)[0], np.nonzero(streams[c] == 1)[0]
        x[zeros[0::5]], x[zeros[1::5]], x[zeros[2::5]], x[zeros[3::5]] = 0.0, -0.0, np.nan, -1e-40
        x[ones[0::3]] = 1e-40  # a positive denormal is a one
        sym[rows, c] = x
    valid[1664:1728, 1:] = 0  # a whole chunk with no entry on two channels (their streams shorten)
    out_valid = (rng.integers(0, 50, (rounds, Cn)) != 0).astype(np.uint8)
    p = Pair(ctx, mode, Cn, rounds)
    res = p.run(sym, valid, out_valid, "masks")
    assert res.counts[0] == 2 and res.counts.sum() >= 4
    assert (res.tow_ms[valid == 0] == 0).all() and (res.sflags[valid == 0] == 0).all()
    vw = (res.sflags & abi.CNAV_S_VALID_WORD) != 0
    assert vw.any() and (~vw[valid != 0]).any()
    p.close()


def records_from(sym, valid, rng, mode):
    """Tracking records whose valid entries carry the symbols as doubles; positive ones include values a float flushes to
    zero.  The other prompt carries noise of the opposite meaning."""
    rec = np.zeros(sym.shape, abi.TRK_EPOCH_DTYPE)
    mag = np.where(rng.integers(0, 4, sym.shape) == 0, 1e-60, 1.0 + rng.uniform(0, 1, sym.shape))
    mine = np.where(sym > 0, mag, -mag)
    rec["prompt_i" if mode == M.L2C else "prompt_q"] = mine
    rec["prompt_q" if mode == M.L2C else "prompt_i"] = -mine
    rec["flags"] = 8 | np.where(valid != 0, 1, 0)
    rec["sample_counter"] = (np.arange(sym.shape[0], dtype=np.uint64)[:, None] * np.uint64(80000) + np.uint64(1 << 33)
                             + np.arange(sym.shape[1], dtype=np.uint64)[None, :])
    return rec, mine


@pytest.mark.parametrize("mode", MODES)
def test_records_host_and_device(ctx, mode):
    """Records from the host and from the device: the comparison is on the double itself (1e-60 > 0, though a float would
    flush it to zero), L2C reads prompt_i and L5 prompt_q, and the message carries the completing record's sample counter."""
    rng = np.random.default_rng(5)
    g = M.golden_streams()
    Cn, n = 2, 1400
    sym = np.stack([M.to_float(g["lead0_neg"][0][:n]), M.to_float(g["lead1_pos"][0][:n])], axis=1)
    valid = np.ones((n, Cn), np.uint8)
    valid[rng.choice(n, 40, replace=False), 1] = 0
    rec, mine = records_from(sym, valid, rng, mode)
    assert (mine.astype(np.float32) == 0).any()
    a = Pair(ctx, mode, Cn, n)
    exp = a.expect(mine, valid, None, rec["sample_counter"])
    a.check(a.dev.run_records(rec), exp, "host records")
    assert a.msgs[0] and a.msgs[0][0][1] == int(rec["sample_counter"][703, 0])
    b = Pair(ctx, mode, Cn, n)
    buf = ctx.upload(rec)
    expb = b.expect(mine, valid, None, rec["sample_counter"])
    b.check(b.dev.run_records(buf.ptr, on_device=True, n_rounds=n), expb, "device records")
    assert b.msgs == a.msgs and len(a.msgs[0]) == 2
    # as floats the tiny positive prompts are zeros: another stream
    c = Pair(ctx, mode, Cn, n)
    resc = c.run(mine.astype(np.float32), valid, None, "narrowed")
    assert resc.counts.sum() < 3
    buf.free()
    for h in (a, b, c):
        h.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["norm_state0", "norm_others"])
def test_near_limit_states_through_state_set(ctx, mode, name):
    """Metrics just under 2^30, written with state_set: in one stream state 0 crosses the limit and the metrics are
    normalised; in the other only other states do, and nothing is."""
    bits, bias = M.golden_streams()[name]
    p = Pair(ctx, mode, 1, len(bits))
    p.mod[0].dec.add_metrics(bias)
    p.dev.set_state(0, state_record(p.mod[0].state()))
    p.check_state("set")
    res = p.run(M.to_float(bits), label=name)
    br = p.mod[0].dec.br
    if name == "norm_state0":
        assert br["norm_taken"] >= 1 and res.counts[0] == 2
        assert p.dev.state(0)["part"][0]["metrics"].max() < (1 << 20)
    else:
        assert br["norm_taken"] == 0 and br["norm_skipped_above"] >= 1
        assert p.dev.state(0)["part"][0]["metrics"].max() > (1 << 30)
    p.close()


@pytest.mark.parametrize("mode", MODES)
def test_state_moves_between_handles(ctx, mode):
    """state_get -> new_channel -> state_set gives the identical continuation, on the same handle and on another."""
    x = M.to_float(M.golden_streams()["lead1_neg"][0][:2000])
    a = Pair(ctx, mode, 1, 2000)
    a.run(x[:1000])
    st = a.dev.state(0)
    a.dev.new_channel(0)
    assert_state(a.dev.state(0), M.CnavBlock(mode).state(), "new_channel")
    a.dev.set_state(0, st)
    b = Pair(ctx, mode, 2, 2000)
    b.dev.set_state(1, st)
    b.mod[1].set_state(a.mod[0].state())
    ra = a.run(x[1000:], label="same handle")
    rb = b.run(np.stack([x[1000:], x[1000:]], axis=1), label="other handle")
    assert ra.counts[0] == 2 and rb.counts[1] == 2 and np.array_equal(ra.tow_ms[:, 0], rb.tow_ms[:, 1])
    assert [m[:1] + m[3:] for m in a.msgs[0][1:]] == [m[:1] + m[3:] for m in b.msgs[1]]  # all but the channel number
    for h in (a, b):
        h.close()


@pytest.mark.parametrize("mode", MODES)
def test_lock_lost_and_found(ctx, mode):
    """12 ruined messages: every disposal is a record, the CRC fails are counted, lock is lost at the eleventh and found
    again; the watchdog fires on the way.  12 x 600 symbols on one channel, in runs of 2400."""
    bits = M.golden_streams()["lossy"][0]
    x = M.to_float(bits)
    p = Pair(ctx, mode, 1, 2400)
    fired = 0
    for k in range(0, len(x), 2400):
        res = p.run(x[k:k + 2400], label=k)
        fired += int(res.faults[0])
    flags = [m[MSG_FIELDS.index("flags")] for m in p.msgs[0]]
    assert fired == 1 and p.mod[0].dec.br["lock_lost"] == 1 and p.mod[0].dec.br["locked_crc_fail"] == 11
    assert sum(1 for f in flags if not f & abi.CNAV_CRC_OK) == 10 and flags[0] & abi.CNAV_CRC_OK and flags[-1] & abi.CNAV_CRC_OK
    p.close()


def test_lookalike_preamble(ctx):
    p = Pair(ctx, M.L2C, 1, 2300)
    res = p.run(M.to_float(M.golden_streams()["lookalike"][0]))
    assert p.mod[0].dec.br["retry_crc_no_lock"] >= 1 and res.counts[0] == 2
    p.close()


def test_l5_tow_inconsistency_and_watchdogs(ctx):
    x = M.to_float(M.stream(M.messages(4, 61, tow_step=2), 0, 61))[:2000]
    p = Pair(ctx, M.L5, 1, 6001)
    res = p.run(x)
    assert p.mod[0].tow_inconsistent == 1 and res.sflags[1279, 0] == abi.CNAV_S_MESSAGE and res.tow_ms[1279, 0] == 0
    p.close()
    for mode in MODES:
        limit = M.WATCHDOG[mode]
        p = Pair(ctx, mode, 1, 6001)
        zeros = np.zeros(limit, np.float32)
        assert p.run(zeros).faults[0] == 0
        assert p.run(zeros[:1]).faults[0] == 1
        assert p.run(zeros).faults[0] == 0
        p.dev.reset_channel(0)
        p.mod[0].reset()
        p.check_state("reset")
        assert p.run(zeros).faults[0] == 0 and p.run(zeros[:1]).faults[0] == 1
        p.close()


def test_rejected_calls(ctx):
    with pytest.raises(abi.GnssHipError) as e:
        engine.GpsCnavTelemetryDecoder(ctx, abi.CNAV_L2C, 1, 0)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.GnssHipError) as e:
        engine.GpsCnavTelemetryDecoder(ctx, abi.CNAV_L5, 0, 10)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.GnssHipError) as e:
        engine.GpsCnavTelemetryDecoder(ctx, 2, 1, 10)
    assert e.value.code == abi.E_INVAL and b"signal" in ctx.lib.gnsship_last_error(ctx.h)
    d = engine.gps_l5_telemetry(ctx, 2, 10)
    assert d.signal == abi.CNAV_L5 and engine.gps_l2c_telemetry(ctx, 1, 10).signal == abi.CNAV_L2C
    d.run_symbols(np.ones((4, 2), np.float32))
    before = d.state(0)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_symbols(np.ones((11, 2), np.float32))
    assert e.value.code == abi.E_INVAL and b"max_rounds" in ctx.lib.gnsship_last_error(ctx.h)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_records(np.zeros((11, 2), abi.TRK_EPOCH_DTYPE))
    assert e.value.code == abi.E_INVAL
    for call in (d.reset_channel, d.new_channel, d.state, lambda ch: d.set_state(ch, before)):
        for ch in (-1, 2):
            with pytest.raises(abi.GnssHipError) as e:
                call(ch)
            assert e.value.code == abi.E_INVAL
    for field, value in (("n_symbols", 128), ("n_decoded", 481), ("decisions_index", 64), ("init", 2)):
        bad = before.copy()
        bad["part"][1][field] = value
        with pytest.raises(abi.GnssHipError) as e:
            d.set_state(0, bad)
        assert e.value.code == abi.E_INVAL and b"gnsship_cnav_state_set" in ctx.lib.gnsship_last_error(ctx.h)
    assert d.state(0).tobytes() == before.tobytes()
    assert d.run_symbols(np.zeros((0, 2), np.float32)).counts.tolist() == [0, 0] and d.state(0).tobytes() == before.tobytes()
    lib = ctx.lib
    assert lib.gnsship_cnav_run_symbols(None, None, None, None, 0, 0, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_cnav_run_trk(None, None, None, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_cnav_state_set(None, 0, None) == abi.E_INVAL
    assert lib.gnsship_cnav_destroy(None) == abi.E_INVAL
    d.close()


@pytest.mark.parametrize("mode", MODES)
def test_run_trk_in_place(ctx, mode):
    """A short tracking run; its device records go through the decoder in place.  No message can appear in so short a
    run: the check is the state, the tow_ms / sflags stream, the equality with run_records and the model, the error
    codes, and the tracker's own records left as they were."""
    import trk_scenarios as S
    from test_gpu_trk import dev_conf
    fs, rounds = 4e6, 400
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, rounds, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(72, sat.code)
    trk.start(0, 72, delay, dop, stamp, first)
    x = np.ascontiguousarray(x, np.complex64)
    buf = ctx.upload(x)
    make = lambda ch, mr: engine.GpsCnavTelemetryDecoder(ctx, mode, ch, mr)
    in_place = make(1, rounds)
    with pytest.raises(abi.GnssHipError) as e:  # nothing launched yet
        in_place.run_trk(trk)
    assert e.value.code == abi.E_STATE
    trk.launch_ptr(buf.ptr, abi.FMT_CF32, first, len(x), rounds, records=True)
    got = in_place.run_trk(trk)  # before the collect
    rec, done = trk.collect()
    again = make(1, rounds)
    res = again.run_trk(trk)  # and after it
    other = make(1, rounds)
    ref = other.run_records(rec)
    wrong = make(2, rounds)
    with pytest.raises(abi.GnssHipError) as e:
        wrong.run_trk(trk)
    assert e.value.code == abi.E_INVAL
    small = make(1, 10)
    with pytest.raises(abi.GnssHipError) as e:
        small.run_trk(trk)
    assert e.value.code == abi.E_INVAL
    sel = (rec[:, 0]["flags"] & 1) != 0
    assert sel.sum() >= 5
    m = M.CnavBlock(mode)
    recs, fault, tow, sf = m.run(rec[sel, 0]["prompt_q" if mode == M.L5 else "prompt_i"], None, None, rec[sel, 0]["sample_counter"])
    assert not recs and not fault
    for r in (got, res, ref):
        assert r.counts[0] == 0 and r.faults[0] == 0
        n = r.tow_ms.shape[0]
        assert n >= done and np.array_equal(r.tow_ms[:done][sel[:done], 0], tow) and np.array_equal(r.sflags[:done][sel[:done], 0], sf)
        assert not r.sflags[:done][~sel[:done], 0].any()
    for h in (in_place, other, again):
        assert_state(h.state(0), m.state())
    assert m.symbol_counter == int(sel.sum())
    plain = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    plain.start(0, 72, delay, dop, stamp, first)
    rec_plain, done_plain = plain.run(x, first, rounds)
    assert done_plain == done and rec_plain.tobytes() == rec.tobytes()
    plain.close()
    for h in (in_place, again, other, wrong, small, trk):
        h.close()
    buf.free()
