"""The device GPS L1 C/A telemetry decoder (tlm_gps_lnav.hip, gnsship_lnav_*) against the restatement of
gps_l1_ca_telemetry_decoder_gs in tests/lnav_model.py.

Contract: exact equality — every field of every subframe record, every tow_ms / sflags entry, counts, faults and every
member of gnsship_lnav_state — for both polarities, the seeded path and a lead-in, any cut of a stream into runs, any
number of channels, validity masks, 180° flags, tracking records (host, device, in place), zeros and NaNs."""
import numpy as np
import pytest

import lnav_model as M
import test_lnav_model as C
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

SUB_FIELDS = ["symbol_counter", "sample_counter", "subframe_id", "tow_s", "crc_error_counter", "parity_fail_mask", "flags"]


class Pair:
    """A device decoder and one model object per channel, fed the same runs and compared after each."""

    def __init__(self, ctx, channels, max_rounds):
        self.C = channels
        self.dev = engine.GpsL1CaTelemetryDecoder(ctx, channels, max_rounds)
        assert self.dev.subframes_per_run == M.subframes_per_run(max_rounds) == abi.lnav_subframes_per_run(max_rounds)
        self.mod = [M.LnavDecoder() for _ in range(channels)]
        self.subs = [[] for _ in range(channels)]  # everything emitted so far, per channel
        self.tow = [[] for _ in range(channels)]   # (tow_ms, sflags) of every symbol so far, per channel

    def close(self):
        self.dev.close()

    def expect(self, sym, valid=None, flags180=None, sample_counters=None):
        """Run the models over sym[n_rounds, C]: per channel (records, fault, tow_ms[n_rounds], sflags[n_rounds])."""
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        out, ran = [], {}
        for c, m in enumerate(self.mod):
            if id(m) in ran:  # channels given the same stream may share one model object
                first = ran[id(m)]
                assert valid is None and sample_counters is None and flags180 is None
                assert np.array_equal(sym[:, c], sym[:, first], equal_nan=True)
                out.append(out[first])
                continue
            ran[id(m)] = c
            sel = np.ones(sym.shape[0], bool) if valid is None else valid[:, c] != 0
            recs, fault, tow, sf = m.run(sym[sel, c], None if sample_counters is None else sample_counters[sel, c],
                                         None if flags180 is None else flags180[sel, c])
            full_tow, full_sf = np.zeros(sym.shape[0], np.uint32), np.zeros(sym.shape[0], np.uint8)
            full_tow[sel], full_sf[sel] = tow, sf
            out.append((recs, fault, full_tow, full_sf))
        return out

    def check(self, res, exp, label=""):
        assert res.counts.tolist() == [len(e[0]) for e in exp], (label, res.counts.tolist())
        assert res.faults.tolist() == [int(e[1]) for e in exp], (label, res.faults.tolist())
        for c, (recs, _, tow, sf) in enumerate(exp):
            assert len(recs) <= self.dev.subframes_per_run
            for k, r in enumerate(recs):
                got = res.subframes[c, k]
                have = tuple(int(got[f]) for f in SUB_FIELDS) + (int(got["channel"]),) + tuple(int(w) for w in got["words"])
                want = tuple(int(r[f]) for f in SUB_FIELDS) + (c,) + tuple(r["words"])
                assert have == want, (label, c, k, have, want)
                self.subs[c].append(have)
            assert np.array_equal(res.tow_ms[:, c], tow), (label, c, np.nonzero(res.tow_ms[:, c] != tow)[0][:5])
            assert np.array_equal(res.sflags[:, c], sf), (label, c, np.nonzero(res.sflags[:, c] != sf)[0][:5])
            self.tow[c].append((tow.copy(), sf.copy()))
        self.check_state(label)

    def check_state(self, label="", channels=None):
        for c in (range(self.C) if channels is None else channels):
            got, want = self.dev.state(c), self.mod[c].state()
            assert got == want, (label, c, got, want)

    def run(self, sym, valid=None, flags180=None, label=""):
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        res = self.dev.run_symbols(sym, valid, flags180)
        self.check(res, self.expect(sym, valid, flags180), label)
        return res


def stream(n, lead, seed=5, sign=1.0):
    return np.float32(sign) * M.build_stream(M.five_subframes(seed)[0], n, lead, seed + 1)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("lead", [0, 37])
def test_device_equals_model(ctx, lead, sign):
    """lead 0: what a tracker hands over (the stream from the symbol after a preamble, the 180° flag as it locked): the
    seeded preamble lets the first subframe decode at counter 300.  lead 37: behind random symbols, at 345."""
    n = 1000
    bits, words = M.five_subframes(5)
    x = C.tracked(bits, n, sign) if lead == 0 else stream(n, lead, sign=sign)
    f180 = np.full((n, 1), sign < 0, np.uint8)
    p = Pair(ctx, 1, n)
    res = p.run(x, flags180=f180)
    first = 300 if lead == 0 else 345
    assert res.counts[0] == 3 and res.subframes[0]["symbol_counter"][:3].tolist() == [first, first + 300, first + 600]
    for k in range(3):
        assert res.subframes[0, k]["words"].tolist() == words[k] and res.subframes[0, k]["flags"] & abi.LNAV_OK
        assert bool(res.subframes[0, k]["flags"] & abi.LNAV_PLL_180) == (sign < 0)
    assert res.subframes[0]["tow_s"][:3].tolist() == [6000, 6006, 6012]
    assert res.tow_ms[-1, 0] == 6012000 + 20 * (n + 8 - (first + 600)) and res.sflags[-1, 0] & abi.LNAV_S_OUTPUT
    p.close()


@pytest.mark.parametrize("cut", [1, 7, 63, 64, 65, 299, 300, 301, 600])
def test_cuts_give_identical_outputs(ctx, cut):
    """The same stream in runs of `cut` symbols: the 64-entry chunk boundary, the due symbol, and the seeding at a cut
    (a reset between two runs)."""
    n = 1000 if cut == 1 else 1300
    bits, _ = M.five_subframes(5)
    x = C.tracked(bits, n)
    reset_at = 420 // cut * cut if cut <= 420 else cut  # a run boundary
    whole = Pair(ctx, 1, n)
    whole.run(x[:reset_at])
    whole.dev.reset_channel(0)
    whole.mod[0].reset()
    whole.run(x[reset_at:])
    p = Pair(ctx, 1, cut)
    for k in range(0, n, cut):
        if k == reset_at:
            p.dev.reset_channel(0)
            p.mod[0].reset()
        p.run(x[k:k + cut], label=f"run at {k}")
    assert p.subs[0] == whole.subs[0] and len(whole.subs[0]) >= 2
    for i in (0, 1):
        assert np.array_equal(np.concatenate([t[i] for t in p.tow[0]]), np.concatenate([t[i] for t in whole.tow[0]]))
    assert p.dev.state(0) == whole.dev.state(0)
    whole.close()
    p.close()


@pytest.mark.parametrize("channels", [1, 5, 257])
def test_channels_with_different_lead_ins(ctx, channels):
    """Subframes fall due at different symbols: in the second run a channel emits one or two, in the third none or one."""
    n = 1300
    leads = [(3 + 61 * (c % 32)) % 300 for c in range(channels)]  # 32 lead-ins: the model runs once per distinct stream
    distinct = [stream(n, leads[c], seed=5 + c % 3, sign=-1.0 if c % 2 else 1.0) for c in range(min(channels, 32))]
    x = np.stack([distinct[c % 32] for c in range(channels)], axis=1)
    p = Pair(ctx, channels, 900)
    p.mod = [p.mod[c % 32] for c in range(channels)]
    p.run(x[:900], label="first")
    res = p.run(x[900:], label="second")  # 400 symbols
    if channels > 1:
        assert set(res.counts.tolist()) == {1, 2}
    third = p.run(x[:100], label="third")
    assert set(third.counts.tolist()) <= {0, 1} and 0 in third.counts.tolist()
    if channels == 257:  # a channel among 256 others equals the channel alone
        alone = Pair(ctx, 1, 900)
        for part in (x[:900, 200], x[900:, 200], x[:100, 200]):
            alone.run(part)
        assert len(alone.subs[0]) == len(p.subs[200]) >= 3
        for a, b in zip(alone.subs[0], p.subs[200]):
            assert a[:7] + a[8:] == b[:7] + b[8:] and b[7] == 200
        alone.close()
    p.close()


def test_noise(ctx):
    """20 000 Gaussian symbols: a state-0 attempt for about every 126 of them, none emitted, and the fault once."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal((20000, 2)).astype(np.float32)
    x[:, 1] = np.sign(x[:, 1]) * np.float32(1e-40)  # denormals keep their sign
    p = Pair(ctx, 2, 20000)
    res = p.run(x)
    assert res.counts.tolist() == [0, 0] and res.faults.tolist() == [1, 1] and not (res.sflags & abi.LNAV_S_OUTPUT).any()
    tried = p.dev.state(0)["subframes_tried"]
    assert tried == p.mod[0].subframes_tried and tried >= 100
    p.close()


def records_from(sym, valid, flags180, rng):
    """Tracking records whose valid entries carry the symbols as doubles that do not round-trip to float."""
    rec = np.zeros(sym.shape, abi.TRK_EPOCH_DTYPE)
    rec["prompt_i"] = sym.astype(np.float64) * (1.0 + rng.uniform(-2e-8, 2e-8, sym.shape))
    rec["prompt_q"] = rng.standard_normal(sym.shape)
    rec["flags"] = 8 | np.where(valid != 0, 1, 0) | (flags180.astype(np.int32) << 2)
    rec["sample_counter"] = (np.arange(sym.shape[0], dtype=np.uint64)[:, None] * np.uint64(80000) + np.uint64(1 << 33)
                             + np.arange(sym.shape[1], dtype=np.uint64)[None, :])
    return rec


def test_valid_masks_and_records(ctx):
    """Gaps in the validity mask, a whole chunk without an entry, and records from the host and from the device with
    flags & 4 seeding inverted (channel 1 carries an inverted stream and the flag)."""
    rng = np.random.default_rng(3)
    Cn, n = 4, 1000
    rounds = 2 * n
    bits, _ = M.five_subframes(5)
    valid = np.zeros((rounds, Cn), np.uint8)
    sym = rng.standard_normal((rounds, Cn)).astype(np.float32) * 9.0  # what sits in invalid entries must not matter
    streams = [C.tracked(bits, n), C.tracked(bits, n, -1.0), stream(n, 11), stream(n, 150, sign=-1.0)]
    for c in range(Cn):
        rows = np.sort(rng.choice(rounds, n, replace=False)) if c else np.arange(n)  # channel 0: nothing in the second half
        valid[rows, c] = 1
        sym[rows, c] = streams[c] * np.float32(1.0 + 0.25 * c)
    valid[1664:1728, 1:] = 0  # a whole chunk with no entry on three channels (their streams shorten)
    flags180 = np.zeros((rounds, Cn), np.uint8)
    flags180[:, 1] = 1
    flags180[5:, 2] = rng.integers(0, 2, rounds - 5)  # read only where the block seeds: the first symbol
    rec = records_from(sym, valid, flags180, rng)
    assert np.any(rec["prompt_i"].astype(np.float32).astype(np.float64) != rec["prompt_i"])
    narrowed = rec["prompt_i"].astype(np.float32)

    a = Pair(ctx, Cn, rounds)
    exp = a.expect(narrowed, valid, flags180, rec["sample_counter"])
    res_a = a.dev.run_symbols(narrowed, valid, flags180)
    for c in range(Cn):  # run_symbols reports no sample counter
        for r in exp[c][0]:
            r["sample_counter_rec"], r["sample_counter"] = r["sample_counter"], 0
    a.check(res_a, exp, "symbols")
    assert res_a.counts[0] == 3 and res_a.counts[1] >= 2 and res_a.counts.sum() >= 8
    assert res_a.subframes[1, 0]["symbol_counter"] == 300 and res_a.subframes[1, 0]["flags"] & abi.LNAV_PLL_180
    assert (res_a.tow_ms[valid == 0] == 0).all() and (res_a.sflags[valid == 0] == 0).all()
    for c in range(Cn):
        for r in exp[c][0]:
            r["sample_counter"] = r["sample_counter_rec"]

    b = Pair(ctx, Cn, rounds)
    b.mod = a.mod  # the models have consumed the stream once; the state comparison is the same
    b.check(b.dev.run_records(rec), exp, "host records")

    d = Pair(ctx, Cn, rounds)
    d.mod = a.mod
    buf = ctx.upload(rec.view(np.uint8).reshape(-1))
    d.check(d.dev.run_records(buf.ptr, on_device=True, n_rounds=rounds), exp, "device records")
    buf.free()
    for p in (a, b, d):
        p.close()


def test_zeros_and_nans(ctx):
    """A zero, a −0 or a NaN is a 0 bit under both polarities and positive in the correlation — exactly."""
    bits, _ = M.five_subframes(5)
    n = 700
    cols, f180 = [], []
    for sign in (1.0, -1.0):
        x = C.tracked(bits, n, sign)
        zero_bits = np.nonzero(np.concatenate(bits)[8:n + 8] == 0)[0]  # +1 when inverted, -1 when not: a 0 bit either way
        x[zero_bits[0::4]] = 0.0
        x[zero_bits[1::4]] = -0.0
        x[zero_bits[2::4]] = np.nan
        cols.append(x)
        f180.append(np.full(n, sign < 0, np.uint8))
    y = C.tracked(bits, n)
    y[292] = np.nan  # the second preamble's first symbol: still a hit, then a 0 bit in word 1
    cols.append(y)
    f180.append(np.ones(n, np.uint8))  # seeded inverted: the first subframe is not found, the second is met in state 0
    z = np.full(n, np.nan, np.float32)
    cols.append(z)
    f180.append(np.zeros(n, np.uint8))
    p = Pair(ctx, 4, n)
    res = p.run(np.stack(cols, axis=1), flags180=np.stack(f180, axis=1))
    assert res.counts.tolist() == [2, 2, 0, 0]
    assert p.dev.state(2)["preamble_index"] >= 600
    st = p.dev.state(3)  # NaNs are positive in the correlation: the only hit is the seeded preamble when it is the oldest
    assert st["subframes_tried"] == 1 and st["preamble_index"] == 300 and st["prev_word"] == 0
    p.close()


def test_corrupted_word10_lose_and_regain_tow0_and_the_densest_run(ctx):
    """The cases of tests/test_lnav_model.py on the device, one per channel: the previous word carried in state 1, loss of
    sync at the third failure and the re-sync in state 0, the TOW-0 subframe's stale stamp, IDs 0 / 7 / 6 with good
    parities, and the stream that emits the most records a run can (a loss, a state-0 success one symbol later)."""
    rng = np.random.default_rng(9)
    n = 2200
    ids = [M.build_subframe(sid, 500 + k, rng.integers(0, 2, 208))[0] for k, sid in enumerate((1, 0, 7, 6, 2))]
    cols = [C.tracked(C.corrupted_word10()[0], n), C.tracked(C.lose_and_regain(), n), C.tracked(C.tow0_case(), n), C.tracked(ids, n),
            C.densest_stream(3)[:n]]
    p = Pair(ctx, 5, 1200)
    x = np.stack(cols, axis=1)
    r1 = p.run(x[:1191], label="first")   # counter 1199: the next symbol of channel 4 is its loss of sync
    r2 = p.run(x[1191:], label="second")  # 1009 symbols
    assert r1.subframes[0]["parity_fail_mask"][:3].tolist() == [0, 1 << 9, 1]
    lost = [s for s in p.subs[1] if s[6] & abi.LNAV_SYNC_LOST]
    assert len(lost) == 1 and lost[0][0] == 1200 and lost[0][4] == 0
    assert [s[3] for s in p.subs[2][:3]] == [604794, 0, 6]
    assert [s[2] for s in p.subs[3][:3]] == [1, 0, 7] and not p.subs[3][1][6] & abi.LNAV_OK and p.subs[3][1][6] & abi.LNAV_PARITY_OK
    assert [s[0] - 1199 for s in p.subs[4][3:]] == [1, 2, 302, 602, 902, 903] and r2.counts[4] == 6 > 1009 // 300 + 2
    p.close()


def test_tlm_separation_and_channel_control(ctx):
    bits, _ = M.five_subframes(5)
    p = Pair(ctx, 4, 6000)
    ones = np.ones((6000, 4), np.float32)
    ones[:1000, 3] = C.tracked(bits, 1000)  # channel 3 decodes three subframes first: its bound moves
    assert p.run(ones[:5992]).faults.tolist() == [0, 0, 0, 0]  # the seeding counts 8
    assert p.run(ones[1000:1001]).faults.tolist() == [1, 1, 1, 0]  # the run that crosses the limit
    assert p.run(ones[1000:]).faults.tolist() == [0, 0, 0, 1]  # only once
    st3 = p.dev.state(3)
    assert st3["stat"] == 0 and st3["tow_set"] == 0 and st3["nav_tow_s"] == 6012
    p.dev.reset_channel(1)
    p.mod[1].reset()
    p.dev.set_satellite(3)
    p.mod[3].set_satellite()
    p.dev.new_channel(2)
    p.mod[2] = M.LnavDecoder()
    p.check_state("after control")
    assert p.dev.state(2) == M.LnavDecoder().state() and p.dev.state(3)["nav_tow_s"] == 0
    st = p.dev.state(1)
    assert st["history_size"] == 0 and st["last_valid_preamble"] == st["symbol_counter"] == 11001 and st["sent_tlm_failed"] == 0
    flat = np.ones((5992, 4), np.float32)
    assert p.run(flat).faults.tolist() == [0, 0, 0, 0]
    assert p.run(flat[:1]).faults.tolist() == [0, 1, 1, 0]
    # reset keeps the error counter, frame sync, the 180° flag and the previous word; the next symbol seeds again
    q = Pair(ctx, 1, 1000)
    x = C.tracked(C.lose_and_regain(), 2000, -1.0)
    q.run(x[:700], flags180=np.ones((700, 1), np.uint8))
    before = q.dev.state(0)
    assert before["crc_error_counter"] == 1 and before["pll_180"] == 1 and before["frame_sync"] == 1 and before["prev_word"] != 0
    q.dev.reset_channel(0)
    q.mod[0].reset()
    q.check_state("after reset")
    after = q.dev.state(0)
    for f in ("crc_error_counter", "pll_180", "frame_sync", "prev_word", "symbol_counter", "nav_tow_s", "tow_at_current_symbol_ms"):
        assert after[f] == before[f]
    res = q.run(x[1200:2000], flags180=np.ones((800, 1), np.uint8))  # from the symbol after the fifth subframe's preamble
    assert res.counts[0] == 2 and res.subframes[0, 0]["symbol_counter"] == 708 + 300
    for h in (p, q):
        h.close()


def test_rejected_calls(ctx):
    with pytest.raises(abi.GnssHipError) as e:
        engine.GpsL1CaTelemetryDecoder(ctx, 1, 0)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.GnssHipError) as e:
        engine.GpsL1CaTelemetryDecoder(ctx, 0, 10)
    assert e.value.code == abi.E_INVAL
    d = engine.gps_l1_ca_telemetry(ctx, 2, 10)
    d.run_symbols(np.ones((4, 2), np.float32))
    before = d.state(0)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_symbols(np.ones((11, 2), np.float32))
    assert e.value.code == abi.E_INVAL and b"max_rounds" in ctx.lib.gnsship_last_error(ctx.h)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_records(np.zeros((11, 2), abi.TRK_EPOCH_DTYPE))
    assert e.value.code == abi.E_INVAL
    for call in (d.reset_channel, d.set_satellite, d.new_channel, d.state):
        for ch in (-1, 2):
            with pytest.raises(abi.GnssHipError) as e:
                call(ch)
            assert e.value.code == abi.E_INVAL
    assert d.state(0) == before
    assert d.run_symbols(np.zeros((0, 2), np.float32)).counts.tolist() == [0, 0] and d.state(0) == before
    lib = ctx.lib
    assert lib.gnsship_lnav_run_symbols(None, None, None, None, 0, 0, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_lnav_run_trk(None, None, None, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_lnav_destroy(None) == abi.E_INVAL
    d.close()


def test_run_trk_in_place(ctx):
    """A short GPS tracking run (the signal carries the preamble the tracker synchronises on); its device records go
    through the decoder in place.  No subframe can appear in so short a run: the check is the state, the tow_ms / sflags
    stream, the equality with run_records and the model, and the tracker's own records left as they were."""
    import trk_scenarios as S
    from test_gpu_trk import dev_conf
    fs, rounds = 4e6, 400
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, rounds, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(72, sat.code)
    trk.start(0, 72, delay, dop, stamp, first)
    x = np.ascontiguousarray(x, np.complex64)
    buf = ctx.upload(x)
    in_place = engine.gps_l1_ca_telemetry(ctx, 1, rounds)
    with pytest.raises(abi.GnssHipError) as e:  # nothing launched yet
        in_place.run_trk(trk)
    assert e.value.code == abi.E_STATE
    trk.launch_ptr(buf.ptr, abi.FMT_CF32, first, len(x), rounds, records=True)
    got = in_place.run_trk(trk)  # before the collect
    rec, done = trk.collect()
    again = engine.gps_l1_ca_telemetry(ctx, 1, rounds)
    res = again.run_trk(trk)  # and after it
    other = engine.gps_l1_ca_telemetry(ctx, 1, rounds)
    ref = other.run_records(rec)
    wrong = engine.gps_l1_ca_telemetry(ctx, 2, rounds)
    with pytest.raises(abi.GnssHipError) as e:
        wrong.run_trk(trk)
    assert e.value.code == abi.E_INVAL
    small = engine.gps_l1_ca_telemetry(ctx, 1, 10)
    with pytest.raises(abi.GnssHipError) as e:
        small.run_trk(trk)
    assert e.value.code == abi.E_INVAL
    sel = (rec[:, 0]["flags"] & 1) != 0
    assert sel.sum() >= 5  # 20 ms symbols once the tracker has its bit synchronisation
    m = M.LnavDecoder()
    recs, fault, tow, sf = m.run(rec[sel, 0]["prompt_i"].astype(np.float32), rec[sel, 0]["sample_counter"], (rec[sel, 0]["flags"] & 4) != 0)
    assert not recs and not fault
    for r in (got, res, ref):
        assert r.counts[0] == 0 and r.faults[0] == 0
        n = r.tow_ms.shape[0]
        assert n >= done and np.array_equal(r.tow_ms[:done][sel[:done], 0], tow) and np.array_equal(r.sflags[:done][sel[:done], 0], sf)
        assert not r.sflags[:done][~sel[:done], 0].any()
    assert in_place.state(0) == other.state(0) == again.state(0) == m.state()
    assert m.state()["history_size"] == 8 + int(sel.sum())
    # the tracker's records are what a tracker without a decoder behind it gives
    plain = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    plain.start(0, 72, delay, dop, stamp, first)
    rec_plain, done_plain = plain.run(x, first, rounds)
    assert done_plain == done and rec_plain.tobytes() == rec.tobytes()
    plain.close()
    for h in (in_place, again, other, wrong, small, trk):
        h.close()
    buf.free()
