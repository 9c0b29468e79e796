"""The device Galileo telemetry framing (tlm_galileo.hip, gnsship_tlm_*) against the numpy restatement of
galileo_telemetry_decoder_gs::general_work in tests/tlm_model.py.

Contract: exact equality — pages (symbol counter, sample counter, channel, flags, CRC-error counter), bits, counts,
faults and every member of gnsship_tlm_state — for each frame type, both Viterbi modes, both polarities, any cut of a
stream into runs, any number of channels, validity masks and tracking records (host, device, in place)."""
import numpy as np
import pytest

import tlm_model as M
import viterbi_model as V
from gnss_sim_receiver_amd import abi, engine, signals

pytestmark = pytest.mark.gpu

FT = {"inav": M.INAV, "fnav": M.FNAV, "cnav": M.CNAV}
MODES = {"reference": V.REFERENCE, "full": V.FULL}
STATE_FIELDS = ["symbol_counter", "preamble_index", "last_valid_preamble", "stat", "crc_error_counter", "history_size", "pll_180",
                "frame_sync", "even_word_arrived", "flag_crc_test", "sent_tlm_failed"]


def stream(ft, n, lead, seed=5):
    return M.build_stream(ft, M.four_parts(ft, seed), n, lead, seed + 1)


def length_for(ft, n_parts, lead):
    g = M.GEOMETRY[ft]
    return lead + g.required + 1 + (1 + n_parts) * g.period + 7


class Pair:
    """A device decoder and one model object per channel, fed the same runs and compared after each."""

    def __init__(self, ctx, ft, channels, max_rounds, mode="reference"):
        self.ft, self.C = ft, channels
        self.dev = engine.GalileoTelemetryDecoder(ctx, ft, channels, max_rounds, mode)
        self.mod = [M.TlmDecoder(ft, MODES[mode]) for _ in range(channels)]
        self.pages = [[] for _ in range(channels)]  # everything emitted so far, per channel: (page record fields, bits)

    def close(self):
        self.dev.close()

    def expect(self, sym, valid=None, sample_counters=None):
        """Run the models over sym[n_rounds, C] and return what the device must give."""
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        out, ran = [], {}
        for c, m in enumerate(self.mod):
            sel = np.ones(sym.shape[0], bool) if valid is None else valid[:, c] != 0
            sc = None if sample_counters is None else sample_counters[sel, c]
            if id(m) in ran:  # channels given the same stream may share one model object
                first = ran[id(m)]
                assert np.array_equal(sym[sel, c], sym[:, first]) and valid is None and sc is None
                out.append(out[first])
                continue
            ran[id(m)] = c
            out.append(m.run(sym[sel, c], sc))
        return out

    def check(self, res, exp, label=""):
        assert res.counts.tolist() == [len(p) for p, _ in exp], (label, res.counts.tolist())
        assert res.faults.tolist() == [int(f) for _, f in exp], (label, res.faults.tolist())
        for c, (pages, _) in enumerate(exp):
            assert len(pages) <= self.dev.pages_per_run
            for k, p in enumerate(pages):
                got = res.pages[c, k]
                want = (p["symbol_counter"], p["sample_counter"], c, p["flags"], p["crc_error_counter"])
                have = tuple(int(got[f]) for f in ("symbol_counter", "sample_counter", "channel", "flags", "crc_error_counter"))
                assert have == want, (label, c, k, have, want)
                assert np.array_equal(res.bits[c, k], p["bits"]), (label, c, k)
                self.pages[c].append((have, res.bits[c, k].copy()))
        self.check_state(label)

    def check_state(self, label="", channels=None):
        for c in (range(self.C) if channels is None else channels):
            got, want = self.dev.state(c), self.mod[c].state()
            assert [got[f] for f in STATE_FIELDS] == [want[f] for f in STATE_FIELDS], (label, c, got, want)

    def run(self, sym, valid=None, label=""):
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        res = self.dev.run_symbols(sym, valid)
        self.check(res, self.expect(sym, valid), label)
        return res


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("mode", ["reference", "full"])
@pytest.mark.parametrize("name", ["inav", "fnav", "cnav"])
def test_device_equals_model(ctx, name, mode, sign):
    ft = FT[name]
    n = length_for(ft, 3, 41)
    x = np.float32(sign) * stream(ft, n, 41)
    p = Pair(ctx, ft, 1, n, mode)
    res = p.run(x)
    assert res.counts[0] == 3
    parts = M.four_parts(ft, 5)
    for k in range(3):  # noiseless: the bits are those built, whatever the mode and the polarity
        assert np.array_equal(res.bits[0, k], parts[(2 + k) % 4])
        assert bool(res.pages[0, k]["flags"] & abi.TLM_PLL_180) == (sign < 0)
    assert res.pages[0, 2]["flags"] & abi.TLM_CRC_OK
    p.close()


@pytest.mark.parametrize("cut", [1, 7, 249, 250, 251, 600])
def test_cuts_give_identical_outputs(ctx, cut):
    """The same I/NAV stream in runs of `cut` symbols: straddling the due symbol and the 64-symbol chunk."""
    n = 1300 if cut == 1 else 1800
    x = stream(M.INAV, n, 29)
    whole = Pair(ctx, M.INAV, 1, n)
    whole.run(x)
    p = Pair(ctx, M.INAV, 1, cut)
    for k in range(0, n, cut):
        p.run(x[k:k + cut], label=f"run at {k}")
    assert len(p.pages[0]) == len(whole.pages[0]) >= 1
    for a, b in zip(p.pages[0], whole.pages[0]):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert p.dev.state(0) == whole.dev.state(0)
    whole.close()
    p.close()


@pytest.mark.parametrize("channels", [1, 5, 257])
def test_channels_with_different_lead_ins(ctx, channels):
    """Pages fall due at different symbols; in the second run some channels emit none, one or two parts."""
    n = 1500
    leads = [(3 + 197 * (c % 32)) % 600 for c in range(channels)]  # 32 lead-ins: the model runs once per distinct stream
    distinct = [stream(M.INAV, n, leads[c], seed=5 + c % 3) for c in range(min(channels, 32))]
    x = np.stack([distinct[c % 32] for c in range(channels)], axis=1)
    p = Pair(ctx, M.INAV, channels, 1200)
    p.mod = [p.mod[c % 32] for c in range(channels)]
    p.run(x[:1200], label="first")
    res = p.run(x[1200:], label="second")
    if channels > 1:
        assert set(res.counts.tolist()) == {0, 1, 2}
    if channels == 257:  # a channel among 256 others equals the channel alone
        alone = Pair(ctx, M.INAV, 1, 1200)
        alone.run(x[:1200, 200])
        alone.run(x[1200:, 200])
        assert len(alone.pages[0]) == len(p.pages[200]) >= 1
        for a, b in zip(alone.pages[0], p.pages[200]):
            assert a[0][:2] + a[0][3:] == b[0][:2] + b[0][3:] and np.array_equal(a[1], b[1])
        alone.close()
    p.close()


def records_from(sym, valid, rng):
    """Tracking records whose valid entries carry the symbols as doubles that do not round-trip to float."""
    rec = np.zeros(sym.shape, abi.TRK_EPOCH_DTYPE)
    rec["prompt_i"] = sym.astype(np.float64) * (1.0 + rng.uniform(-2e-8, 2e-8, sym.shape))
    rec["prompt_q"] = rng.standard_normal(sym.shape)
    rec["flags"] = 8 | np.where(valid != 0, 1, 0) | (rng.integers(0, 2, sym.shape) << 2)
    rec["sample_counter"] = (np.arange(sym.shape[0], dtype=np.uint64)[:, None] * np.uint64(16000) + np.uint64(1 << 33)
                             + np.arange(sym.shape[1], dtype=np.uint64)[None, :])
    return rec


def test_valid_masks_and_records(ctx):
    rng = np.random.default_rng(3)
    C, n = 4, 1500
    rounds = 2 * n
    valid = np.zeros((rounds, C), np.uint8)
    sym = rng.standard_normal((rounds, C)).astype(np.float32) * 9.0  # what sits in invalid entries must not matter
    streams = [stream(M.INAV, n, 11 + 50 * c) * np.float32(1.0 + 0.25 * c) for c in range(C)]
    for c in range(C):
        rows = np.sort(rng.choice(rounds, n, replace=False)) if c else np.arange(n)  # channel 0: nothing in the second half
        valid[rows, c] = 1
        sym[rows, c] = streams[c]
    valid[100:164, 1:] = 0  # a whole chunk with no entry on three channels (their streams shorten)
    rec = records_from(sym, valid, rng)
    assert np.any(rec["prompt_i"].astype(np.float32).astype(np.float64) != rec["prompt_i"])
    narrowed = rec["prompt_i"].astype(np.float32)

    a = Pair(ctx, M.INAV, C, rounds)
    exp = a.expect(narrowed, valid, rec["sample_counter"])
    res_a = a.dev.run_symbols(narrowed, valid)
    for c in range(C):  # run_symbols reports no sample counter
        for pg in exp[c][0]:
            pg["sample_counter_rec"], pg["sample_counter"] = pg["sample_counter"], 0
    a.check(res_a, exp, "symbols")
    assert res_a.counts.sum() >= 4
    for c in range(C):
        for pg in exp[c][0]:
            pg["sample_counter"] = pg["sample_counter_rec"]

    b = Pair(ctx, M.INAV, C, rounds)
    b.mod = a.mod  # the models have consumed the stream once; the state comparison is the same
    b.check(b.dev.run_records(rec), exp, "host records")

    d = Pair(ctx, M.INAV, C, rounds)
    d.mod = a.mod
    buf = ctx.upload(rec.view(np.uint8).reshape(-1))
    d.check(d.dev.run_records(buf.ptr, on_device=True, n_rounds=rounds), exp, "device records")
    buf.free()
    for p in (a, b, d):
        p.close()


@pytest.mark.parametrize("where", ["last", "first"])
def test_due_symbol_at_the_edge_of_a_run(ctx, where):
    lead = 17
    g = M.GEOMETRY[M.INAV]
    due = lead + g.required + 1 + 2 * g.period  # symbols up to and including the first due one
    x = stream(M.INAV, due + 300, lead)
    p = Pair(ctx, M.INAV, 1, due + 300)
    cut = due if where == "last" else due - 1
    r1 = p.run(x[:cut])
    r2 = p.run(x[cut:cut + 1])
    assert (r1.counts[0], r2.counts[0]) == ((1, 0) if where == "last" else (0, 1))
    p.run(x[cut + 1:])
    p.close()


def test_two_parts_in_one_run(ctx):
    lead = 23
    g = M.GEOMETRY[M.INAV]
    due = lead + g.required + 1 + 2 * g.period
    x = stream(M.INAV, due + 700, lead)
    p = Pair(ctx, M.INAV, 1, 600)
    assert p.dev.pages_per_run == 3
    k = due - 40
    for a in range(0, k, 600):
        p.run(x[a:min(a + 600, k)])
    res = p.run(x[k:k + 600])
    assert res.counts[0] == 3 and res.pages[0]["symbol_counter"].tolist() == [due, due + 250, due + 500]
    p.close()


def test_corrupted_parts_lose_and_regain_sync(ctx):
    """One data symbol flipped in each of seven consecutive parts, then clean."""
    ft, lead = M.INAV, 31
    g = M.GEOMETRY[ft]
    n = lead + 26 * g.period
    x = stream(ft, n, lead).copy()
    for k in range(4, 11):  # stream parts 4..10: the first two emitted parts are clean
        x[lead + k * g.period + g.P + 8 * 3] *= -1.0  # row 0, column 24: de-interleaved position 192, a first symbol of its pair
    p = Pair(ctx, ft, 1, n)
    res = p.run(x)
    flags = res.pages[0]["flags"][:res.counts[0]]
    assert np.count_nonzero(flags & abi.TLM_SYNC_LOST) == 1  # and where, and the re-sync instant: equal to the model's (Pair.check)
    lost = int(np.nonzero(flags & abi.TLM_SYNC_LOST)[0][0])
    assert not flags[lost] & abi.TLM_FRAME_SYNC and res.counts[0] > lost + 1 and flags[res.counts[0] - 1] & abi.TLM_FRAME_SYNC
    p.close()


@pytest.mark.parametrize("name,limit", [("inav", 15000), ("fnav", 2500)])
def test_tlm_separation(ctx, name, limit):
    ft = FT[name]
    p = Pair(ctx, ft, 3, limit)
    ones = np.ones((limit, 3), np.float32)
    assert p.run(ones).faults.tolist() == [0, 0, 0]
    assert p.run(ones[:1]).faults.tolist() == [1, 1, 1]  # the run that crosses the limit
    assert p.run(ones[:limit]).faults.tolist() == [0, 0, 0]  # only once
    p.dev.reset_channel(1)
    p.mod[1].reset()
    p.check_state("after reset")
    assert p.run(ones[:limit]).faults.tolist() == [0, 0, 0]
    assert p.run(ones[:1]).faults.tolist() == [0, 1, 0]
    p.dev.set_satellite(2)
    p.mod[2].set_satellite()
    p.run(ones[:limit])
    assert p.run(ones[:1]).faults.tolist() == [0, 0, 1]
    p.close()


def test_channel_control(ctx):
    """reset_channel keeps the history, the counters, the stored even part and the sticky CRC flag; new_channel does not."""
    lead = 19
    g = M.GEOMETRY[M.INAV]
    n = length_for(M.INAV, 6, lead)
    x = stream(M.INAV, n, lead)
    p = Pair(ctx, M.INAV, 3, n)
    xs = np.stack([x, x, x], axis=1)
    k = lead + g.required + 1 + 3 * g.period + 100  # two parts emitted (even, odd: flag_crc_test set), mid-part
    p.run(xs[:k])
    assert p.dev.state(0)["flag_crc_test"] == 1 and p.dev.state(0)["stat"] == 2
    p.dev.reset_channel(0)
    p.mod[0].reset()
    p.dev.new_channel(1)
    p.mod[1] = M.TlmDecoder(M.INAV)
    p.dev.set_satellite(2)
    p.mod[2].set_satellite()
    p.check_state("after control")
    st = p.dev.state(0)
    assert st["stat"] == 0 and st["flag_crc_test"] == 1 and st["history_size"] == g.required + 1 and st["symbol_counter"] == k
    assert p.dev.state(1) == M.TlmDecoder(M.INAV).state()
    res = p.run(xs[k:])  # the kept history lets channel 0 re-synchronise at once; channel 1 starts over
    assert res.counts[0] >= 1 and res.counts[2] > res.counts[0] and res.counts[1] < res.counts[2]
    assert res.pages[0, 0]["flags"] & abi.TLM_CRC_OK  # sticky: the first part after the reset reports the old verdict
    p.close()


def test_rejected_calls(ctx):
    with pytest.raises(abi.GnssHipError) as e:
        engine.GalileoTelemetryDecoder(ctx, 4, 1, 10)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.GnssHipError) as e:
        engine.GalileoTelemetryDecoder(ctx, abi.TLM_INAV, 1, 10, mode=7)
    assert e.value.code == abi.E_INVAL
    with pytest.raises(abi.GnssHipError) as e:
        engine.GalileoTelemetryDecoder(ctx, abi.TLM_INAV, 1, 0)
    assert e.value.code == abi.E_INVAL
    d = engine.galileo_inav_telemetry(ctx, 2, 10)
    d.run_symbols(np.ones((4, 2), np.float32))
    before = d.state(0)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_symbols(np.ones((11, 2), np.float32))
    assert e.value.code == abi.E_INVAL and b"max_rounds" in ctx.lib.gnsship_last_error(ctx.h)
    for call in (d.reset_channel, d.set_satellite, d.new_channel, d.state):
        for ch in (-1, 2):
            with pytest.raises(abi.GnssHipError) as e:
                call(ch)
            assert e.value.code == abi.E_INVAL
    assert d.state(0) == before
    lib = ctx.lib
    assert lib.gnsship_tlm_run_symbols(None, None, None, 0, 0, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_tlm_run_trk(None, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_tlm_destroy(None) == abi.E_INVAL
    d.close()


def test_end_to_end_e1_and_run_trk(ctx):
    """One Galileo E1 satellite at 4 Msps, 50 dB-Hz, 8-bit samples, 7.5 s generated on the device, four built I/NAV parts
    cycling on E1-B; tracked from truth; the tracker's device records go through the decoder in place (run_trk), which
    equals run_records on the collected records and the model on their prompts; the parts decode with good CRCs."""
    import torch
    from oracle import trk as T
    from test_gpu_trk import dev_conf
    fs, vl = 4e6, 16000
    parts = M.four_parts(M.INAV, 21)
    symbols = np.concatenate([M.build_part(M.INAV, b) for b in parts])
    bits = "".join("0" if s > 0 else "1" for s in symbols)
    sat = signals.Satellite(prn=11, doppler_hz=1210.0, code_delay_chips=100.3, cn0_dbhz=50.0, system="GAL", carrier_phase_rad=1.0,
                            secondary=T.E1C_SECONDARY, bits=bits)
    first = int(fs)
    rounds = 1875
    n = (rounds + 4) * vl
    x = signals.generate_if_device(fs, n, [sat], seed=0x6E550031, start=first, device="cuda")
    raw = signals.to_ibyte(x.cpu().numpy())
    del x
    torch.cuda.empty_cache()
    k = T.conf("GAL", fs, vl, pull_in_time_s=0, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GAL"), 1)
    ctx.set_code(70, sat.code)
    ctx.set_code(71, sat.code_data)
    trk.start(0, 70, signals.acq_delay_samples(sat, fs, 0, first), sat.doppler_hz, 0, first, data_code_id=71, prn=sat.prn)
    buf = ctx.upload(raw)
    in_place = engine.galileo_inav_telemetry(ctx, 1, rounds)
    with pytest.raises(abi.GnssHipError) as e:  # nothing launched yet
        in_place.run_trk(trk)
    assert e.value.code == abi.E_STATE
    trk.launch_ptr(buf.ptr, abi.FMT_CI8, first, len(raw), rounds, records=True)
    got = in_place.run_trk(trk)  # before the collect
    rec, done = trk.collect()
    assert done >= rounds - 2
    again = engine.galileo_inav_telemetry(ctx, 1, rounds)
    res = again.run_trk(trk)  # and after it
    other = engine.galileo_inav_telemetry(ctx, 1, rounds)
    ref = other.run_records(rec)
    wrong = engine.galileo_inav_telemetry(ctx, 2, rounds)
    with pytest.raises(abi.GnssHipError) as e:
        wrong.run_trk(trk)
    assert e.value.code == abi.E_INVAL
    for r in (got, res):
        assert r.counts[0] == ref.counts[0] and r.faults[0] == ref.faults[0]
        assert np.array_equal(r.pages[0, :r.counts[0]], ref.pages[0, :r.counts[0]])
        assert np.array_equal(r.bits[0, :r.counts[0]], ref.bits[0, :r.counts[0]])
    assert in_place.state(0) == other.state(0) == again.state(0)
    # the model on the valid prompts
    sel = (rec[:, 0]["flags"] & 1) != 0
    m = M.TlmDecoder(M.INAV)
    pages, fault = m.run(rec[sel, 0]["prompt_i"].astype(np.float32), rec[sel, 0]["sample_counter"])
    assert ref.counts[0] == len(pages) >= 2 and not fault
    for i, pg in enumerate(pages):
        assert int(ref.pages[0, i]["symbol_counter"]) == pg["symbol_counter"] and int(ref.pages[0, i]["sample_counter"]) == pg["sample_counter"]
        assert int(ref.pages[0, i]["flags"]) == pg["flags"] and np.array_equal(ref.bits[0, i], pg["bits"])
        assert any(np.array_equal(pg["bits"], b) for b in parts), i  # 50 dB-Hz: every part decodes to one of those built
    assert any(pg["flags"] & M.F_CRC_EVALUATED and pg["flags"] & M.F_CRC_OK for pg in pages)
    assert other.state(0) == {**m.state()}
    for h in (in_place, again, other, wrong, trk):
        h.close()
    buf.free()
