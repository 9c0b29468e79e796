"""The device BeiDou D1/D2 telemetry decoder (tlm_bds_dnav.hip, gnsship_dnav_*) against the restatement of
beidou_b1i_telemetry_decoder_gs / beidou_b3i_telemetry_decoder_gs in tests/dnav_model.py.

Contract: exact equality — every field of every subframe record, every tow_ms / sflags entry, counts and every member of
gnsship_dnav_state — for both signals and polarities, D1, D2 and the B3I split case, any cut of a stream into runs, any
number of channels, validity and output-valid masks, tracking records (host, device, in place), zeros and NaNs, and every
15-bit input of the BCH decoder.  No run is longer than 1300 symbols."""
import numpy as np
import pytest

import dnav_model as M
import test_dnav_model as C
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

REC_FIELDS = ["symbol_counter", "sample_counter", "fra_id", "pnum", "sow", "corrected_mask", "tow_at_current_symbol_ms", "flags"]


class Pair:
    """A device decoder and one model object per channel, fed the same runs and compared after each."""

    def __init__(self, ctx, signal, prns, max_rounds):
        self.C = len(prns)
        self.dev = engine.BeidouDnavTelemetryDecoder(ctx, self.C, max_rounds, signal)
        assert self.dev.subframes_per_run == M.subframes_per_run(max_rounds) == abi.dnav_subframes_per_run(max_rounds)
        self.mod = []
        for c, prn in enumerate(prns):
            if prn:  # PRN 0: the object as gnsship_dnav_create left it
                self.dev.new_channel(c, prn)
            self.mod.append(M.Decoder(signal, prn, c))
        self.subs = [[] for _ in prns]  # everything emitted so far, per channel
        self.tow = [[] for _ in prns]   # (tow_ms, sflags) of every run so far, per channel

    def close(self):
        self.dev.close()

    def expect(self, sym, valid=None, out_valid=None, sample_counters=None):
        """Run the models over sym[n_rounds, C]: per channel (records, tow_ms[n_rounds], sflags[n_rounds])."""
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        out, ran = [], {}
        for c, m in enumerate(self.mod):
            if id(m) in ran:  # channels given the same stream may share one model object
                first = ran[id(m)]
                assert valid is None and out_valid is None and sample_counters is None
                assert np.array_equal(sym[:, c], sym[:, first], equal_nan=True)
                out.append(out[first])
                continue
            ran[id(m)] = c
            col = lambda a: None if a is None else np.asarray(a)[:, c:c + 1]
            recs, tow, sf = M.run([m], sym[:, c:c + 1], col(valid), col(out_valid), col(sample_counters))
            out.append((recs[0], tow[:, 0], sf[:, 0]))
        return out

    def check(self, res, exp, label=""):
        assert res.counts.tolist() == [len(e[0]) for e in exp], (label, res.counts.tolist())
        for c, (recs, tow, sf) in enumerate(exp):
            assert len(recs) <= self.dev.subframes_per_run
            for k, r in enumerate(recs):
                got = res.subframes[c, k]
                have = tuple(int(got[f]) for f in REC_FIELDS) + (int(got["channel"]),) + tuple(int(w) for w in got["words"])
                want = tuple(int(r[f]) for f in REC_FIELDS) + (c,) + tuple(r["words"])
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

    def run(self, sym, valid=None, out_valid=None, label=""):
        sym = np.asarray(sym, np.float32).reshape(-1, self.C)
        res = self.dev.run_symbols(sym, valid, out_valid)
        self.check(res, self.expect(sym, valid, out_valid), label)
        return res

    def reset(self, c):
        self.dev.reset_channel(c)
        self.mod[c].reset()

    def set_satellite(self, c, prn):
        self.dev.set_satellite(c, prn)
        self.mod[c].set_satellite(prn)


def build(d2, specs, lead=0, inverted=False, seed=1, amplitude=1.0):
    """lead symbols of +1, the subframes of specs [(FraID, Pnum, SOW), ...] with random payloads, eleven symbols of +1."""
    rng = np.random.default_rng(seed)
    subs = [M.build_subframe(d2, f, p, s, rng.integers(0, 2, 182))[1] for f, p, s in specs]
    x = np.concatenate([np.ones(lead, np.float32), M.stream(subs, inverted=inverted), np.ones(11, np.float32)])
    return x * np.float32(amplitude)


def clean(signal, prn, lead=0, inverted=False, n_sub=4, sow0=345600, seed=1):
    """The clean stream of tests/test_dnav_model.py that suits the decoder the block picks for this PRN."""
    f = C.d2_stream if M.is_d2_decoder(signal, prn) else C.d1_stream
    return f(lead, n_sub, sow0, inverted, seed)


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("lead", [0, 37])
@pytest.mark.parametrize("prn", [20, 3, 60])
@pytest.mark.parametrize("signal", [M.B1I, M.B3I])
def test_device_equals_model(ctx, signal, prn, lead, inverted):
    """D1 (PRN 20), D2 (PRN 3) and PRN 60 — D2 on B1I, the D1 decoder with 2 ms symbols on B3I, where the D1 stream's
    6-second steps then contradict the clock and zero the TOW."""
    x = clean(signal, prn, lead, inverted)
    assert len(x) == 1211 + lead
    p = Pair(ctx, signal, [prn], len(x))
    res = p.run(x)
    assert res.counts[0] == 3 and res.subframes[0]["symbol_counter"][:3].tolist() == [611 + lead, 911 + lead, 1211 + lead]
    flags = res.subframes[0]["flags"][:3]
    assert all(bool(f & abi.DNAV_INVERTED) == inverted for f in flags)
    assert flags[0] & abi.DNAV_STATE1 and not flags[1] & abi.DNAV_STATE1
    split = signal == M.B3I and prn == 60
    assert bool(flags[0] & abi.DNAV_D2_DECODER) == (prn == 3 or (prn == 60 and not split))
    assert bool(flags[0] & abi.DNAV_D2_TIMING) == (prn != 20)
    assert bool(flags[1] & abi.DNAV_TOW_ZEROED) == split
    d = 20 if prn == 20 else 2
    assert res.tow_ms[610 + lead, 0] == (res.subframes[0, 0]["sow"] + 14) * 1000 + 311 * d
    assert res.sflags[610 + lead, 0] == abi.DNAV_S_VALID_WORD | abi.DNAV_S_SUBFRAME | (abi.DNAV_S_INVERTED if inverted else 0)
    assert not res.sflags[:610 + lead, 0].any() and not res.tow_ms[:610 + lead, 0].any()
    p.close()


@pytest.mark.parametrize("cut", [1, 7, 63, 64, 65, 299, 300, 301, 311, 600])
def test_cuts_give_identical_outputs(ctx, cut):
    """The same stream in runs of `cut` symbols: the 64-entry chunk boundary, the due symbol and the history's capacity at
    a cut, and a reset between two runs (the TOW and valid_word go, the state and the history stay)."""
    x = clean(M.B3I, 20, 23)[:1000 if cut == 1 else 1300]
    n = len(x)
    reset_at = 700 // cut * cut if cut <= 700 else cut  # a run boundary at or near the first decode (634)
    whole = Pair(ctx, M.B3I, [20], n)
    whole.run(x[:reset_at])
    whole.reset(0)
    whole.run(x[reset_at:])
    p = Pair(ctx, M.B3I, [20], cut)
    for k in range(0, n, cut):
        if k == reset_at:
            p.reset(0)
        p.run(x[k:k + cut], label=f"run at {k}")
    assert p.subs[0] == whole.subs[0] and len(whole.subs[0]) >= 2
    for i in (0, 1):
        assert np.array_equal(np.concatenate([t[i] for t in p.tow[0]]), np.concatenate([t[i] for t in whole.tow[0]]))
    assert p.dev.state(0) == whole.dev.state(0)
    whole.close()
    p.close()


@pytest.mark.parametrize("channels", [1, 5, 257])
def test_channels_with_different_lead_ins(ctx, channels):
    """Subframes fall due at different symbols of a run; B1I, D2 and D1 channels side by side."""
    leads = [(3 + 61 * (c % 32)) % 89 for c in range(channels)]  # 32 lead-ins: the model runs once per distinct stream
    prns = [(3, 20, 60)[c % 3] for c in range(min(channels, 32))]
    distinct = [clean(M.B1I, prns[c], leads[c], inverted=bool(c % 2), seed=5 + c % 3)[:1211] for c in range(min(channels, 32))]
    x = np.stack([distinct[c % 32] for c in range(channels)], axis=1)
    p = Pair(ctx, M.B1I, [prns[c % 32] for c in range(channels)], 900)
    p.mod = [p.mod[c % 32] for c in range(channels)]
    first = p.run(x[:900], label="first")
    second = p.run(x[900:], label="second")  # 311 symbols
    assert set(first.counts.tolist()) == {1} and set(second.counts.tolist()) <= {1, 2}  # 2: the lead-in of 0, due at 1211 too
    if channels > 1:
        assert len(set(second.subframes[:, 0]["symbol_counter"].tolist())) == min(channels, 32)
    if channels == 257:  # a channel among 256 others equals the channel alone
        alone = Pair(ctx, M.B1I, [prns[200 % 32]], 900)
        for part in (x[:900, 200], x[900:, 200]):
            alone.run(part)
        assert len(alone.subs[0]) == len(p.subs[200]) >= 2
        for a, b in zip(alone.subs[0], p.subs[200]):
            assert a[:8] + a[9:] == b[:8] + b[9:] and b[8] == 200
        alone.close()
    p.close()


def records_from(sym, valid, rng):
    """Tracking records whose valid entries carry the symbols as doubles that do not round-trip to float."""
    rec = np.zeros(sym.shape, abi.TRK_EPOCH_DTYPE)
    rec["prompt_i"] = sym.astype(np.float64) * (1.0 + rng.uniform(-2e-8, 2e-8, sym.shape))
    rec["prompt_q"] = rng.standard_normal(sym.shape)
    rec["flags"] = 8 | np.where(valid != 0, 1, 0)
    rec["sample_counter"] = (np.arange(sym.shape[0], dtype=np.uint64)[:, None] * np.uint64(80000) + np.uint64(1 << 33)
                             + np.arange(sym.shape[1], dtype=np.uint64)[None, :])
    return rec


def test_valid_masks_out_valid_and_records(ctx):
    """Gaps in the validity mask, a whole chunk without an entry, output-valid flags that drop valid_word (one of them on
    a decode's own symbol is not looked at when the stamp runs; one right behind it is), and the same entries as records
    from the host and from the device."""
    rng = np.random.default_rng(3)
    prns = [20, 3, 60, 20]
    n, rounds = 1211, 1300
    valid = np.zeros((rounds, 4), np.uint8)
    sym = rng.standard_normal((rounds, 4)).astype(np.float32) * 9.0  # what sits in invalid entries must not matter
    rows_of = []
    for c in range(4):
        rows = np.sort(rng.choice(rounds, n, replace=False)) if c else np.arange(n)  # channel 0: nothing behind its stream
        if c == 3:
            rows = np.concatenate([np.arange(600), np.arange(664, 664 + 611)])  # a whole chunk with no entry
        valid[rows, c] = 1
        sym[rows, c] = clean(M.B3I, prns[c], 0, inverted=c == 1, seed=3 + c)[:n] * np.float32(1.0 + 0.25 * c)
        rows_of.append(rows)
    out_valid = np.ones((rounds, 4), np.uint8)
    out_valid[rows_of[0][610], 0] = 0   # the first decode's own symbol: the stamp does not look
    out_valid[rows_of[0][700], 0] = 0   # valid_word falls here and the TOW stops; the next stamp (911) disagrees with the
                                        # stopped clock and zeroes it, the one after (1211) is accepted
    out_valid[rows_of[1][611], 1] = 0   # right behind the stamp
    out_valid[rows_of[2][400], 2] = 0   # while valid_word is false: nothing
    out_valid[rows_of[3][909:913], 3] = 0  # around a decode (911) whose stamp brings valid_word back

    a = Pair(ctx, M.B3I, prns, rounds)
    exp = a.expect(sym, valid, out_valid)
    res = a.dev.run_symbols(sym, valid, out_valid)
    a.check(res, exp, "symbols")
    assert res.counts.tolist() == [3, 3, 3, 3]
    assert (res.tow_ms[valid == 0] == 0).all() and (res.sflags[valid == 0] == 0).all()
    r0 = rows_of[0]
    assert res.sflags[r0[610], 0] & abi.DNAV_S_VALID_WORD and res.sflags[r0[699], 0] & abi.DNAV_S_VALID_WORD
    assert not res.sflags[r0[700]:r0[909] + 1, 0].any() and res.tow_ms[r0[800], 0] == res.tow_ms[r0[700], 0] != 0
    assert res.sflags[r0[910], 0] == abi.DNAV_S_SUBFRAME and res.tow_ms[r0[910], 0] == 0 and res.subframes[0, 1]["flags"] & abi.DNAV_TOW_ZEROED
    assert res.sflags[r0[1210], 0] == abi.DNAV_S_SUBFRAME | abi.DNAV_S_VALID_WORD
    assert not res.sflags[rows_of[1][611], 1] & abi.DNAV_S_VALID_WORD and res.sflags[rows_of[1][610], 1] & abi.DNAV_S_VALID_WORD
    assert res.sflags[rows_of[3][910], 3] & abi.DNAV_S_VALID_WORD and not res.sflags[rows_of[3][911], 3] & abi.DNAV_S_VALID_WORD

    # records: the output-valid flag of a record entry is true
    rec = records_from(sym, valid, rng)
    assert np.any(rec["prompt_i"].astype(np.float32).astype(np.float64) != rec["prompt_i"])
    narrowed = rec["prompt_i"].astype(np.float32)
    b = Pair(ctx, M.B3I, prns, rounds)
    exp = b.expect(narrowed, valid, None, rec["sample_counter"])
    b.check(b.dev.run_records(rec), exp, "host records")
    assert b.dev.run_records(rec[:0]).counts.tolist() == [0, 0, 0, 0]
    d = Pair(ctx, M.B3I, prns, rounds)
    d.mod = b.mod  # the models have consumed the stream once; the state comparison is the same
    buf = ctx.upload(rec.view(np.uint8).reshape(-1))
    d.check(d.dev.run_records(buf.ptr, on_device=True, n_rounds=rounds), exp, "device records")
    buf.free()
    assert exp[1][0][0]["sample_counter"] == rec["sample_counter"][rows_of[1][610], 1]
    # floats on the device
    s = Pair(ctx, M.B3I, prns, rounds)
    s.mod = a.mod
    bufs = [ctx.upload(np.ascontiguousarray(v).view(np.uint8).reshape(-1)) for v in (sym, valid, out_valid)]
    res_d = s.dev.run_symbols(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, on_device=True, n_rounds=rounds)
    assert res_d.subframes.tobytes() == res.subframes.tobytes() and np.array_equal(res_d.tow_ms, res.tow_ms)
    assert np.array_equal(res_d.sflags, res.sflags) and res_d.counts.tolist() == res.counts.tolist()
    s.check_state("device symbols")
    for bf in bufs:
        bf.free()
    for p in (a, b, d, s):
        p.close()


def test_polarity_edge_zeros_and_nans(ctx):
    """A state-2 subframe whose preamble is corrupted so that corr <= 0 is decoded inverted; +0, −0 and NaN are positive in
    the correlation and a −1 bit under both polarities, in the preamble window and in the payload."""
    cols = []
    x = clean(M.B1I, 20)
    x[600:606] = -x[600:606]  # six of eleven: corr −1 at 911
    cols.append(x)
    x = clean(M.B1I, 20)
    x[900:911] = -x[900:911]  # the whole preamble: corr −11 at 1211, inverted as well
    cols.append(x)
    for inverted in (False, True):
        x = clean(M.B1I, 20, inverted=inverted)
        ones = np.nonzero(np.array(M.PREAMBLE) > 0)[0]  # the preamble's '1's: positive symbols, negative when inverted
        for base in (0, 300, 600, 900):
            x[base + ones[0]] = 0.0    # positive in the correlation: still a hit under the normal polarity,
            x[base + ones[1]] = -0.0   # a miss under the inverted one, where these entries were negative
            x[base + ones[2]] = np.nan
        pay = np.array([i for i in range(311, 1200, 7) if i % 300 >= 11])
        x[pay[0::3]] = 0.0
        x[pay[1::3]] = -0.0
        x[pay[2::3]] = np.nan
        cols.append(x)
    cols.append(np.full(1211, np.nan, np.float32))  # all positive: never a hit
    cols.append(np.zeros(1211, np.float32))
    p = Pair(ctx, M.B1I, [20] * 6, 1211)
    res = p.run(np.stack(cols, axis=1))
    assert res.counts.tolist() == [3, 3, 3, 0, 0, 0]
    assert [bool(f & abi.DNAV_INVERTED) for f in res.subframes[0]["flags"][:3]] == [False, True, False]
    assert [bool(f & abi.DNAV_INVERTED) for f in res.subframes[1]["flags"][:3]] == [False, False, True]
    assert not any(f & abi.DNAV_INVERTED for f in res.subframes[2]["flags"][:3])
    assert res.subframes[2, 0]["words"][0] >> 19 == 0b00000010010  # the three zeroed '1's of the preamble read as 0 bits
    assert p.dev.state(4)["stat"] == 0 and p.dev.state(5)["history_size"] == 311
    p.close()


def row_of(words, r):
    """Row r (0..17) of a record's words: the 15 bits decode_bch15_11_01 returned."""
    w = int(words[1 + r // 2])
    return ((w >> 19) & 0x7FF) << 4 | ((w >> 4) & 0xF) if r % 2 == 0 else ((w >> 8) & 0x7FF) << 4 | (w & 0xF)


def test_bch_every_15_bit_pattern_in_some_row(ctx):
    """1821 channels whose first decoded subframe carries, over its 18 rows, all 32 768 fifteen-bit patterns in a random
    order (so every row position sees 1821 random ones): words, corrected_mask and every other field equal the model;
    every non-codeword is touched; a double error is miscorrected to another codeword."""
    rng = np.random.default_rng(77)
    nch = 1821
    patterns = np.concatenate([rng.permutation(1 << 15), rng.integers(0, 1 << 15, nch * 18 - (1 << 15))]).reshape(nch, 18)
    cw = sum(b << (14 - i) for i, b in enumerate(M.bch_encode(M.int_bits(0x5A3, 11))))
    patterns[1820, 15] = cw ^ 0b11      # two errors (the last ten slots are behind the permutation)
    patterns[1820, 16] = cw ^ (1 << 9)  # one
    patterns[1820, 17] = cw
    assert len(set(patterns.reshape(-1).tolist())) == 1 << 15
    base = C.d1_stream(0, 3, 777, seed=2)[:611]
    x = np.repeat(base[:, None], nch, axis=1)
    bits = (patterns[:, :, None] >> (14 - np.arange(15))) & 1          # [ch, row, column]
    for r in range(18):
        w, rr = 1 + r // 2, r % 2
        x[300 + 30 * w + rr:300 + 30 * w + 30:2, :] = np.where(bits[:, r, :].T > 0, 1.0, -1.0)
    p = Pair(ctx, M.B3I, [20] * nch, 611)
    res = p.dev.run_symbols(x)
    exp = p.expect(x)
    assert res.counts.tolist() == [1] * nch
    for c in range(nch):
        r = exp[c][0][0]
        got = res.subframes[c, 0]
        assert tuple(int(w) for w in got["words"]) == tuple(r["words"]), c
        assert tuple(int(got[f]) for f in REC_FIELDS) == tuple(int(r[f]) for f in REC_FIELDS), c
        assert np.array_equal(res.tow_ms[:, c], exp[c][1]) and np.array_equal(res.sflags[:, c], exp[c][2])
    p.check_state("bch", channels=[0, 7, 1820])
    codewords = {sum(b << (14 - i) for i, b in enumerate(M.bch_encode(M.int_bits(v, 11)))) for v in range(2048)}
    for c in range(0, nch, 13):
        for r in range(18):
            assert bool((int(res.subframes[c, 0]["corrected_mask"]) >> r) & 1) == (int(patterns[c, r]) not in codewords)
            assert row_of(res.subframes[c, 0]["words"], r) in codewords
    words, mask = res.subframes[1820, 0]["words"], int(res.subframes[1820, 0]["corrected_mask"])
    assert row_of(words, 16) == row_of(words, 17) == cw and (mask >> 15) & 7 == 0b011
    wrong = row_of(words, 15)
    assert wrong in codewords and wrong != cw and bin(wrong ^ cw).count("1") == 3
    p.close()


def test_stamp_d1_ids_and_a_sow_jump(ctx):
    """D1: FraID 0, 6 and 7 leave the SOW and the flag alone while the TOW keeps counting; a SOW that jumps zeroes the TOW
    and valid_word; the next subframe is accepted because the TOW it is compared with is 0."""
    s = 5000
    specs = [(1, 0, s), (1, 0, s + 6), (0, 0, 9), (6, 0, 99), (2, 77, s + 24), (7, 0, 1), (3, 0, s + 100), (4, 127, s + 106)]
    x = build(False, specs, lead=5)
    p = Pair(ctx, M.B1I, [20], 1300)
    for k in range(0, len(x), 1300):
        p.run(x[k:k + 1300])
    subs = p.subs[0]
    i = {f: k for k, f in enumerate(REC_FIELDS)}
    assert [q[i["fra_id"]] for q in subs] == [1, 0, 6, 2, 7, 3, 4]
    assert [q[i["sow"]] for q in subs] == [s + 6, s + 6, s + 6, s + 24, s + 24, s + 100, s + 106]
    assert [bool(q[i["flags"]] & abi.DNAV_NEW_SOW) for q in subs] == [True, False, False, True, False, True, True]
    assert [bool(q[i["flags"]] & abi.DNAV_TOW_ZEROED) for q in subs] == [False] * 5 + [True, False]
    first = (s + 6 + 14) * 1000 + 311 * 20
    assert [q[i["tow_at_current_symbol_ms"]] for q in subs] == [first, first + 6000, first + 12000, first + 18000, first + 24000, 0,
                                                                 (s + 106 + 14) * 1000 + 311 * 20]
    assert subs[3][i["pnum"]] == 77 and subs[6][i["pnum"]] == 127
    assert p.dev.state(0)["valid_word"] == 1 and p.dev.state(0)["sow_set"] == 1
    p.close()


def test_stamp_d2_only_fraid_1_pages_1_to_10(ctx):
    """D2: FraID 2..5 and FraID 1 with Pnum 0 or 11..15 leave the SOW alone while the TOW keeps counting 2 ms a symbol; the
    FraID 1 page ten subframes (6 s) behind the first agrees with that clock."""
    s = 7000
    specs = [(1, 1, s - 1), (1, 1, s), (2, 3, 11), (3, 4, 12), (4, 5, 13), (5, 6, 14), (1, 0, 15), (1, 11, 16), (1, 12, 17), (1, 13, 18),
             (1, 14, 19), (1, 10, s + 6), (1, 15, 20)]
    x = build(True, specs, lead=2)
    p = Pair(ctx, M.B3I, [3], 1300)
    for k in range(0, len(x), 1300):
        p.run(x[k:k + 1300])
    subs = p.subs[0]
    i = {f: k for k, f in enumerate(REC_FIELDS)}
    assert [(q[i["fra_id"]], q[i["pnum"]]) for q in subs] == [(f, pn) for f, pn, _ in specs[1:]]
    assert [bool(q[i["flags"]] & abi.DNAV_NEW_SOW) for q in subs] == [True] + [False] * 9 + [True, False]
    assert not any(q[i["flags"]] & abi.DNAV_TOW_ZEROED for q in subs)
    first = (s + 14) * 1000 + 311 * 2
    assert [q[i["tow_at_current_symbol_ms"]] for q in subs] == [first + 600 * k for k in range(12)]
    assert [q[i["sow"]] for q in subs] == [s] * 10 + [s + 6] * 2
    p.close()


def test_set_satellite_new_channel_and_the_tight_record_bound(ctx):
    """set_satellite between runs changes the decoder and the timing and nothing else: state 2, the due symbol and the
    history stay.  new_channel gives a new object.  A run of max_rounds = 601 symbols that starts on a due symbol emits
    max_rounds / 300 + 1 = 3 records."""
    x = C.d1_stream(0, 4, 4000)
    assert len(x) == 1211
    p = Pair(ctx, M.B1I, [20, 20, 0], 601)
    assert p.dev.subframes_per_run == 3
    xs = np.stack([x, x, x], axis=1)
    p.check_state("as created")  # channel 2 is on PRN 0: D1, 20 ms
    assert p.dev.state(2)["symbol_duration_ms"] == 20 and p.dev.state(2)["d2_decoder"] == 0
    p.run(xs[:601])
    p.run(xs[601:610])
    p.set_satellite(1, 3)  # D1 → D2 with nine symbols to go to the first decode
    p.check_state("after set_satellite")
    st = p.dev.state(1)
    assert st["d2_decoder"] == 1 and st["symbol_duration_ms"] == 2 and st["stat"] == 1 and st["history_size"] == 311
    res = p.run(xs[610:])  # 601 symbols
    assert res.counts.tolist() == [3, 3, 3]
    assert res.subframes[0]["symbol_counter"].tolist() == [611, 911, 1211]
    assert all(f & abi.DNAV_D2_DECODER and f & abi.DNAV_D2_TIMING for f in res.subframes[1]["flags"])
    assert not any(f & abi.DNAV_D2_DECODER for f in res.subframes[0]["flags"])
    assert res.subframes[1]["words"].tolist() == res.subframes[0]["words"].tolist()  # the same history, decoded alike
    p.set_satellite(1, 20)  # and back
    p.dev.new_channel(0, 60)
    p.mod[0] = M.Decoder(M.B1I, 60, 0)
    p.check_state("after new_channel")
    st = p.dev.state(0)
    assert st["history_size"] == 0 and st["symbol_counter"] == 0 and st["d2_decoder"] == 1 and st["prn"] == 60
    res = p.run(xs[:601])
    assert res.counts.tolist() == [0, 2, 2] and res.subframes[1]["symbol_counter"][:2].tolist() == [1511, 1811]
    p.close()


def test_rejected_calls(ctx):
    for args in ((1, 0, abi.DNAV_B1I), (0, 10, abi.DNAV_B1I), (1, 10, 2), (1, 10, -1)):
        with pytest.raises(abi.GnssHipError) as e:
            engine.BeidouDnavTelemetryDecoder(ctx, *args)
        assert e.value.code == abi.E_INVAL
    d = engine.beidou_b3i_telemetry(ctx, 2, 10)
    d.run_symbols(np.ones((4, 2), np.float32))
    before = d.state(0)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_symbols(np.ones((11, 2), np.float32))
    assert e.value.code == abi.E_INVAL and b"max_rounds" in ctx.lib.gnsship_last_error(ctx.h)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_records(np.zeros((11, 2), abi.TRK_EPOCH_DTYPE))
    assert e.value.code == abi.E_INVAL
    for call in (d.reset_channel, lambda ch: d.set_satellite(ch, 3), lambda ch: d.new_channel(ch, 3), d.state):
        for ch in (-1, 2):
            with pytest.raises(abi.GnssHipError) as e:
                call(ch)
            assert e.value.code == abi.E_INVAL
    for prn in (-1, 64):
        for call in (d.set_satellite, d.new_channel):
            with pytest.raises(abi.GnssHipError) as e:
                call(0, prn)
            assert e.value.code == abi.E_INVAL
    assert d.state(0) == before
    assert d.run_symbols(np.zeros((0, 2), np.float32)).counts.tolist() == [0, 0] and d.state(0) == before
    lib = ctx.lib
    assert lib.gnsship_dnav_run_symbols(None, None, None, None, 0, 0, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_dnav_run_trk(None, None, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_dnav_destroy(None) == abi.E_INVAL
    d.close()


def test_run_trk_in_place(ctx):
    """A short tracking run; its device records go through the decoder in place.  No subframe can appear in so short a
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
    make = lambda ch, mr: engine.beidou_b3i_telemetry(ctx, ch, mr)
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
    m = M.Decoder(M.B3I, 0)
    recs, tow, sf = M.run([m], rec[:, :1]["prompt_i"].astype(np.float32), sel[:, None], None, rec[:, :1]["sample_counter"])
    assert not recs[0]
    for r in (got, res, ref):
        assert r.counts[0] == 0
        n = r.tow_ms.shape[0]
        assert n >= done and np.array_equal(r.tow_ms[:done, 0], tow[:done, 0]) and np.array_equal(r.sflags[:done, 0], sf[:done, 0])
    assert in_place.state(0) == other.state(0) == again.state(0) == m.state()
    assert m.state()["history_size"] == min(311, int(sel.sum()))
    plain = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    plain.start(0, 72, delay, dop, stamp, first)
    rec_plain, done_plain = plain.run(x, first, rounds)
    assert done_plain == done and rec_plain.tobytes() == rec.tobytes()
    plain.close()
    for h in (in_place, again, other, wrong, small, trk):
        h.close()
    buf.free()
