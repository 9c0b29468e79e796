"""The device GLONASS GNAV telemetry decoder (tlm_glo_gnav.hip, gnsship_gnav_*) against the restatement of
glonass_l1_ca_telemetry_decoder_gs / glonass_l2_ca_telemetry_decoder_gs in tests/gnav_model.py.

Contract: exact equality — every field of every string record, every tow_ms / sflags entry, counts and every member of
gnsship_gnav_state (doubles by their bits) — for both polarities, any cut of a stream into runs, validity masks, tracking
records (host, device, in place), zeros, NaNs and sums that cancel, every single- and double-bit error of a string, and the
stamp over slices of its inputs.  The device accumulates half-bits as symbols arrive and keeps sign bits only; the model
keeps the doubles and decodes from the history, as the block does.

A string is decoded 2000 symbols after the second time mark seen with a full history, so the shortest stream that decodes
strings 1 to 5 and sets the time of week has 14 000 symbols and a lead-in; the deep cases start one symbol before a decode
through gnsship_gnav_state_set."""
import copy

import numpy as np
import pytest

import gnav_model as M
import test_gnav_model as C
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

REC_FIELDS = ["symbol_counter", "sample_counter", "channel", "prn", "string_id", "flipped_bit", "tow_at_current_symbol_ms", "flags"]
DOUBLES = ("tow_at_current_symbol", "tow", "tau_c", "tau_gps", "chip_acc")


bits_of = C.bits_of


def to_record(d: dict) -> np.ndarray:
    """A model state() as one abi.GNAV_STATE_DTYPE record."""
    st = np.zeros(1, abi.GNAV_STATE_DTYPE)
    for k, v in d.items():
        st[k][0] = v
    return st[0]


def state_key(st) -> tuple:
    """A device record or a model dict as a comparable tuple, doubles by their bits."""
    out = []
    for name in abi.GNAV_STATE_DTYPE.names:
        if name == "reserved":
            continue
        v = st[name]
        out.append((name, bits_of(v) if name in DOUBLES else (tuple(int(q) for q in v) if np.ndim(v) else int(v))))
    return tuple(out)


def assert_state(dev, c, model, label=""):
    got, want = state_key(dev.state(c)), state_key(model.state())
    assert got == want, (label, c, [(g, w) for g, w in zip(got, want) if g != w])


def rec_key(r, c=None) -> tuple:
    """A device record or a model dict as a comparable tuple."""
    return tuple(int(r[f]) for f in REC_FIELDS) + (bits_of(r["tow"]),) + tuple(int(w) for w in r["bits"])


def check(res, exp, spr, label=""):
    """res: an engine.GnavResult; exp: (records per channel, tow[n, C], sflags[n, C]) from the model."""
    recs, tow, sf = exp
    assert res.counts.tolist() == [len(r) for r in recs], (label, res.counts.tolist(), [len(r) for r in recs])
    for c, rs in enumerate(recs):
        assert len(rs) <= spr
        for k, r in enumerate(rs):
            assert rec_key(res.strings[c, k]) == rec_key(r), (label, c, k, rec_key(res.strings[c, k]), rec_key(r))
    assert np.array_equal(res.tow_ms, tow), (label, np.argwhere(res.tow_ms != tow)[:5])
    assert np.array_equal(res.sflags, sf), (label, np.argwhere(res.sflags != sf)[:5])


# ------------------------------------------------------------------------------------------------ the 16-channel stream
N16, ORDER = 15100, C.ORDER


def channel_stream(c, rng):
    """Channel c of the main stream: a lead-in of 1 + 61 c symbols, odd channels inverted, strings 4 5 1 2 3 4 5 1 of a frame
    of its own, magnitudes of its own."""
    strings = M.frame_strings(t_k_raw=int(rng.integers(0, 4096)), t_b_raw=0 if c == 14 else int(rng.integers(1, 96)), n_t=int(rng.integers(1, 1462)),
                              n=1 + c, n_4=int(rng.integers(1, 10)), tau_c=int(rng.integers(-2 ** 20, 2 ** 20)), tau_gps=int(rng.integers(-2 ** 12, 2 ** 12)),
                              rng=rng, ids=ORDER)
    x = M.stream(strings, lead=1 + 61 * c, inverted=bool(c & 1))[:N16]
    if c % 3 == 1:
        x = x * rng.uniform(0.2, 3.0, len(x)).astype(np.float32)
    elif c % 3 == 2:
        x = x * np.float32(1e-3 * (c + 1))
    return x


@pytest.fixture(scope="module")
def stream16():
    """symbols[N16, 16], the model's outputs for them and the models after them.  Channels 0..9 are clean; 10: NaNs in the
    data; 11: +0 and -0 in the data and in a time mark; 12: half-bits whose ten symbols cancel to exactly 0, and sums whose
    value depends on the order of addition; 13: a time mark more than half wrong in state 2 (corr <= 0, not a hit: decoded
    inverted); 14: t_b == 0; 15: noise, never a hit."""
    rng = np.random.default_rng(2026)
    x = np.stack([channel_stream(c, rng) for c in range(16)], axis=1)
    data = lambda c, k: 1 + 61 * c + 300 + 2000 * k  # the first data symbol (0-based row) of string k of channel c
    rows = data(10, 2) + rng.choice(1700 * 5, 60, replace=False)
    x[rows, 10] = np.nan
    rows = data(11, 2) + rng.choice(2000 * 5, 90, replace=False)  # time marks included
    x[rows[0::2], 11] = 0.0
    x[rows[1::2], 11] = -0.0
    for k in range(2, 7):
        for h in rng.choice(170, 3, replace=False):
            r = data(12, k) + 10 * h
            x[r:r + 10, 12] = np.float32(0.75) * np.array([1, -1, 1, 1, -1, -1, 1, -1, -1, 1], np.float32)
        r = data(12, k) + 10 * int(rng.integers(0, 170))
        x[r:r + 10, 12] = np.array([3e30, 1, -3e30, -0.5, 0, 0, 0, 0, 0, 0], np.float32)  # in order: -0.5; exactly: +0.5
    r = data(13, 3) - 300  # the time mark in front of string 3's data, tested at that string's decode
    x[r:r + 160, 13] = -x[r:r + 160, 13]
    x[:, 15] = rng.standard_normal(N16).astype(np.float32)
    models = [M.Decoder(0, c) for c in range(16)]
    recs, tow, sf = M.run(models, x)
    return x, (recs, tow, sf), models


def test_stream16_is_what_it_says(stream16):
    """The model's view of the stream: strings 1..5 decoded, the time of week set by string 5 at symbol 14 000 + lead, the
    PRN moved by string 4, the inverted channels inverted, the dirty channels dirty."""
    x, (recs, tow, sf), models = stream16
    for c in range(10):
        lead = 1 + 61 * c
        assert [r["symbol_counter"] for r in recs[c]] == [6000 + lead + 2000 * k for k in range(5)]
        assert [r["string_id"] for r in recs[c]] == [1, 2, 3, 4, 5]
        assert all(r["flags"] & M.CRC_OK and not r["flags"] & M.CORRECTED and bool(r["flags"] & M.INVERTED) == bool(c & 1) for r in recs[c])
        assert [r["prn"] for r in recs[c]] == [0, 0, 0, 1 + c, 1 + c] and recs[c][3]["flags"] & M.SLOT_UPDATED
        assert recs[c][4]["flags"] & (M.NEW_TOW | M.NEW_EPHEMERIS | M.NEW_UTC_MODEL) == M.NEW_TOW | M.NEW_EPHEMERIS | M.NEW_UTC_MODEL
        assert not (sf[:14000 + lead - 1, c] & M.S_VALID_WORD).any() and (sf[14000 + lead - 1:, c] & M.S_VALID_WORD).all()
        assert models[c].state()["ephemeris_str"] == [0, 0, 0, 0]
    assert any(not r["flags"] & M.CRC_OK for r in recs[10]) and any(not r["flags"] & M.CRC_OK or r["flags"] & M.CORRECTED for r in recs[12])
    assert [bool(r["flags"] & M.INVERTED) for r in recs[13]][:3] == [True, False, True]
    assert recs[14][4]["flags"] & M.NEW_TOW and not recs[14][4]["flags"] & M.NEW_EPHEMERIS and models[14].state()["ephemeris_str"] == [1, 1, 1, 1]
    assert not recs[15] and models[15].stat == 0


@pytest.mark.parametrize("cut", [1, 63, 64, 65, 1999, 2000, 2001, N16])
def test_cuts_give_the_models_outputs(ctx, stream16, cut):
    """16 channels at different offsets and polarities, clean and dirty, in runs of `cut` symbols: every output and the
    state after the last run equal the model's over the whole stream."""
    x, (recs, tow, sf), models = stream16
    dev = engine.glonass_l1_ca_telemetry(ctx, 16, cut)
    assert dev.strings_per_run == M.strings_per_run(cut) == abi.gnav_strings_per_run(cut)
    got = [[] for _ in range(16)]
    tows, sfs = [], []
    for k in range(0, N16, cut):
        res = dev.run_symbols(x[k:k + cut])
        for c in np.nonzero(res.counts)[0]:
            assert res.counts[c] <= dev.strings_per_run
            got[c] += [rec_key(res.strings[c, i]) for i in range(res.counts[c])]
        tows.append(res.tow_ms)
        sfs.append(res.sflags)
    assert got == [[rec_key(r) for r in rs] for rs in recs]
    assert np.array_equal(np.concatenate(tows), tow) and np.array_equal(np.concatenate(sfs), sf)
    for c in range(16):
        assert_state(dev, c, models[c], f"cut {cut}")
    dev.close()


# ------------------------------------------------------------------------------------------------ masks and records
def records_from(sym, valid, rng):
    """Tracking records whose valid entries carry the symbols as doubles that do not round-trip to float."""
    rec = np.zeros(sym.shape, abi.TRK_EPOCH_DTYPE)
    rec["prompt_i"] = sym.astype(np.float64) * (1.0 + rng.uniform(-2e-8, 2e-8, sym.shape))
    rec["prompt_q"] = rng.standard_normal(sym.shape)
    rec["flags"] = 8 | np.where(valid != 0, 1, 0)
    rec["sample_counter"] = (np.arange(sym.shape[0], dtype=np.uint64)[:, None] * np.uint64(4000) + np.uint64(1 << 33)
                             + np.arange(sym.shape[1], dtype=np.uint64)[None, :])
    return rec


def test_valid_masks_and_records(ctx):
    """Holes in the validity mask; the same entries as floats and masks on the device; as records from the host and the
    device, where the symbol is the record's double: one half-bit is 1 + 2^-40 then -1, positive as doubles, zero as floats."""
    rng = np.random.default_rng(3)
    n, rounds = 8200, 8800
    valid = np.zeros((rounds, 4), np.uint8)
    sym = rng.standard_normal((rounds, 4)).astype(np.float32) * 9.0  # what sits in invalid entries must not matter
    rows_of = []
    for c in range(4):
        rows = np.sort(rng.choice(rounds, n, replace=False)) if c else np.arange(n)
        if c == 3:
            rows = np.concatenate([np.arange(6000), np.arange(6600, 6600 + n - 6000)])  # a long gap
        valid[rows, c] = 1
        strings = M.frame_strings(t_k_raw=77 * c, n_t=5 + c, n=3 + c, rng=rng, ids=(4, 5, 1, 2))
        sym[rows, c] = M.stream(strings, lead=7 + 50 * c, inverted=c == 1)[:n]
        rows_of.append(rows)
    spr = M.strings_per_run(rounds)
    a = engine.glonass_l2_ca_telemetry(ctx, 4, rounds)
    ma = [M.Decoder(0, c) for c in range(4)]
    exp = M.run(ma, sym, valid)
    res = a.run_symbols(sym, valid, np.zeros_like(valid))  # out_valid is not read
    check(res, exp, spr, "symbols")
    assert res.counts.tolist() == [2, 2, 2, 2] and (res.tow_ms[valid == 0] == 0).all() and (res.sflags[valid == 0] == 0).all()
    for c in range(4):
        assert_state(a, c, ma[c], "symbols")
    bufs = [ctx.upload(np.ascontiguousarray(v).view(np.uint8).reshape(-1)) for v in (sym, valid)]
    s = engine.glonass_l2_ca_telemetry(ctx, 4, rounds)
    res_d = s.run_symbols(bufs[0].ptr, bufs[1].ptr, None, on_device=True, n_rounds=rounds)
    assert res_d.strings.tobytes() == res.strings.tobytes() and np.array_equal(res_d.tow_ms, res.tow_ms) and np.array_equal(res_d.sflags, res.sflags)
    for bf in bufs:
        bf.free()

    rec = records_from(sym, valid, rng)
    r0 = rows_of[0][7 + 300 + 2000 * 2 + 10 * 20]  # a pair of half-bits of string 1 of channel 0
    rec["prompt_i"][r0:r0 + 10, 0] = [1.0 + 2.0 ** -40, -1.0, 0, 0, 0, 0, 0, 0, 0, 0]
    rec["prompt_i"][r0 + 10:r0 + 20, 0] = -1.0  # "10" as doubles, "00" as floats
    mb = [M.Decoder(0, c) for c in range(4)]
    exp = M.run(mb, rec["prompt_i"], valid, rec["sample_counter"])
    narrow = M.run([M.Decoder(0, 0)], rec["prompt_i"][:, :1].astype(np.float32), valid[:, :1], rec["sample_counter"][:, :1])
    assert [r["bits"] for r in narrow[0][0]] != [r["bits"] for r in exp[0][0]]  # the doubles matter
    b = engine.glonass_l1_ca_telemetry(ctx, 4, rounds)
    check(b.run_records(rec), exp, spr, "host records")
    assert exp[0][1][0]["sample_counter"] == rec["sample_counter"][rows_of[1][6000 + 7 + 50 - 1], 1]
    assert b.run_records(rec[:0]).counts.tolist() == [0, 0, 0, 0]
    d = engine.glonass_l1_ca_telemetry(ctx, 4, rounds)
    buf = ctx.upload(rec.view(np.uint8).reshape(-1))
    check(d.run_records(buf.ptr, on_device=True, n_rounds=rounds), exp, spr, "device records")
    buf.free()
    for c in range(4):
        assert_state(b, c, mb[c], "host records")
        assert_state(d, c, mb[c], "device records")
    for h in (a, s, b, d):
        h.close()


def test_run_trk_in_place(ctx):
    """A short tracking run; its device records go through the decoder in place.  No string can appear in so short a run:
    the check is the state, the tow_ms / sflags stream, the equality with run_records and the model, the error codes."""
    import trk_scenarios as S
    from test_gpu_trk import dev_conf
    fs, rounds = 4e6, 400
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, rounds, rotator_avx=1)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), 1)
    ctx.set_code(72, sat.code)
    trk.start(0, 72, delay, dop, stamp, first)
    x = np.ascontiguousarray(x, np.complex64)
    buf = ctx.upload(x)
    make = lambda ch, mr: engine.glonass_l1_ca_telemetry(ctx, ch, mr)
    in_place = make(1, rounds)
    with pytest.raises(abi.GnssHipError) as e:  # nothing launched yet
        in_place.run_trk(trk)
    assert e.value.code == abi.E_STATE
    trk.launch_ptr(buf.ptr, abi.FMT_CF32, first, len(x), rounds, records=True)
    got = in_place.run_trk(trk)  # before the collect
    rec, done = trk.collect()
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
    m = M.Decoder(0, 0)
    recs, tow, sf = M.run([m], rec[:, :1]["prompt_i"], sel[:, None], rec[:, :1]["sample_counter"])
    assert not recs[0]
    for r in (got, ref):
        assert r.counts[0] == 0
        assert r.tow_ms.shape[0] >= done and np.array_equal(r.tow_ms[:done, 0], tow[:done, 0]) and np.array_equal(r.sflags[:done, 0], sf[:done, 0])
    assert_state(in_place, 0, m)
    assert_state(other, 0, m)
    for h in (in_place, other, wrong, small, trk):
        h.close()
    buf.free()


# ------------------------------------------------------------------------------------------------ one symbol before a decode
@pytest.fixture(scope="module")
def primed():
    """tests/test_gnav_model.primed_model: a model one symbol before the decode of a string 5 (symbol 14 003 of its stream),
    the stream's remaining symbols, the string's characters."""
    return C.primed_model()


with_string = C.with_string


def launch_cases(ctx, cases, max_rounds=1):
    """cases: [(model, last symbol)].  One channel per case: state_set, one launch of one symbol, everything compared."""
    n = len(cases)
    dev = engine.glonass_l1_ca_telemetry(ctx, n, max_rounds)
    for c, (m, _) in enumerate(cases):
        m.channel = c
        dev.set_state(c, to_record(m.state()))
    x = np.array([[s for _, s in cases]], np.float32)
    res = dev.run_symbols(x)
    exp = M.run([m for m, _ in cases], x)
    check(res, exp, dev.strings_per_run, "cases")
    return dev, res, exp


def test_state_set_one_symbol_before_a_decode(ctx, primed):
    """The state of the model goes to a new handle; the decode of string 5 and everything after it equal the model's."""
    template, rest, chars = primed
    m = copy.deepcopy(template)
    dev = engine.glonass_l1_ca_telemetry(ctx, 2, len(rest))
    dev.set_state(1, to_record(m.state()))
    assert_state(dev, 1, m, "after set")
    assert state_key(dev.state(0)) == state_key(M.Decoder(0, 0).state())
    x = np.stack([np.zeros(len(rest), np.float32), rest], axis=1)
    m.channel = 1
    res = dev.run_symbols(x)
    exp = M.run([M.Decoder(0, 0), m], x)
    check(res, exp, dev.strings_per_run, "after state_set")
    assert res.counts.tolist() == [0, 7] and res.strings[1, 0]["symbol_counter"] == 14003 and res.strings[1, 0]["flags"] & abi.GNAV_NEW_TOW
    assert res.strings[1, 0]["string_id"] == 5 and res.sflags[0, 1] == abi.GNAV_S_VALID_WORD | abi.GNAV_S_STRING
    assert_state(dev, 1, m, "after the run")
    bad = to_record(m.state())
    for name, value in (("stat", 3), ("history_size", 1999), ("crc_error_counter", -1), ("tow_set", 2)):
        st = bad.copy()
        st[name] = value
        with pytest.raises(abi.GnssHipError) as e:
            dev.set_state(1, st)
        assert e.value.code == abi.E_INVAL
    assert_state(dev, 1, m, "after rejected sets")
    dev.close()


def test_every_single_and_double_bit_error(ctx, primed):
    """All 85 single-bit and all 3570 double-bit errors of one string 5, and the string itself, one channel each in one
    launch.  The block's third branch asks for odd parity over bits 8..84 of the word as received, so which single errors
    it accepts depends on the string: this one has even parity there, and every single error is accepted — corrected in an
    information bit, left alone in beta_1..beta_7 — except the one in the overall parity bit, which is rejected.  (With odd
    parity the information-bit errors are rejected and the parity-bit error flips bit 0: tests/test_gnav_model.py.)"""
    template, _, chars = primed
    flips = [()] + [(i,) for i in range(85)] + [(i, j) for i in range(85) for j in range(i + 1, 85)]
    assert len(flips) == 1 + 85 + 3570
    cases = []
    for f in flips:
        ch = list(chars)
        for i in f:
            ch[i] ^= 1
        cases.append(with_string(template, ch))
    dev, res, exp = launch_cases(ctx, cases)
    assert res.counts.tolist() == [1] * len(flips)
    flags = res.strings[:, 0]["flags"]
    clean_bits = res.strings[0, 0]["bits"].tolist()
    assert flags[0] & abi.GNAV_CRC_OK and not flags[0] & abi.GNAV_CORRECTED
    for c in range(1, 86):
        i = flips[c][0]  # character i is bit 84 - i
        if i == 0:       # the idle character is not sent: the relative code starts from 0 whatever it is
            assert flags[c] & abi.GNAV_CRC_OK and not flags[c] & abi.GNAV_CORRECTED and res.strings[c, 0]["bits"].tolist() == clean_bits
            continue
        assert bool(flags[c] & abi.GNAV_CRC_OK) == (84 - i != 7)
        if 84 - i == 7:
            continue
        if 84 - i >= 8:
            assert flags[c] & abi.GNAV_CORRECTED and res.strings[c, 0]["flipped_bit"] == 84 - i and res.strings[c, 0]["bits"].tolist() == clean_bits
        else:
            assert not flags[c] & abi.GNAV_CORRECTED and res.strings[c, 0]["flipped_bit"] == -1
    assert (flags[86:] & abi.GNAV_CRC_OK == 0).sum() > 3000  # most double errors are rejected; the rest are what the block does
    for c in (0, 1, 40, 86, 3000, len(flips) - 1):
        assert_state(dev, c, cases[c][0], "errors")
    dev.close()


whole_tow = C.whole_tow


def test_stamp_slices_and_a_negative_stamp(ctx, primed):
    """One string-5 decode per channel, in one launch: all 4096 raw t_k (N_T 500, N_4 6), all 2048 N_T (with a t_k that rolls
    the date back) and all 32 N_4 (N_T 1461 and 60: both sides of 29 February 2100), each with random signed tau_c and
    tau_gps; 300 cases random in everything; the largest and smallest tau; and two negative stamps, which only members
    set from outside can give: the low 32 bits of the int64 value."""
    template, _, _ = primed
    rng = np.random.default_rng(5)
    raw_of = lambda t_k: (t_k // 3600) << 7 | (t_k % 3600 // 60) << 1 | (t_k % 60 // 30)
    specs = [(raw, 500, 6) for raw in range(4096)] + [(raw_of(3 * 3600 - 40), n_t, 6) for n_t in range(2048)]
    specs += [(100, n_t, n_4) for n_4 in range(32) for n_t in (1461, 60)]
    specs += [(int(rng.integers(0, 4096)), int(rng.integers(0, 2048)), int(rng.integers(0, 32))) for _ in range(300)]
    taus = [(int(rng.integers(-2 ** 31 + 1, 2 ** 31)), int(rng.integers(-2 ** 21 + 1, 2 ** 21))) for _ in specs]
    specs += [(100, 500, 6)] * 4
    taus += [(2 ** 31 - 1, 2 ** 21 - 1), (-2 ** 31 + 1, -2 ** 21 + 1), (0, 0), (-1, 1)]
    cases = []
    for (raw, n_t, n_4), (tc, tg) in zip(specs, taus):
        five = M.frame_strings(n_4=n_4, tau_c=tc, tau_gps=tg, rng=rng, ids=(5,))[0]
        m, last = with_string(template, five)
        m.nav.t_k = (raw >> 7) * 3600 + ((raw >> 1) & 63) * 60 + (raw & 1) * 30
        m.nav.n_t = n_t
        cases.append((m, last))
    # no string can make d_TOW negative (its whole seconds are at least 17, the corrections below 1.002): the members can
    three = M.frame_strings(rng=rng, ids=(3,))[0]
    m, last = with_string(template, three)
    m.nav.tow, m.nav.tow_new = -0.25, True  # an accepted string 3 takes the stamp from it
    cases.append((m, last))
    m, last = with_string(template, three)
    m.tow_cur = -0.5                         # and this one counts on from a negative clock
    cases.append((m, last))
    dev, res, exp = launch_cases(ctx, cases)
    assert res.counts.tolist() == [1] * len(cases)
    n_five = len(specs)
    assert (res.strings[:n_five, 0]["flags"] & (abi.GNAV_CRC_OK | abi.GNAV_NEW_TOW | abi.GNAV_CORRECTED) == abi.GNAV_CRC_OK | abi.GNAV_NEW_TOW).all()
    for c in (0, 4095, 4096, 6144, n_five, n_five + 1):
        assert_state(dev, c, cases[c][0], "stamp")
    for c, ((raw, n_t, n_4), (tc, tg)) in enumerate(zip(specs, taus)):  # the model's calendar against plain day counting
        t_k = (raw >> 7) * 3600 + ((raw >> 1) & 63) * 60 + (raw & 1) * 30
        assert res.strings[c, 0]["tow"] == float(whole_tow(n_4, n_t, t_k)) + (tc * 2.0 ** -31 + tg * 2.0 ** -30), c
    assert res.strings[n_five, 0]["flags"] & abi.GNAV_NEW_TOW and res.tow_ms[0, n_five] == (-550) & 0xFFFFFFFF
    assert res.tow_ms[0, n_five + 1] == (-499) & 0xFFFFFFFF and bits_of(dev.state(n_five + 1)["tow_at_current_symbol"]) == bits_of(-0.5 + 0.001)
    dev.close()


def test_loss_of_sync_and_the_way_back(ctx, primed):
    """Six bad strings counted, the seventh drops frame sync and returns to state 0 (the counter is not cleared); from
    there the time marks are found again with the window the decode gathered, and state 2 comes back 4000 symbols on."""
    template, rest, chars = primed
    bad = list(chars)
    bad[20] ^= 1
    bad[33] ^= 1
    m, last = with_string(template, bad)
    m.crc_error_counter, m.frame_sync = 6, True
    keep, _ = with_string(template, bad)
    keep.crc_error_counter, keep.frame_sync = 5, True
    n = 4100
    dev = engine.glonass_l1_ca_telemetry(ctx, 2, n)
    x = np.stack([np.concatenate([[last], rest[1:n]])] * 2, axis=1).astype(np.float32)
    for c, mod in enumerate((m, keep)):
        mod.channel = c
        dev.set_state(c, to_record(mod.state()))
    res = dev.run_symbols(x[:1])
    check(res, M.run([m, keep], x[:1]), dev.strings_per_run, "the seventh")
    st = dev.state(0)
    assert st["stat"] == 0 and st["frame_sync"] == 0 and st["crc_error_counter"] == 7 and not res.strings[0, 0]["flags"] & abi.GNAV_CRC_OK
    st = dev.state(1)
    assert st["stat"] == 2 and st["frame_sync"] == 1 and st["crc_error_counter"] == 6
    res = dev.run_symbols(x[1:])
    check(res, M.run([m, keep], x[1:]), dev.strings_per_run, "the way back")
    assert res.counts.tolist() == [0, 2] and m.stat == 2 and m.preamble_index == 14003 + 4000
    for c, mod in enumerate((m, keep)):
        assert_state(dev, c, mod, "after")
    dev.close()


def test_the_tight_record_bound_set_satellite_and_new_channel(ctx, primed):
    """A run of max_rounds = 2001 symbols that starts on a due symbol emits max_rounds / 2000 + 1 = 2 records.
    set_satellite moves the PRN and nothing else; new_channel gives a new object."""
    template, rest, _ = primed
    m = copy.deepcopy(template)
    dev = engine.glonass_l2_ca_telemetry(ctx, 1, 2001)
    assert dev.strings_per_run == 2
    dev.set_state(0, to_record(m.state()))
    dev.set_satellite(0, 9)
    m.set_satellite(9)
    assert_state(dev, 0, m, "set_satellite")
    x = rest[:2001, None]
    res = dev.run_symbols(x)
    check(res, M.run([m], x), 2, "tight")
    assert res.counts.tolist() == [2] and res.strings[0]["symbol_counter"].tolist() == [14003, 16003] and res.strings[0, 0]["prn"] == 9
    dev.new_channel(0, 4)
    assert state_key(dev.state(0)) == state_key(M.Decoder(4, 0).state())
    dev.close()


def test_the_filling_ring(ctx):
    """A stream whose first 300 symbols are a time mark: while the ring fills, the first 300 symbols are tested again on
    every symbol (state 1 from symbol 300); the mark at 4000 is more than 2000 after it and sends the block back to state 0."""
    rng = np.random.default_rng(8)
    x = M.stream(M.frame_strings(rng=rng, ids=(1, 2, 3)), lead=0)[:4100, None]
    dev = engine.glonass_l1_ca_telemetry(ctx, 1, 2000)
    m = M.Decoder(0, 0)
    for k, end, want in ((0, 299, (0, 0)), (299, 300, (1, 300)), (300, 2000, (1, 300)), (2000, 3999, (1, 300)), (3999, 4100, (0, 300))):
        part = x[k:end]
        check(dev.run_symbols(part), M.run([m], part), dev.strings_per_run, f"at {k}")
        st = dev.state(0)
        assert (st["stat"], st["preamble_index"]) == want
        assert_state(dev, 0, m, f"at {k}")
    dev.close()


def test_rejected_calls(ctx):
    for args in ((1, 0, abi.GNAV_L1CA), (0, 10, abi.GNAV_L1CA), (1, 10, 2), (1, 10, -1)):
        with pytest.raises(abi.GnssHipError) as e:
            engine.GlonassGnavTelemetryDecoder(ctx, *args)
        assert e.value.code == abi.E_INVAL
    d = engine.glonass_l2_ca_telemetry(ctx, 2, 10)
    d.run_symbols(np.ones((4, 2), np.float32))
    before = state_key(d.state(0))
    with pytest.raises(abi.GnssHipError) as e:
        d.run_symbols(np.ones((11, 2), np.float32))
    assert e.value.code == abi.E_INVAL and b"max_rounds" in ctx.lib.gnsship_last_error(ctx.h)
    with pytest.raises(abi.GnssHipError) as e:
        d.run_records(np.zeros((11, 2), abi.TRK_EPOCH_DTYPE))
    assert e.value.code == abi.E_INVAL
    for call in (lambda ch: d.set_satellite(ch, 3), lambda ch: d.new_channel(ch, 3), d.state, lambda ch: d.set_state(ch, d.state(0))):
        for ch in (-1, 2):
            with pytest.raises(abi.GnssHipError) as e:
                call(ch)
            assert e.value.code == abi.E_INVAL
    for prn in (-1, 64):
        for call in (d.set_satellite, d.new_channel):
            with pytest.raises(abi.GnssHipError) as e:
                call(0, prn)
            assert e.value.code == abi.E_INVAL
    assert state_key(d.state(0)) == before
    assert d.run_symbols(np.zeros((0, 2), np.float32)).counts.tolist() == [0, 0] and state_key(d.state(0)) == before
    lib = ctx.lib
    assert lib.gnsship_gnav_run_symbols(None, None, None, None, 0, 0, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_gnav_run_trk(None, None, None, None, None, None, None) == abi.E_INVAL
    assert lib.gnsship_gnav_destroy(None) == abi.E_INVAL
    d.close()
