"""Every call the five telemetry decoders reject (gnsship_tlm_*, gnsship_lnav_*, gnsship_cnav_*, gnsship_dnav_*,
gnsship_gnav_*): the return code and the exact bytes of gnsship_last_error.

The decoders share one host layer (csrc/tlm_host.h); the texts a caller sees are part of the C ABI and are written out
here as literals, one table per family.  Every rejected call returns before a decoder kernel is launched.  The two
gnsship_*_run_trk rejections that compare against a tracker's run need one short tracking run (65 rounds, the decoders
hold 64), shared by the module."""
import ctypes

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

CHANNELS, ROUNDS = 2, 64
INVAL, STATE = abi.E_INVAL, abi.E_STATE
SENTINEL = b"gnsship_trk_records_device: null argument"

# family -> (configuration type, a configuration create accepts, output pointers of a run, masks of run_symbols,
#            run_trk reports its rounds)
FAMILIES = {
    "tlm": (abi.TlmConf, dict(frame_type=abi.TLM_INAV, vit_mode=abi.VIT_MODE_REFERENCE, max_rounds=ROUNDS, reserved=0), 4, 1, False),
    "lnav": (abi.LnavConf, dict(max_rounds=ROUNDS, reserved=0), 5, 2, True),
    "cnav": (abi.CnavConf, dict(max_rounds=ROUNDS, signal=abi.CNAV_L2C, reserved=0), 5, 2, True),
    "dnav": (abi.DnavConf, dict(max_rounds=ROUNDS, signal=abi.DNAV_B1I, reserved=0), 4, 2, True),
    "gnav": (abi.GnavConf, dict(max_rounds=ROUNDS, signal=abi.GNAV_L1CA, reserved=0), 4, 2, True),
}

# create: (configuration members changed or None for a null configuration, max_channels, text after "gnsship_<f>_create: ")
CREATE = {
    "tlm": [(None, 2, "null configuration"),
            (dict(frame_type=0), 2, "frame_type must be GNSSHIP_TLM_INAV, _FNAV or _CNAV"),
            (dict(frame_type=4), 2, "frame_type must be GNSSHIP_TLM_INAV, _FNAV or _CNAV"),
            (dict(vit_mode=2), 2, "unknown vit_mode"), (dict(vit_mode=-1), 2, "unknown vit_mode"),
            (dict(max_rounds=0), 2, "1 <= max_rounds <= 2^20"), (dict(max_rounds=(1 << 20) + 1), 2, "1 <= max_rounds <= 2^20"),
            (dict(reserved=1), 2, "reserved must be 0"),
            ({}, 0, "1 <= max_channels <= 2^20"), ({}, (1 << 20) + 1, "1 <= max_channels <= 2^20")],
    "lnav": [(None, 2, "null configuration"),
             (dict(max_rounds=0), 2, "1 <= max_rounds <= 2^20"), (dict(max_rounds=(1 << 20) + 1), 2, "1 <= max_rounds <= 2^20"),
             (dict(reserved=1), 2, "reserved must be 0"),
             ({}, 0, "1 <= max_channels <= 2^20"), ({}, (1 << 20) + 1, "1 <= max_channels <= 2^20")],
}
for _f, _names in (("cnav", "GNSSHIP_CNAV_L2C or GNSSHIP_CNAV_L5"), ("dnav", "GNSSHIP_DNAV_B1I or GNSSHIP_DNAV_B3I"),
                   ("gnav", "GNSSHIP_GNAV_L1CA or GNSSHIP_GNAV_L2CA")):
    CREATE[_f] = CREATE["lnav"][:3] + [(dict(signal=-1), 2, "signal must be " + _names), (dict(signal=2), 2, "signal must be " + _names)] + \
        CREATE["lnav"][3:]

# channel calls: family -> [(function, takes a PRN)]
CHANNEL_CALLS = {
    "tlm": [("reset_channel", False), ("set_satellite", False), ("new_channel", False)],
    "lnav": [("reset_channel", False), ("set_satellite", False), ("new_channel", False)],
    "cnav": [("reset_channel", False), ("new_channel", False)],
    "dnav": [("reset_channel", False), ("set_satellite", True), ("new_channel", True)],
    "gnav": [("set_satellite", True), ("new_channel", True)],
}

# state_set: (members changed in an all-zero state, text after "gnsship_<f>_state_set: ")
CNAV_FLAGS = "a part's flags must be 0 or 1"
STATE_SET = {
    "cnav": [({("part", 0, "old_is_metrics2"): 2}, CNAV_FLAGS), ({("part", 0, "preamble_seen"): 2}, CNAV_FLAGS),
             ({("part", 0, "invert"): 2}, CNAV_FLAGS), ({("part", 0, "message_lock"): 2}, CNAV_FLAGS),
             ({("part", 1, "crc_ok"): 2}, CNAV_FLAGS), ({("part", 1, "init"): 2}, CNAV_FLAGS),
             ({("part", 0, "n_symbols"): 64}, "n_symbols must be below the part's decode threshold"),
             ({("part", 1, "init"): 1, ("part", 1, "n_symbols"): 128}, "n_symbols must be below the part's decode threshold"),
             ({("part", 0, "n_decoded"): 481}, "n_decoded <= 480"), ({("part", 1, "decisions_index"): 64}, "decisions_index < 64"),
             ({("pll_180",): 2}, "the block's flags must be 0 or 1"), ({("valid_word",): 2}, "the block's flags must be 0 or 1"),
             ({("sent_tlm_failed",): 2}, "the block's flags must be 0 or 1")],
    "gnav": [(m, "stat 0..2, history_size == min(symbol_counter, 2000), crc_error_counter >= 0, flags 0 or 1") for m in (
        {("stat",): 3}, {("stat",): -1}, {("history_size",): 1}, {("history_size",): -1}, {("symbol_counter",): 5},
        {("symbol_counter",): 2001, ("history_size",): 2001}, {("crc_error_counter",): -1}, {("frame_sync",): 2},
        {("ephemeris_str", 3): 2}, {("utc_model_str_5",): 2}, {("tow_set",): 2}, {("tow_new",): 2})],
}
STATE_DTYPE = {"cnav": abi.CNAV_STATE_DTYPE, "gnav": abi.GNAV_STATE_DTYPE}


@pytest.fixture(scope="module")
def trackers(ctx):
    """idle: never run.  one / two: 1 and 2 channels, 65 rounds of records left on the device.  other: on a second context."""
    import trk_scenarios as S
    from test_gpu_trk import dev_conf
    fs, rounds = 4e6, ROUNDS + 1
    sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, rounds, rotator_avx=1)
    ctx.set_code(72, sat.code)
    buf = ctx.upload(np.ascontiguousarray(x, np.complex64))
    made = {"idle": engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), CHANNELS)}
    for name, nch in (("one", 1), ("two", CHANNELS)):
        t = made[name] = engine.DllPllVemlTracking(ctx, dev_conf(k, "GPS"), nch)
        for ch in range(nch):
            t.start(ch, 72, delay, dop, stamp, first)
        t.launch_ptr(buf.ptr, abi.FMT_CF32, first, len(x), rounds, records=True)
    ctx2 = engine.Context(0)
    made["other"] = engine.DllPllVemlTracking(ctx2, dev_conf(k, "GPS"), CHANNELS)
    yield made
    for name in ("one", "two"):
        made[name].collect()
    for t in made.values():
        t.close()
    ctx2.close()


class Rejections:
    def __init__(self, ctx, family, idle):
        self.ctx, self.lib, self.f, self.idle = ctx, ctx.lib, family, idle  # idle: a tracker handle for the call in between
        self.seen = 0

    def fn(self, name):
        return getattr(self.lib, f"gnsship_{self.f}_{name}")

    def expect(self, name, args, code, text):
        """The call returns `code` and leaves exactly "gnsship_<f>_<name>: <text>" as the context's last error."""
        assert self.lib.gnsship_trk_records_device(self.idle, None, None, None) == INVAL  # another text in between
        assert self.lib.gnsship_last_error(self.ctx.h) == SENTINEL
        rc = self.fn(name)(*args)
        got = self.lib.gnsship_last_error(self.ctx.h)
        want = f"gnsship_{self.f}_{name}: {text}".encode()
        assert (rc, got) == (code, want), (self.f, name, args)
        self.seen += 1


def put(st, path, value):
    for key in path[:-1]:
        st = st[key]
    st[path[-1]] = value


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_rejection_and_its_text(ctx, trackers, family):
    conf_type, conf_ok, n_out, n_masks, rounds_out = FAMILIES[family]
    R = Rejections(ctx, family, trackers["idle"].h)
    outs = (None,) * n_out

    for changed, nch, text in CREATE[family]:
        conf = None if changed is None else ctypes.byref(conf_type(**{**conf_ok, **changed}))
        h = ctypes.c_void_p(1)
        R.expect("create", (ctx.h, conf, nch, ctypes.byref(h)), INVAL, text)
        assert h.value is None

    h = ctypes.c_void_p()
    abi.check(R.fn("create")(ctx.h, ctypes.byref(conf_type(**conf_ok)), CHANNELS, ctypes.byref(h)), "create", ctx.h)
    try:
        sym = np.ones((2, CHANNELS), np.float32)
        rec = np.zeros((2, CHANNELS), abi.TRK_EPOCH_DTYPE)
        sp, rp, masks = ctypes.c_void_p(sym.ctypes.data), ctypes.c_void_p(rec.ctypes.data), (None,) * n_masks
        for n in (-1, ROUNDS + 1):
            R.expect("run_symbols", (h, sp, *masks, 0, n, *outs), INVAL, "0 <= n_rounds <= max_rounds")
            R.expect("run_records", (h, rp, 0, n, *outs), INVAL, "0 <= n_rounds <= max_rounds")
        for on_device in (0, 1):
            R.expect("run_symbols", (h, None, *masks, on_device, 2, *outs), INVAL, "null symbols")
            R.expect("run_records", (h, None, on_device, 2, *outs), INVAL, "null records")

        rounds = ctypes.c_int32(-7)
        tail = (*outs, ctypes.byref(rounds)) if rounds_out else outs
        R.expect("run_trk", (h, None, *tail), INVAL, "null tracking handle")
        R.expect("run_trk", (h, trackers["other"].h, *tail), INVAL, "the tracking handle is on another context")
        R.expect("run_trk", (h, trackers["idle"].h, *tail), STATE, "the tracker's last run kept no records on the device")
        R.expect("run_trk", (h, trackers["one"].h, *tail), INVAL, "the handles' max_channels differ")
        R.expect("run_trk", (h, trackers["two"].h, *tail), INVAL, "the tracker's run had more rounds than max_rounds")
        assert rounds.value == -7  # written only ahead of a launch

        for name, takes_prn in CHANNEL_CALLS[family]:
            for ch in (-1, CHANNELS):
                R.expect(name, (h, ch, 3) if takes_prn else (h, ch), INVAL, "channel out of range")
            if takes_prn:
                for prn in (-1, 64):
                    R.expect(name, (h, 0, prn), INVAL, "0 <= prn <= 63")
        for name in ("reset_channel", "set_satellite", "new_channel"):
            assert hasattr(ctx.lib, f"gnsship_{family}_{name}") == (name in dict(CHANNEL_CALLS[family]))

        R.expect("state_get", (h, 0, None), INVAL, "null state")
        room = np.zeros(4096, np.uint8)  # larger than any family's state
        for ch in (-1, CHANNELS):
            R.expect("state_get", (h, ch, ctypes.cast(ctypes.c_void_p(room.ctypes.data), R.fn("state_get").argtypes[2])), INVAL,
                     "channel out of range")
        assert not room.any()

        assert hasattr(ctx.lib, f"gnsship_{family}_state_set") == (family in STATE_SET)
        if family in STATE_SET:
            zero = np.zeros((), STATE_DTYPE[family])
            R.expect("state_set", (h, 0, None), INVAL, "null state")
            for ch in (-1, CHANNELS):
                R.expect("state_set", (h, ch, ctypes.c_void_p(zero.ctypes.data)), INVAL, "channel out of range")
            for changed, text in STATE_SET[family]:
                st = zero.copy()
                for path, value in changed.items():
                    put(st, path, value)
                R.expect("state_set", (h, 0, ctypes.c_void_p(st.ctypes.data)), INVAL, text)
            abi.check(R.fn("state_set")(h, 0, ctypes.c_void_p(zero.ctypes.data)), "state_set", ctx.h)  # the table's base is accepted
    finally:
        assert R.fn("destroy")(h) == abi.OK
    expected = len(CREATE[family]) + 8 + 5 + sum(4 if p else 2 for _, p in CHANNEL_CALLS[family]) + 3 + \
        (3 + len(STATE_SET[family]) if family in STATE_SET else 0)
    assert R.seen == expected
