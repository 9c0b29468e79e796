"""Every call the four stream blocks reject (gnsship_acq_resampler_*, gnsship_cond_*, gnsship_mit_*, gnsship_vit_*): the
return code and the exact bytes of gnsship_last_error.

The blocks' create, run and destroy are made of the helpers of csrc/host_api.h; the texts a caller sees are part of the
C ABI and are written out here as literals.  Every rejected call returns before a kernel is launched, and the handles
are the smallest there are.  The calls that take no context (the tap designs, the threshold, a null handle or output)
return GNSSHIP_E_INVAL and leave the context's text alone."""
import ctypes

import numpy as np
import pytest

from gnss_sim_receiver_amd import abi

pytestmark = pytest.mark.gpu

INVAL = abi.E_INVAL
SENTINEL = b"gnsship_code_set: bad code id / length (1..16384)"
NAN = float("nan")


class Rejections:
    def __init__(self, ctx):
        self.ctx, self.lib, self.seen = ctx, ctx.lib, 0

    def sentinel(self):
        assert self.lib.gnsship_code_set(self.ctx.h, -1, None, 0) == INVAL  # another text in between
        assert self.lib.gnsship_last_error(self.ctx.h) == SENTINEL

    def expect(self, name, args, text):
        """The call returns GNSSHIP_E_INVAL and leaves exactly "<name>: <text>" as the context's last error."""
        self.sentinel()
        rc = getattr(self.lib, name)(*args)
        assert (rc, self.lib.gnsship_last_error(self.ctx.h)) == (INVAL, f"{name}: {text}".encode()), (name, args)
        self.seen += 1

    def silent(self, name, args):
        """The call returns GNSSHIP_E_INVAL and writes no text."""
        self.sentinel()
        rc = getattr(self.lib, name)(*args)
        assert (rc, self.lib.gnsship_last_error(self.ctx.h)) == (INVAL, SENTINEL), (name, args)
        self.seen += 1


def vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_acq_resampler(ctx):
    R, h = Rejections(ctx), ctypes.c_void_p(1)
    taps = np.array([0.25, 0.5, 0.25], np.float32)
    create = "1 <= n_taps <= 4096, decimation >= 1, max_in_samples >= decimation"
    for tp, nt, dec, max_in in ((None, 3, 2, 64), (abi.fptr(taps), 0, 2, 64), (abi.fptr(taps), 4097, 2, 64), (abi.fptr(taps), 3, 0, 64),
                                (abi.fptr(taps), 3, 2, 1)):
        R.expect("gnsship_acq_resampler_create", (ctx.h, tp, nt, dec, max_in, ctypes.byref(h)), create)
        assert h.value is None
        h = ctypes.c_void_p(1)
    R.silent("gnsship_acq_resampler_create", (None, abi.fptr(taps), 3, 2, 64, ctypes.byref(h)))
    R.silent("gnsship_acq_resampler_create", (ctx.h, abi.fptr(taps), 3, 2, 64, None))
    d, n = ctypes.c_int(), ctypes.c_int()
    for args in ((4000000, 1e6, None, None, 0, ctypes.byref(n)), (4000000, 1e6, ctypes.byref(d), None, 0, None),
                 (0, 1e6, ctypes.byref(d), None, 0, ctypes.byref(n)), (4000000, 0.0, ctypes.byref(d), None, 0, ctypes.byref(n))):
        R.silent("gnsship_acq_resampler_design", args)
    for args in ((1.0, 4e6, 1e6, 1e5, None, 0, None), (1.0, 0.0, 1e6, 1e5, None, 0, ctypes.byref(n)), (1.0, 4e6, 0.0, 1e5, None, 0, ctypes.byref(n)),
                 (1.0, 4e6, 2.5e6, 1e5, None, 0, ctypes.byref(n)), (1.0, 4e6, 1e6, 0.0, None, 0, ctypes.byref(n)),
                 (1.0, 4e6, 1e6, 1e6, abi.fptr(taps), 3, ctypes.byref(n))):  # the last: 9 taps into room for 3
        R.silent("gnsship_firdes_low_pass", args)
    for name in ("reset", "destroy"):
        R.silent(f"gnsship_acq_resampler_{name}", (None,))

    abi.check(ctx.lib.gnsship_acq_resampler_create(ctx.h, abi.fptr(taps), 3, 2, 64, ctypes.byref(h)), "create", ctx.h)
    try:
        x = np.zeros(64, np.complex64)
        run = "n_in must be a multiple of the decimation, <= max_in_samples"
        for ptr, fmt, n_in in ((None, abi.FMT_CF32, 64), (vp(x), 3, 64), (vp(x), -1, 64), (vp(x), abi.FMT_CF32, 0), (vp(x), abi.FMT_CF32, 1),
                               (vp(x), abi.FMT_CF32, 66), (vp(x), abi.FMT_CF32, 63)):
            for on_device in (0, 1):
                R.expect("gnsship_acq_resampler_run", (h, ptr, fmt, on_device, n_in, None, None, None), run)
        R.silent("gnsship_acq_resampler_run", (None, vp(x), abi.FMT_CF32, 0, 64, None, None, None))
    finally:
        assert ctx.lib.gnsship_acq_resampler_destroy(h) == abi.OK
    assert R.seen == 5 + 2 + 4 + 6 + 2 + 14 + 1


def test_conditioner(ctx):
    R, h = Rejections(ctx), ctypes.c_void_p(1)
    taps = np.array([0.25, 0.5, 0.25], np.float32)

    def bands(n=1, **changed):
        arr = (abi.CondBand * max(1, n))()
        for b in range(n):
            arr[b] = abi.CondBand(**{**dict(if_hz=1000.0, decimation=2, taps=abi.fptr(taps), n_taps=3), **changed})
        return arr

    null_taps = ctypes.POINTER(ctypes.c_float)()
    cases = [((1e6, None, 1, 64), "1 <= n_bands <= 4"), ((1e6, bands(), 0, 64), "1 <= n_bands <= 4"), ((1e6, bands(5), 5, 64), "1 <= n_bands <= 4")]
    cases += [((fs, bands(), 1, 64), "fs_in must be a whole number of Hz in [1, 2^31)") for fs in (0.0, 0.5, 1000.5, 2147483648.0, NAN)]
    cases += [((1e6, bands(), 1, n), "1 <= max_in_samples <= 2^30") for n in (0, (1 << 30) + 1)]
    cases += [((1e6, bands(if_hz=f), 1, 64), "if_hz must be a whole number of Hz") for f in (0.5, 9.0e15, NAN)]
    cases += [((1e6, bands(decimation=0), 1, 64), "decimation >= 1")]
    cases += [((1e6, bands(**c), 1, 64), "1 <= n_taps <= 4096") for c in (dict(taps=null_taps), dict(n_taps=0), dict(n_taps=4097))]
    cases += [((1e6, bands(decimation=65), 1, 64), "max_in_samples below a band's decimation")]
    for (fs, arr, nb, max_in), text in cases:
        R.expect("gnsship_cond_create", (ctx.h, fs, arr, nb, max_in, ctypes.byref(h)), text)
        assert h.value is None
        h = ctypes.c_void_p(1)
    R.silent("gnsship_cond_create", (None, 1e6, bands(), 1, 64, ctypes.byref(h)))
    R.silent("gnsship_cond_create", (ctx.h, 1e6, bands(), 1, 64, None))
    n = ctypes.c_int()
    for args in ((1e6, 2, 0.0, 0.0, None, 0, None), (1e6, 0, 0.0, 0.0, None, 0, ctypes.byref(n)), (0.0, 2, 0.0, 0.0, None, 0, ctypes.byref(n)),
                 (NAN, 2, 0.0, 0.0, None, 0, ctypes.byref(n)), (1e6, 2, -1.0, 0.0, None, 0, ctypes.byref(n)), (1e6, 2, 0.0, -1.0, None, 0, ctypes.byref(n))):
        R.silent("gnsship_cond_lowpass_taps", args)
    for fmt in (-1, 6, 0x100 | (3 << 4), 0x100 | (8 << 4), 0x100 | (2 << 4) | (3 << 2)):  # packed: 3 and 8 bits, components 3
        assert ctx.lib.gnsship_cond_fmt_bits(fmt) == 0, fmt
    for name, args in (("reset", (None, 0)), ("samples_in", (None, ctypes.byref(ctypes.c_uint64()))), ("destroy", (None,))):
        R.silent(f"gnsship_cond_{name}", args)

    abi.check(ctx.lib.gnsship_cond_create(ctx.h, 1e6, bands(), 1, 64, ctypes.byref(h)), "create", ctx.h)
    try:
        x = np.zeros(64, np.complex64)
        tail = (None, None, None, None)
        for on_device in (0, 1):
            for ptr, fmt in ((None, abi.FMT_CF32), (vp(x), -1), (vp(x), 6)):
                R.expect("gnsship_cond_run", (h, ptr, fmt, on_device, 64, *tail), "null input or unknown sample format")
            for n_in in (0, -2, 66):
                R.expect("gnsship_cond_run", (h, vp(x), abi.FMT_CF32, on_device, n_in, *tail), "1 <= n_in <= max_in_samples")
            R.expect("gnsship_cond_run", (h, vp(x), abi.FMT_CF32, on_device, 63, *tail), "n_in must be a multiple of every band's decimation")
            # four 2-bit real samples in a byte: 2 and 62 are whole multiples of the decimation, not of 4
            for n_in in (2, 62):
                R.expect("gnsship_cond_run", (h, vp(x), abi.FMT_NSR, on_device, n_in, *tail),
                         "n_in must be a multiple of the samples per byte of a packed format")
        R.expect("gnsship_cond_reset", (h, (1 << 62)), "first_sample below 2^62")
        R.silent("gnsship_cond_samples_in", (h, None))
        R.silent("gnsship_cond_run", (None, vp(x), abi.FMT_CF32, 0, 64, *tail))
        count = ctypes.c_uint64(7)
        abi.check(ctx.lib.gnsship_cond_samples_in(h, ctypes.byref(count)), "samples_in", ctx.h)
        assert count.value == 0  # no rejected run counted its samples
    finally:
        assert ctx.lib.gnsship_cond_destroy(h) == abi.OK
    assert R.seen == len(cases) + 2 + 6 + 3 + 2 * 9 + 3


def test_mitigation(ctx):
    R, h = Rejections(ctx), ctypes.c_void_p(1)
    ok = dict(kind=abi.MIT_NOTCH_LITE, pfa=0.001, threshold=0.0, p_c_factor=0.9, length=2, n_segments_est=4, n_segments_reset=100,
              n_segments_coeff=1, chain_form=abi.MIT_CHAIN_AUTO)
    pfa = "pfa must be in (0, 1) when no threshold is given"
    cases = [(None, 64, "null configuration"), (dict(kind=-1), 64, "unknown kind"), (dict(kind=3), 64, "unknown kind"),
             (dict(length=1), 64, "2 <= length <= 1024"), (dict(length=1025), 64, "2 <= length <= 1024"),
             (dict(n_segments_est=0), 64, "n_segments_est >= 1"), (dict(n_segments_coeff=0), 64, "n_segments_coeff >= 1"),
             (dict(chain_form=-1), 64, "unknown chain form"), (dict(chain_form=3), 64, "unknown chain form"),
             ({}, 0, "1 <= max_in_samples <= 2^30"), ({}, (1 << 30) + 1, "1 <= max_in_samples <= 2^30"),
             (dict(pfa=0.0), 64, pfa), (dict(pfa=1.0), 64, pfa), (dict(pfa=NAN), 64, pfa),
             (dict(pfa=0.0, threshold=-1.0), 64, pfa), (dict(pfa=NAN, threshold=NAN), 64, pfa)]  # a threshold that is not above 0 is none
    for changed, max_in, text in cases:
        conf = None if changed is None else ctypes.byref(abi.MitConf(**{**ok, **changed}))
        R.expect("gnsship_mit_create", (ctx.h, conf, max_in, ctypes.byref(h)), text)
        assert h.value is None
        h = ctypes.c_void_p(1)
    R.silent("gnsship_mit_create", (None, ctypes.byref(abi.MitConf(**ok)), 64, ctypes.byref(h)))
    R.silent("gnsship_mit_create", (ctx.h, ctypes.byref(abi.MitConf(**ok)), 64, None))
    t = ctypes.c_float()
    for args in ((0.01, 2, None), (0.0, 2, ctypes.byref(t)), (1.0, 2, ctypes.byref(t)), (NAN, 2, ctypes.byref(t)), (0.01, 1, ctypes.byref(t)),
                 (0.01, 1025, ctypes.byref(t))):
        R.silent("gnsship_mit_threshold", args)
    for name, args in (("reset", (None,)), ("state_get", (None, ctypes.byref(abi.MitState()))), ("destroy", (None,))):
        R.silent(f"gnsship_mit_{name}", args)

    # n_segments_coeff is the notch-lite filter's: the other two kinds take any value
    for kind in (abi.MIT_PULSE_BLANKING, abi.MIT_NOTCH):
        abi.check(ctx.lib.gnsship_mit_create(ctx.h, ctypes.byref(abi.MitConf(**{**ok, "kind": kind, "n_segments_coeff": 0})), 64, ctypes.byref(h)),
                  "create", ctx.h)
        assert ctx.lib.gnsship_mit_destroy(h) == abi.OK
    abi.check(ctx.lib.gnsship_mit_create(ctx.h, ctypes.byref(abi.MitConf(**ok)), 64, ctypes.byref(h)), "create", ctx.h)
    try:
        x = np.zeros(64, np.complex64)
        for on_device in (0, 1):
            for n_in in (-1, 65):
                R.expect("gnsship_mit_run", (h, vp(x), on_device, n_in, None, None, None, None), "0 <= n_in <= max_in_samples")
            R.expect("gnsship_mit_run", (h, None, on_device, 1, None, None, None, None), "null input")
        R.silent("gnsship_mit_state_get", (h, None))
        R.silent("gnsship_mit_run", (None, vp(x), 0, 64, None, None, None, None))
        st = abi.MitState()
        abi.check(ctx.lib.gnsship_mit_state_get(h, ctypes.byref(st)), "state_get", ctx.h)
        assert (st.samples_in, st.samples_out, st.pending_samples) == (0, 0, 0)  # no rejected run took its samples
    finally:
        assert ctx.lib.gnsship_mit_destroy(h) == abi.OK
    assert R.seen == len(cases) + 2 + 6 + 3 + 6 + 2


def test_viterbi(ctx):
    R, h = Rejections(ctx), ctypes.c_void_p(1)
    ok = dict(constraint_length=7, rate_n=2, g=(ctypes.c_int32 * 2)(121, 91), data_length=10, interleaver_rows=0, interleaver_cols=0, invert_g2=0,
              mode=abi.VIT_MODE_REFERENCE)
    g = lambda a, b: (ctypes.c_int32 * 2)(a, b)  # noqa: E731
    length, product = "data_length >= 1 and 2*(data_length + 6) <= 1024 symbols", "interleaver_rows*interleaver_cols must equal 2*(data_length + 6)"
    cases = [(None, 2, "null configuration"), (dict(constraint_length=6), 2, "constraint_length 7 and rate_n 2 only"),
             (dict(rate_n=3), 2, "constraint_length 7 and rate_n 2 only"),
             (dict(g=g(-1, 91)), 2, "g[] must be 7-bit words"), (dict(g=g(121, 128)), 2, "g[] must be 7-bit words"),
             (dict(data_length=0), 2, length), (dict(data_length=507), 2, length),
             (dict(interleaver_rows=8, interleaver_cols=0), 2, product), (dict(interleaver_rows=0, interleaver_cols=4), 2, product),
             (dict(interleaver_rows=-4, interleaver_cols=-8), 2, product), (dict(interleaver_rows=8, interleaver_cols=5), 2, product),
             (dict(mode=-1), 2, "unknown mode"), (dict(mode=2), 2, "unknown mode"),
             ({}, 0, "1 <= max_channels <= 2^20"), ({}, (1 << 20) + 1, "1 <= max_channels <= 2^20")]
    for changed, nch, text in cases:
        conf = None if changed is None else ctypes.byref(abi.VitConf(**{**ok, **changed}))
        R.expect("gnsship_vit_create", (ctx.h, conf, nch, ctypes.byref(h)), text)
        assert h.value is None
        h = ctypes.c_void_p(1)
    R.silent("gnsship_vit_create", (None, ctypes.byref(abi.VitConf(**ok)), 2, ctypes.byref(h)))
    R.silent("gnsship_vit_create", (ctx.h, ctypes.byref(abi.VitConf(**ok)), 2, None))
    sec = np.full(64, 5.0, np.float32)
    for name, args in (("reset_channel", (None, 0)), ("state_get", (None, 0, abi.fptr(sec))), ("destroy", (None,))):
        R.silent(f"gnsship_vit_{name}", args)

    abi.check(ctx.lib.gnsship_vit_create(ctx.h, ctypes.byref(abi.VitConf(**ok)), 2, ctypes.byref(h)), "create", ctx.h)
    try:
        sym = np.ones((3, 32), np.float32)
        i32p = ctypes.POINTER(ctypes.c_int32)

        def chans(*c):
            a = np.array(c, np.int32)
            return a, a.ctypes.data_as(i32p)

        keep, two = chans(0, 1)
        for on_device in (0, 1):
            for n in (-1, (1 << 22) + 1):
                R.expect("gnsship_vit_run", (h, vp(sym), on_device, n, two, None, None, None), "0 <= n_frames <= 2^22")
            R.expect("gnsship_vit_run", (h, None, on_device, 2, two, None, None, None), "null symbols or channels")
            R.expect("gnsship_vit_run", (h, vp(sym), on_device, 2, None, None, None, None), "null symbols or channels")
            for bad in ((0, -1), (2, 0)):
                keep_bad, p = chans(*bad)
                R.expect("gnsship_vit_run", (h, vp(sym), on_device, 2, p, None, None, None), "channel out of range")
            for twice in ((1, 1), (0, 1, 0)):
                keep_twice, p = chans(*twice)
                R.expect("gnsship_vit_run", (h, vp(sym), on_device, len(twice), p, None, None, None),
                         "a channel may appear once per call in reference mode")
        for ch in (-1, 2):
            R.expect("gnsship_vit_reset_channel", (h, ch), "channel out of range")
            R.expect("gnsship_vit_state_get", (h, ch, abi.fptr(sec)), "channel out of range")
        R.silent("gnsship_vit_state_get", (h, 0, None))
        R.silent("gnsship_vit_run", (None, vp(sym), 0, 2, two, None, None, None))
        assert (sec == 5.0).all()
        assert ctx.lib.gnsship_vit_run(h, None, 0, 0, None, None, None, None) == abi.OK  # no frame: nothing is read
    finally:
        assert ctx.lib.gnsship_vit_destroy(h) == abi.OK
    assert R.seen == len(cases) + 2 + 3 + 2 * 8 + 4 + 2
