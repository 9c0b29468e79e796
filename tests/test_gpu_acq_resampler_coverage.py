"""The acquisition resampler (acq_resampler.hip) on the device over every tile shape, tap parity and LDS size of
tests/acq_resampler_cases.py, against oracle.FirDecimator.

Contract, as in tests/test_gpu_acq_resampler.py: decimated samples bit-equal to the oracle's serial float dot products,
history carried across calls.  The taps are asymmetric (seeded normal values / n_taps), so a reversed or mirrored tap
window cannot pass: tests/test_acq_resampler_cases.py shows on the oracle alone that reversed taps change the output
in every call of the pattern used here, and recomputes the tile (opb) and LDS figures of the table.

Per shape: a stream of D·nk samples with at least three tiles, the last one partial; calls of D, D, 7·D samples and the
rest (single outputs; where n_taps − 1 > D two successive calls shorter than the history); then a reset, after which
the first 10·D samples again equal a new oracle object.  The automatic designs for 100 and 80 Msps input, the
realistic shapes whose tiles are cut short and whose LDS passes 64 KiB, run with their own (symmetric) taps."""
import numpy as np
import pytest

import acq_resampler_cases as C
from gnss_sim_receiver_amd import abi, engine
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FMT = {"cf32": abi.FMT_CF32, "ci16": abi.FMT_CI16, "ci8": abi.FMT_CI8}


def bits(y):
    return np.ascontiguousarray(y, np.complex64).view(np.uint32)


def check_streaming(ctx, taps, d, fmt, seed, on_device=False):
    t = len(taps)
    nk = C.n_outputs(t, d)
    n = d * nk
    raw, x = C.stream(fmt, n, seed)
    per = 1 if fmt == "cf32" else 2
    r = engine.AcqResampler(ctx, taps, d, n)
    ref = O.FirDecimator(taps, d)
    src = ctx.upload(raw) if on_device else None
    cuts = C.cuts(d, nk)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if on_device:
            ptr, n_out = r.run(src.ptr + a * per * raw.itemsize, fmt=FMT[fmt], on_device=True, n_in=b - a)
            assert n_out == (b - a) // d
            ctx.sync()
            out = engine.DeviceBuffer.wrap(ctx, ptr, 8 * n_out).download(np.empty(n_out, np.complex64))
        else:
            out = r.run(raw[a * per: b * per])
        exp = ref(x[a:b])
        assert len(out) == (b - a) // d
        assert np.array_equal(bits(out), bits(exp)), (t, d, fmt, a, b, float(np.max(np.abs(out - exp))))
    r.reset()
    again = r.run(raw[: 10 * d * per])
    assert np.array_equal(bits(again), bits(O.FirDecimator(taps, d)(x[: 10 * d])))
    r.close()
    if src is not None:
        src.free()


@pytest.mark.parametrize("name,t,d,fmt", C.cases(), ids=[c[0] for c in C.cases()])
def test_asymmetric_taps_every_tile_shape(ctx, name, t, d, fmt):
    print(f"{name}: opb {C.opb_of(t, d)}, dynamic LDS {C.lds_bytes(t, d)} B, {C.n_outputs(t, d)} outputs")
    check_streaming(ctx, C.asymmetric_taps(t), d, fmt, seed=t + d)


@pytest.mark.parametrize("key,fmt", list(zip(C.DESIGNS, C.FORMATS)), ids=["100M-2M-cf32", "100M-1M-ci16", "80M-2M-ci8"])
def test_automatic_designs_above_64_kib(ctx, key, fmt):
    d, taps = engine.acq_resampler_design(ctx.lib, *key)
    assert (len(taps), d) == C.DESIGN_SHAPES[key][:2]
    assert C.lds_bytes(len(taps), d) > 65536 and C.opb_of(len(taps), d) < 256
    check_streaming(ctx, taps, d, fmt, seed=d)


def test_device_pointer_input(ctx):
    (t, d), fmt = C.DEVICE_INPUT
    check_streaming(ctx, C.asymmetric_taps(t), d, fmt, seed=t + d, on_device=True)
