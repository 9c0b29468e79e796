"""Packed real IF end to end on the GPU: the 2-bit real-sampled 16 Msps stream of tests/cond_ingest_scenarios.py
(GPS L1 C/A at +4 MHz, four samples to a byte as Two_Bit_Packed_File_Signal_Source reads them) is uploaded as it is
— 1.2 MB instead of 38 MB as gr_complex — and goes through the signal conditioner in three blocks into one device
buffer; acquisition and tracking then consume the conditioned 4 Msps band in place (device pointers), as in
tests/test_gpu_cond_dual_band.py.

Contract: the conditioned stream within the accuracy contract of the float64 model fed the unpacked samples;
acquisition's peak bin and code index equal the oracle acquisition's on the same device-conditioned samples and
sit within one Doppler bin and ±1 decimated sample of the synthetic truth; every field of all 294 tracking
records per channel equals the oracle loop's fed the same samples (test_gpu_trk.compare_exact)."""
import numpy as np
import pytest

from gnss_sim_receiver_amd import abi, engine

import cond_ingest_scenarios as P
import cond_model as M
import cond_scenarios as C
from test_gpu_trk import compare_exact, dev_conf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def conditioned(ctx):
    """(DeviceBuffer of the conditioned band, its host copy, taps)."""
    raw, _ = P.packed_stream()
    h = P.taps(lambda fs, d: engine.cond_lowpass_taps(ctx.lib, fs, d))
    n_out = P.N_IN // P.DECIM
    buf = engine.DeviceBuffer(ctx, 8 * n_out)
    src = ctx.upload(raw)
    assert src.nbytes == P.N_IN // 4 == 1_200_000
    block = 1_600_000
    cond = engine.SignalConditioner(ctx, P.FS, [(P.IF_HZ, P.DECIM, h)], block)
    for b0 in range(0, P.N_IN, block):
        dst = [buf.ptr + 8 * (b0 // P.DECIM)]
        got = cond.run(src.ptr + b0 // 4, fmt=P.FMT, on_device=True, n_in=block, dev_dst=dst)
        assert got == [(dst[0], block // P.DECIM)]
    assert cond.samples_in() == P.N_IN
    ctx.sync()
    y = buf.download(np.empty(n_out, np.complex64))
    cond.close()
    src.free()
    yield buf, y, h
    buf.free()


def test_conditioned_stream_meets_the_accuracy_contract(conditioned):
    """The first 40 000 outputs and the 40 000 across the second block edge against the float64 model."""
    _, y, h = conditioned
    x = P.packed_stream()[1]
    n = 40_000 * P.DECIM
    assert M.contract_ratio(y[:40_000], *M.model(x[:n], h, P.DECIM, P.IF_HZ, P.FS), len(h)) <= 1.0
    a = 1_600_000 - n // 2                 # input sample where the second window starts (a multiple of D)
    pre = len(h) - 1                       # the window's history, so its outputs see the samples before it
    assert pre % P.DECIM == 0 and a % P.DECIM == 0
    ref, bnd = M.model(x[a - pre: a + n], h, P.DECIM, P.IF_HZ, P.FS, first=a - pre)
    k = pre // P.DECIM
    assert M.contract_ratio(y[a // P.DECIM: (a + n) // P.DECIM], ref[k:], bnd[k:], len(h)) <= 1.0


def test_acquisition_and_tracking_on_the_conditioned_stream(ctx, conditioned):
    buf, y, h = conditioned
    system = P.SYSTEM
    fs = C.fs_out(system)
    a, n = C.dwell(system)
    sats = P.satellites()
    acq = engine.PcpsAcquisition(ctx, fs, n, C.DOPPLER_MAX, C.DOPPLER_STEP, 0, True, **C.acq_args(system))
    k = C.trk_conf(system)
    trk = engine.DllPllVemlTracking(ctx, dev_conf(k, system), len(sats))
    results = []
    for ch, sat in enumerate(sats):
        acq.set_local_code(C.local_code(system, sat.prn))
        (res,), _ = acq.run(engine.DeviceBuffer.wrap(ctx, buf.ptr + 8 * a, 8 * n), fmt=abi.FMT_CF32)
        ref = C.oracle_acquisition(system, sat.prn, y)
        assert (res.doppler_index, res.code_index, res.doppler_hz) == (ref.doppler_index, ref.code_index, ref.doppler_hz), sat.prn
        C.check_acquisition_against_truth(system, sat, res, len(h))
        results.append(res)
        ctx.set_code(100 + ch, sat.code)
        delay, dop, stamp, first = C.trk_start(system, res)
        trk.start(ch, 100 + ch, delay, dop, stamp, first, prn=sat.prn)
    acq.close()
    epochs = C.epochs(system)
    assert epochs == 294
    rec, rounds = trk.run(buf, 0, epochs, fmt=abi.FMT_CF32, n_buffer_samples=len(y))
    trk.close()
    assert rounds == epochs
    for ch, sat in enumerate(sats):
        ref = C.oracle_track(system, sat, y, results[ch])
        assert len(ref) == epochs
        compare_exact(rec[:, ch], ref, f"PRN {sat.prn} on the conditioned 2-bit stream")
        assert abs(ref["carrier_doppler_hz"][-1] - sat.doppler_hz) < 10.0
