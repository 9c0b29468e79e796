"""Throughput of the GLONASS tracking loop on the persistent generic pipeline: a measurement, not a gate.

    python scripts/glo_throughput.py [--channels 24] [--fs 10000000] [--epochs 60] [--runs 24]

24 GLONASS L1 C/A channels (PRN 1..24 on their table's frequency channels, 45 dB-Hz) at 10 Msps, each run from a fresh
start over --epochs epochs of a device-resident buffer, and beside it the same count of GPS L1 C/A channels on the
generic rotator at the same N on the engine they already had — the same kernel with dll_pll_veml_tracking's loop.
Timed with two events on the context's stream around the launch; the first 4 runs are discarded, the median (with the
spread) of the rest is reported, in channel-epochs per second and as a multiple of real time (24 channels of 1 ms
epochs in step).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnss_sim_receiver_amd import abi, codes, engine, signals  # noqa: E402


def measure(ctx, conf, sats, code_of, x, fs, epochs, runs):
    n_ch = len(sats)
    buf = ctx.upload(x)
    for ch, s in enumerate(sats):
        ctx.set_code(100 + ch, code_of(s))
    trk = engine.DllPllVemlTracking(ctx, conf, n_ch)
    starts = [(ch, 100 + ch, (s.code_delay_chips / s.code_freq()) * fs + 0.2, s.doppler_hz + 10.0, 0, 0, -1, s.prn) for ch, s in enumerate(sats)]
    times, ran = [], []
    for i in range(runs + 4):
        trk.start_many(starts)
        ctx.event_record(0)
        trk.launch_ptr(buf.ptr, abi.FMT_CF32, 0, len(x), epochs, records=True)
        ctx.event_record(1)
        rec, done = trk.collect()
        if i >= 4:
            times.append(ctx.event_elapsed_ms(0, 1))
            ran.append(int(np.count_nonzero(rec["flags"] & 8)))
    eng = trk.last_engine()
    trk.close()
    buf.free()
    return np.array(times), ran, eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=24)
    ap.add_argument("--fs", type=int, default=10000000)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--runs", type=int, default=24)
    a = ap.parse_args()
    fs, vl, n = float(a.fs), a.fs // 1000, (a.epochs + 3) * (a.fs // 1000)
    rng = np.random.Generator(np.random.PCG64(24))
    glo = [signals.Satellite(prn=1 + p % 24, doppler_hz=float(rng.uniform(-4000, 4000)), code_delay_chips=float(rng.uniform(0, 511)),
                             carrier_phase_rad=float(rng.uniform(0, 6.28)), cn0_dbhz=45.0, system="GLO_L1") for p in range(a.channels)]
    gps = signals.random_sky(a.channels, seed=24, cn0=45.0, prns=[1 + p % 32 for p in range(a.channels)])
    cases = [("GLONASS L1 C/A (trk_glo_loop.h)", engine.glonass_l1_ca_trk_conf(fs), glo, lambda s: codes.glonass_l1_ca_code_gen_float()),
             ("GPS L1 C/A, generic rotator", abi.TrkConf.defaults(abi.SYS_GPS_L1CA, fs, vl, rotator=abi.ROTATOR_GENERIC), gps, lambda s: s.code)]
    with engine.Context(0) as ctx:
        print(f"{a.channels} channels, fs {a.fs}, N {vl}, {a.epochs} epochs per run, median of {a.runs} runs after 4 discarded")
        for name, conf, sats, code_of in cases:
            x = signals.generate_if(fs, n, sats, seed=5)
            t, ran, eng = measure(ctx, conf, sats, code_of, x, fs, a.epochs, a.runs)
            med = float(np.median(t))
            ce = float(np.median(ran))
            print(f"  {name}: {abi.TRK_ENGINE_NAMES[eng]}; {med:.3f} ms per run (min {t.min():.3f}, max {t.max():.3f}); "
                  f"{int(ce)} channel-epochs per run; {ce / med * 1e3:.0f} channel-epochs/s; {a.epochs / med:.2f} x real time")


if __name__ == "__main__":
    main()
