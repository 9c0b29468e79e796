"""Time the GLONASS FDMA acquisition sweep against one single-grid run per frequency channel.

    python scripts/glo_acq_sweep_time.py [--fs 10000000] [--runs 30]

All 14 frequency channels, ±5 kHz in 500 Hz steps, one 1 ms dwell of a resident device buffer, no grid kept.
Each figure is the median over --runs timed repetitions (after 5 discarded ones) of the time between two events on
the context's stream around the calls; the single-grid figure times the 14 runs only, not the 14 set_grid calls that
rebuild the wipe-off table on the host between them (those are reported separately, by the wall clock).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnss_sim_receiver_amd import codes, engine, signals  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=10000000)
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()
    fs, n, chans, dmax, step = a.fs, a.fs // 1000, list(range(-7, 7)), 5000, 500
    sats = [signals.Satellite(prn=1, doppler_hz=1500.0, code_delay_chips=17.4, cn0_dbhz=47.0, system="GLO_L1", freq_channel=k) for k in (-7, 0, 6)]
    x = signals.generate_if(fs, n, sats, seed=1)
    with engine.Context(0) as ctx:
        buf = ctx.upload(x)
        sweep = engine.glonass_l1_ca_pcps_acquisition(ctx, fs, dmax, step, freq_channels=chans)
        single = engine.PcpsAcquisition(ctx, fs, n, dmax, step, chip_rate=codes.GLONASS_L1_CA_CODE_RATE_CPS)
        single.set_local_code(codes.glonass_l1_ca_acquisition_code(fs))
        t_sweep, t_single, t_grids = [], [], []
        for i in range(a.runs + 5):
            ctx.event_record(0)
            sweep.run_fdma(buf)
            ctx.event_record(1)
            ctx.sync()
            ms, wall = 0.0, 0.0
            for k in chans:
                t0 = time.perf_counter()
                single.set_grid(dmax, step, codes.glonass_doppler_bias_hz("1G", k))
                wall += time.perf_counter() - t0
                ctx.event_record(2)
                single.run(buf)
                ctx.event_record(3)
                ctx.sync()
                ms += ctx.event_elapsed_ms(2, 3)
            if i >= 5:
                t_sweep.append(ctx.event_elapsed_ms(0, 1))
                t_single.append(ms)
                t_grids.append(wall * 1e3)
        sweep.close()
        single.close()
        buf.free()
    print(f"fs {fs} N {n}: {len(chans)} channels x {sweep.n_bins} bins; median of {a.runs} runs")
    print(f"  FDMA sweep (one run_fdma)        {np.median(t_sweep):8.3f} ms  (min {min(t_sweep):.3f}, max {max(t_sweep):.3f})")
    print(f"  {len(chans)} single-grid runs             {np.median(t_single):8.3f} ms  (min {min(t_single):.3f}, max {max(t_single):.3f})")
    print(f"  their {len(chans)} set_grid calls (host)    {np.median(t_grids):8.3f} ms")


if __name__ == "__main__":
    main()
