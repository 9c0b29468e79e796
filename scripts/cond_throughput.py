#!/usr/bin/env python3
"""Throughput of the signal conditioner (gnsship_cond_run) at the C5 shape, and what it buys the channels.

1. Conditioner: 50 Msps ibyte, two bands at ±7 161 000 Hz, decimation 5, the adapter's default low-pass
   taps (241) — one launch per block conditions both bands.  Timed with HIP events on the context stream:
   warm-up runs, then the median of the timed runs.  Prints the input rate in Msps and the real-time
   factor (input rate / 50 Msps).  Condition: the factor must exceed 1 on one GPU (exit status 1 otherwise).
2. Channels, for information: 12 GPS L1 C/A channels in closed loop, time per 1 ms epoch of all 12,
   (a) on the conditioned 10 Msps band (if_hz = 0, N = 10000) and (b) as before this stage existed, on the
   50 Msps ibyte stream with the IF fused into the carrier NCO (if_hz = 7 161 000, N = 50000).

--fmt times part 1 with another input form of the same random stream (real int8, or random bytes of a packed
form; the channels of part 2 read ibyte and run with --fmt ci8 only).  --shape twobit-packed is the shape of the
reference's packed configuration instead (conf/gnss-sdr_GPS_L1_nsr_twobit_packed.conf:35-91: 20.48 Msps, one band
at IF 5 500 000 Hz — the configuration's non-integer IF rounded to whole Hz —, decimation 8, default low-pass taps).

Needs a GPU.  One JSON line at the end carries every figure.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 50_000_000
F_IF = 7_161_000
DECIM = 5
# --shape: (input rate, band centres, decimation)
SHAPES = {"c5": (FS, [F_IF, -F_IF], DECIM), "twobit-packed": (20_480_000, [5_500_000], 8)}


def input_forms(abi):
    """--fmt name -> (format value, bytes per sample)."""
    two = abi.fmt_two_bit_packed
    return {"ci8": (abi.FMT_CI8, 2.0), "ri8": (abi.FMT_RI8, 1.0), "2bit-real": (two("real"), 0.25), "2bit-iq": (two("iq"), 0.5),
            "4bit-iq": (abi.fmt_four_bit_cpx("iq"), 1.0), "nsr": (abi.FMT_NSR, 0.25), "2bit-cpx": (abi.FMT_TWO_BIT_CPX, 0.5)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--block-ms", type=int, default=100, help="samples per gnsship_cond_run, in ms of the 50 Msps stream")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=160, help="timed tracking epochs")
    ap.add_argument("--repeats", type=int, default=5, help="tracking timings (median reported)")
    ap.add_argument("--no-channels", action="store_true")
    ap.add_argument("--fmt", default="ci8", help="input form of the conditioner run: ci8, ri8, 2bit-real, 2bit-iq, 4bit-iq, nsr, 2bit-cpx")
    ap.add_argument("--shape", default="c5", choices=sorted(SHAPES))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("cond_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    from gnss_sim_receiver_amd import abi, engine, signals

    forms = input_forms(abi)
    if args.fmt not in forms:
        print(f"cond_throughput: --fmt must be one of {sorted(forms)}", file=sys.stderr)
        return 2
    fmt, sample_bytes = forms[args.fmt]
    fs, centres, decim = SHAPES[args.shape]
    out = {"fs_in": fs, "bands_hz": centres, "decimation": decim, "fmt": args.fmt}
    with engine.Context(0) as ctx:
        taps = engine.cond_lowpass_taps(ctx.lib, float(fs), decim)
        out["n_taps"] = len(taps)
        n_in = fs // 1000 * args.block_ms
        rng = np.random.default_rng(5)
        if args.fmt == "ci8":
            raw = rng.integers(-100, 101, 2 * n_in, dtype=np.int8)
        elif args.fmt == "ri8":
            raw = rng.integers(-100, 101, n_in, dtype=np.int8)
        else:
            raw = rng.integers(0, 256, int(n_in * sample_bytes), dtype=np.uint8)
        src = ctx.upload(raw)
        cond = engine.SignalConditioner(ctx, fs, [(f, decim, taps) for f in centres], n_in)
        for _ in range(args.warmup):
            cond.run(src.ptr, fmt=fmt, on_device=True, n_in=n_in)
        ctx.sync()
        ms = []
        for _ in range(max(10, args.runs)):
            ctx.event_record(0)
            cond.run(src.ptr, fmt=fmt, on_device=True, n_in=n_in)
            ctx.event_record(1)
            ctx.sync()
            ms.append(ctx.event_elapsed_ms(0, 1))
        med = statistics.median(ms)
        msps = n_in / med / 1e3
        rtf = msps * 1e6 / fs
        # algorithmic bytes: s B in + sum_b 8/D_b B out per input sample
        gbs = n_in * (sample_bytes + len(centres) * 8 / decim) / med / 1e6
        out.update(block_samples=n_in, cond_ms_median=med, cond_ms_min=min(ms), cond_ms_max=max(ms), input_msps=msps, real_time_factor=rtf,
                   algorithmic_gb_s=gbs)
        print(f"conditioner, {args.fmt} in: {n_in} samples per run, {len(centres)} band{'s' if len(centres) > 1 else ''}, {len(taps)} taps, "
              f"D {decim}: median {med:.3f} ms over {len(ms)} runs "
              f"(min {min(ms):.3f}, max {max(ms):.3f}) = {msps:.0f} Msps in, {rtf:.1f}x real time of the {fs / 1e6:g} Msps stream, "
              f"{gbs:.1f} GB/s algorithmic")
        cond.close()
        src.free()

        if not args.no_channels and args.fmt == "ci8" and args.shape == "c5":
            n_ch = 12
            rng = np.random.default_rng(0x6E550005)
            sats = [signals.Satellite(prn=p, doppler_hz=float(rng.uniform(-4000, 4000)), code_delay_chips=float(rng.uniform(0, 1000)),
                                      cn0_dbhz=47.0, carrier_phase_rad=float(rng.uniform(0, 6.28)), f_if_hz=float(F_IF), bits="1000101100110")
                    for p in range(1, n_ch + 1)]
            warm = 40
            total = warm + args.epochs
            n = (total + 4) * (FS // 1000)
            x = signals.generate_if_device(float(FS), n, sats, seed=7, start=0, device="cuda")
            iq = torch.view_as_real(x).reshape(-1)
            raw_t = torch.clamp(torch.round(iq * 8.0), -127, 127).to(torch.int8).contiguous()
            del x, iq
            torch.cuda.synchronize()
            # the conditioned band, whole, in the caller's buffer (GPS band only is what the channels read)
            cond = engine.SignalConditioner(ctx, FS, [(F_IF, DECIM, taps), (-F_IF, DECIM, taps)], n)
            band = engine.DeviceBuffer(ctx, 8 * (n // DECIM))
            cond.run(raw_t.data_ptr(), fmt=abi.FMT_CI8, on_device=True, n_in=n, dev_dst=[band.ptr, None])
            ctx.sync()
            cond.close()
            group_delay = (len(taps) - 1) / 2.0 / DECIM

            def time_loop(fs, fmt, ptr, n_buf, if_hz, extra_delay):
                vl = int(fs // 1000)
                res = []
                for _ in range(args.repeats):
                    conf = abi.TrkConf.defaults(abi.SYS_GPS_L1CA, float(fs), vl, if_hz=float(if_hz))
                    trk = engine.DllPllVemlTracking(ctx, conf, n_ch)
                    for ch, s in enumerate(sats):
                        ctx.set_code(ch, s.code)
                        trk.start(ch, ch, signals.acq_delay_samples(s, float(fs), 0, 0) + extra_delay + 0.2, s.doppler_hz + 15.0, 0, 0, prn=s.prn)
                    done = trk.run_ptr(ptr, fmt, 0, n_buf, warm)
                    t0 = time.perf_counter()
                    done2 = trk.run_ptr(ptr, fmt, 0, n_buf, args.epochs)  # returns after the device finished
                    dt = time.perf_counter() - t0
                    states = trk.states()
                    trk.close()
                    if done != warm or done2 != args.epochs or np.any(states < 2):
                        raise RuntimeError(f"tracking at {fs} sps: rounds {done}+{done2}, states {states.tolist()}")
                    res.append(dt * 1e3 / args.epochs)
                return statistics.median(res)

            ms_cond = time_loop(FS // DECIM, abi.FMT_CF32, band.ptr, n // DECIM, 0.0, group_delay)
            ms_if = time_loop(FS, abi.FMT_CI8, raw_t.data_ptr(), n, float(F_IF), 0.0)
            cond_ms_per_epoch = med / args.block_ms
            out.update(channels=n_ch, trk_ms_per_epoch_conditioned_10msps=ms_cond, trk_ms_per_epoch_if_50msps=ms_if,
                       cond_ms_per_epoch_of_stream=cond_ms_per_epoch)
            print(f"{n_ch} GPS channels, closed loop, per 1 ms epoch of all channels: {ms_cond:.4f} ms on the conditioned 10 Msps band "
                  f"(+ {cond_ms_per_epoch:.4f} ms of conditioner per ms of stream, both bands), {ms_if:.4f} ms at 50 Msps with if_hz")
            band.free()
    print(json.dumps(out))
    if not out["real_time_factor"] > 1.0:
        print("cond_throughput: the conditioner is slower than its input stream", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
