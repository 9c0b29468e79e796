#!/usr/bin/env python3
"""Throughput of the interference mitigation (gnsship_mit_run): pulse blanking, the notch in its serial and its
speculative chain form, and the notch lite, each on two device-resident CF32 streams in blocks of 2^20 samples:

  noise   unit-variance complex noise;
  cw      the same noise plus a continuous CW tone of 10σ: once the first estimation window is over the notches
          filter every segment, one unbroken run of the recursion y[n] = b[n] + a[n]·y[n−1] — the worst case
          for the chain.

The adapters' defaults throughout (length 32, segments_est 12500, segments_reset 5000000, pfa 0.04 / 0.001,
p_c_factor 0.9).  Timed with HIP events on the context stream: warm-up runs (they pass the estimation window),
then the median of the timed runs.  Every line carries the rate in Msamples/s, its ratio to real time at
50 Msps (the project's highest stream rate, C5) and, with --cond, to the single-band CF32 rate of the signal
conditioner (50 Msps, IF 7 161 000 Hz, decimation 5, the adapter's default low-pass taps), and the chain
counters.  Condition: the default (auto) form of the notch must exceed real time at 50 Msps on the cw stream
(exit status 1 otherwise).

Needs a GPU.  One JSON line at the end carries every figure.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS = 50_000_000
BLOCK = 1 << 20


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4, help="distinct blocks of the stream, cycled")
    ap.add_argument("--cond", action="store_true", help="also time the single-band CF32 signal conditioner")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("mit_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    from gnss_sim_receiver_amd import abi, engine

    out = {"block_samples": BLOCK, "real_time_msps": FS / 1e6, "lines": []}
    with engine.Context(0) as ctx:
        def timed(run):
            for _ in range(args.warmup):
                run(0)
            ctx.sync()
            ms = []
            for i in range(max(10, args.runs)):
                ctx.event_record(0)
                run(i)
                ctx.event_record(1)
                ctx.sync()
                ms.append(ctx.event_elapsed_ms(0, 1))
            return statistics.median(ms), min(ms), max(ms)

        rng = np.random.default_rng(5)
        n = BLOCK * args.blocks
        noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        cw = (noise + 10.0 * np.exp(2j * np.pi * 0.0731 * np.arange(n))).astype(np.complex64)
        streams = {"noise": ctx.upload(noise), "cw": ctx.upload(cw)}

        cond_msps = None
        if args.cond:
            taps = engine.cond_lowpass_taps(ctx.lib, float(FS), 5)
            n_cond = BLOCK // 5 * 5  # a multiple of the decimation
            cond = engine.SignalConditioner(ctx, FS, [(7_161_000, 5, taps)], n_cond)
            med, lo, hi = timed(lambda i: cond.run(streams["noise"].ptr + 8 * BLOCK * (i % args.blocks), fmt=abi.FMT_CF32, on_device=True, n_in=n_cond))
            cond.close()
            cond_msps = n_cond / med / 1e3
            out["cond_single_band_cf32_msps"] = cond_msps
            print(f"signal conditioner, CF32 in, 1 band, {len(taps)} taps, D 5: median {med:.3f} ms = {cond_msps:.0f} Msps, {cond_msps * 1e6 / FS:.1f}x real time")

        configs = [("pulse blanking", "pulse-blanking", "auto"), ("notch, serial", "notch", "serial"), ("notch, speculative", "notch", "speculative"),
                   ("notch, auto", "notch", "auto"), ("notch lite, auto", "notch-lite", "auto")]
        auto_cw = None
        for label, kind, form in configs:
            for sname, buf in streams.items():
                f = engine.InterferenceMitigation(ctx, kind, BLOCK, chain_form=form)
                med, lo, hi = timed(lambda i: f.run(buf.ptr + 8 * BLOCK * (i % args.blocks), on_device=True, n_in=BLOCK))
                st = f.state()
                f.close()
                msps = BLOCK / med / 1e3
                line = {"filter": label, "stream": sname, "ms_median": med, "ms_min": lo, "ms_max": hi, "msps": msps, "x_real_time": msps * 1e6 / FS,
                        "chain_form": st["chain_form"], "filter_state": st["filter_state"], "chunk_samples": st["chunk_samples"],
                        "warmup_samples": st["warmup_samples"], "chunks_speculated": st["chunks_speculated"], "chunks_replayed": st["chunks_replayed"]}
                if cond_msps:
                    line["x_conditioner"] = msps / cond_msps
                out["lines"].append(line)
                if label == "notch, auto" and sname == "cw":
                    auto_cw = line["x_real_time"]
                print(f"{label:20s} {sname:6s}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) = {msps:8.0f} Msps, {line['x_real_time']:6.1f}x real time"
                      + (f", {line['x_conditioner']:.2f}x the conditioner" if cond_msps else "")
                      + f"; form {st['chain_form']}, speculated {st['chunks_speculated']}, replayed {st['chunks_replayed']}")
        for b in streams.values():
            b.free()
    print(json.dumps(out))
    if not (auto_cw and auto_cw > 1.0):
        print("mit_throughput: the notch's default form is slower than a 50 Msps stream on the continuous-CW input", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
