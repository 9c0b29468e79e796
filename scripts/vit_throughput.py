#!/usr/bin/env python3
"""Throughput of the device Viterbi decoder (gnsship_vit_run) on Galileo I/NAV page parts: 163 840 frames of 240
symbols resident on the device, one per channel — what the headline channel count (README.md) produces in one
second, so real time needs 163 840 frames/s.  Both modes: "reference" (Viterbi_Decoder::decode as written) and
"full" (both symbols in the metric).

The frames are encoded random bits (K = 7, G1 = 171o, G2 = 133o inverted, 8 × 30 interleaver), ±1 symbols plus
Gaussian noise of sigma 0.3.  A run is one gnsship_vit_run over all frames: the upload of the per-frame channel
numbers, the decode kernel, the bits left on the device.  Timed with HIP events on the context stream: warm-up runs,
then the median of the timed runs.  Prints frames/s per mode, its ratio to real time, and the bit errors of the last
run against the encoded bits.  One JSON line at the end carries every figure.

Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS = 163_840
ROWS, COLS, LL = 8, 30, 114
G = (0o171, 0o133)


def encode_pages(bits):
    """bits uint8[n, LL] → float32[n, 240] as transmitted: encoded with 6 tail bits, G2 inverted, interleaved."""
    n = bits.shape[0]
    tail = np.concatenate([bits.astype(np.int64), np.zeros((n, 6), np.int64)], axis=1)
    state = np.zeros(n, np.int64)
    sym = np.zeros((n, 2 * (LL + 6)), np.float32)

    def parity(x):
        p = np.zeros_like(x)
        for k in range(7):
            p ^= (x >> k) & 1
        return p

    for t in range(LL + 6):
        w = (tail[:, t] << 6) ^ state
        sym[:, 2 * t] = 2 * parity(w & G[0]) - 1
        sym[:, 2 * t + 1] = -(2 * parity(w & G[1]) - 1)
        state = w >> 1
    # the interleaver: written column-wise into 30 × 8, read row-wise (the de-interleaver's inverse)
    return np.ascontiguousarray(sym.reshape(n, COLS, ROWS).swapaxes(1, 2)).reshape(n, ROWS * COLS)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=CHANNELS)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("vit_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    from gnss_sim_receiver_amd import engine

    n = args.frames
    rng = np.random.default_rng(11)
    truth = rng.integers(0, 2, (n, LL)).astype(np.uint8)
    sym = encode_pages(truth)
    sym += (args.sigma * rng.standard_normal(sym.shape, dtype=np.float32))
    channels = np.arange(n, dtype=np.int32)
    out = {"frames": n, "frame_symbols": ROWS * COLS, "sigma": args.sigma, "real_time_frames_per_s": CHANNELS, "lines": []}
    with engine.Context(0) as ctx:
        src = ctx.upload(sym)
        dst = engine.DeviceBuffer(ctx, n * LL)
        for mode in ("reference", "full"):
            dec = engine.galileo_inav_page_decoder(ctx, n, mode=mode)
            run = lambda: dec.run(src.ptr, channels, on_device=True, bits_dev=dst.ptr, host=False)
            for _ in range(args.warmup):
                run()
            ctx.sync()
            ms = []
            for _ in range(max(5, args.runs)):
                ctx.event_record(0)
                run()
                ctx.event_record(1)
                ctx.sync()
                ms.append(ctx.event_elapsed_ms(0, 1))
            med, lo, hi = statistics.median(ms), min(ms), max(ms)
            # bit errors of new objects on these frames (the timed runs carried their metrics on)
            for c in range(0, n, max(1, n // 64)):
                dec.reset_channel(c)
            sample = np.arange(0, n, max(1, n // 64), dtype=np.int32)
            got = dec.run(np.ascontiguousarray(sym[sample]), sample)
            errors = int(np.count_nonzero(got != truth[sample]))
            dec.close()
            fps = n / (med * 1e-3)
            line = {"mode": mode, "ms_median": med, "ms_min": lo, "ms_max": hi, "frames_per_s": fps, "x_real_time": fps / CHANNELS,
                    "sample_frames": int(sample.size), "sample_bit_errors": errors}
            out["lines"].append(line)
            print(f"{mode:10s}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) for {n} frames = {fps:,.0f} frames/s, "
                  f"{line['x_real_time']:.0f}x the {CHANNELS} frames/s of real time; {errors} bit errors in {sample.size} new-object frames")
        src.free()
        dst.free()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
