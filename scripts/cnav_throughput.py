#!/usr/bin/env python3
"""Throughput of the device GPS CNAV telemetry decoder (gnsship_cnav_run_symbols): symbols per second against the channel
count, for both signals.  Every channel carries the same noiseless built message stream, resident on the device; a run is
one call over all channels of one second of symbols (50 rounds for L2C, 100 for L5) with no host copy of the outputs, so
real time needs one run per second.  On such a stream both parts decode until one locks (after the first message); from
then on one part decodes 32 bits per 64 symbols and the other is flushed, which is the steady state timed here.

Timed with HIP events on the context stream: warm-up runs, then the median of the timed runs.  One line per signal and
channel count, and one JSON line at the end with every figure.  DESIGN.md records the result of a run on an MI355X.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHANNELS = (256, 4096, 32768, 163_840)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("cnav_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import cnav_model as M
    from gnss_sim_receiver_amd import abi, engine

    out = {"lines": []}
    with engine.Context(0) as ctx:
        for signal, name, rounds in ((abi.CNAV_L2C, "L2C", 50), (abi.CNAV_L5, "L5", 100)):
            timed_runs = args.warmup + max(5, args.runs)
            first = -(-704 // rounds) * rounds  # the first message comes out at symbol 704: locked from there on
            total = first + timed_runs * rounds
            x = M.to_float(M.stream(M.messages(total // 600 + 2, 5), 0, 5)[:total])
            for n in args.channels:
                dec = engine.GpsCnavTelemetryDecoder(ctx, signal, n, rounds)
                buf = engine.DeviceBuffer(ctx, 4 * rounds * n)
                ms = []
                for k in range(0, total, rounds):
                    buf.upload(np.ascontiguousarray(np.repeat(x[k:k + rounds, None], n, axis=1), np.float32))
                    ctx.event_record(0)
                    dec.run_symbols(buf.ptr, on_device=True, n_rounds=rounds, host=False)
                    ctx.event_record(1)
                    ctx.sync()
                    if k >= first + args.warmup * rounds:
                        ms.append(ctx.event_elapsed_ms(0, 1))
                st = dec.state(n - 1)
                assert st["part"][0]["message_lock"] == 1 and st["symbol_counter"] == total and st["valid_word"] == 1, st
                med = statistics.median(ms)
                line = {"signal": name, "channels": n, "rounds_per_run": rounds, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                        "symbols_per_s": n * rounds / (med * 1e-3), "x_real_time": 1e3 / med}
                out["lines"].append(line)
                print(f"{name:3s} {n:7d} channels: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) per second of symbols = "
                      f"{line['symbols_per_s']:.3e} symbols/s, {1e3 / med:.0f}x real time")
                buf.free()
                dec.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
