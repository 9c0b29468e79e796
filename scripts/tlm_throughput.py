#!/usr/bin/env python3
"""Throughput of the device Galileo telemetry framing (gnsship_tlm_run_symbols) on I/NAV: 163 840 channels, one second
of symbols each (250 rounds) resident on the device — what the headline channel count (README.md) produces in one
second, so real time needs one run per second.

Two states of the frame-sync machine:
  locked     every channel in state 2 on a noiseless built stream: a ring append per symbol and one page part (de-interleave,
             G2, Viterbi, CRC-24Q) per channel and run;
  searching  every channel in state 0 on a full history of random signs: the preamble correlation after every symbol.
A run is one gnsship_tlm_run_symbols over all channels with the symbols on the device and no host copy of the outputs.
Timed with HIP events on the context stream: warm-up runs, then the median of the timed runs.  One JSON line at the end
carries every figure.

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

CHANNELS = 163_840
ROUNDS = 250


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=CHANNELS)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="reference", choices=["reference", "full"])
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("tlm_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import tlm_model as M
    from gnss_sim_receiver_amd import abi, engine

    n = args.channels
    g = M.GEOMETRY[M.INAV]
    lead = 40
    locked_at = lead + g.required + 1 + g.period  # state 2 from here on
    first = -(-locked_at // ROUNDS) * ROUNDS
    total = first + (args.warmup + max(5, args.runs)) * ROUNDS
    x = M.build_stream(M.INAV, M.four_parts(M.INAV, 5), total, lead, 6)
    rng = np.random.default_rng(11)
    out = {"channels": n, "rounds_per_run": ROUNDS, "mode": args.mode, "lines": []}
    with engine.Context(0) as ctx:
        buf = engine.DeviceBuffer(ctx, 4 * ROUNDS * n)

        def timed(dec, blocks, label, check):
            ms = []
            for k, blk in enumerate(blocks):
                buf.upload(np.ascontiguousarray(np.repeat(blk[:, None], n, axis=1), np.float32))
                ctx.event_record(0)
                dec.run_symbols(buf.ptr, on_device=True, n_rounds=ROUNDS, host=False)
                ctx.event_record(1)
                ctx.sync()
                if k >= args.warmup:
                    ms.append(ctx.event_elapsed_ms(0, 1))
            med, lo, hi = statistics.median(ms), min(ms), max(ms)
            st = dec.state(n - 1)
            line = {"state": label, "ms_median": med, "ms_min": lo, "ms_max": hi, "channel_seconds_per_s": n / (med * 1e-3),
                    "x_real_time": 1e3 / med, "last_channel": st}
            check(st)
            out["lines"].append(line)
            print(f"{label:10s}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) per second of symbols of {n} channels = "
                  f"{line['x_real_time']:.0f}x real time; channel {n - 1}: stat {st['stat']}, crc errors {st['crc_error_counter']}")

        dec = engine.galileo_inav_telemetry(ctx, n, ROUNDS, mode=args.mode)
        for k in range(0, first, ROUNDS):  # to state 2
            buf.upload(np.ascontiguousarray(np.repeat(x[k:k + ROUNDS, None], n, axis=1), np.float32))
            dec.run_symbols(buf.ptr, on_device=True, n_rounds=ROUNDS, host=False)
        assert dec.state(0)["stat"] == 2 and dec.state(n - 1)["stat"] == 2

        def locked(st):
            assert st["stat"] == 2 and st["frame_sync"] == 1 and st["crc_error_counter"] == 0, st

        timed(dec, [x[k:k + ROUNDS] for k in range(first, total, ROUNDS)], "locked", locked)
        dec.close()

        dec = engine.galileo_inav_telemetry(ctx, n, ROUNDS, mode=args.mode)
        noise = M.lead_in(M.INAV, total + g.P, 9)[:total]  # random signs with no preamble in them: the search never ends
        for k in range(0, first, ROUNDS):
            buf.upload(np.ascontiguousarray(np.repeat(noise[k:k + ROUNDS, None], n, axis=1), np.float32))
            dec.run_symbols(buf.ptr, on_device=True, n_rounds=ROUNDS, host=False)

        def searching(st):
            assert st["stat"] == 0 and st["history_size"] == g.required + 1, st

        timed(dec, [noise[k:k + ROUNDS] for k in range(first, total, ROUNDS)], "searching", searching)
        dec.close()
        buf.free()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
