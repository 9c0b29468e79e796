#!/usr/bin/env python3
"""Throughput of the device BeiDou D1/D2 telemetry decoder (gnsship_dnav_run_symbols, gnsship_dnav_run_records): one second
of symbols of 163 840 channels, which is 50 rounds for a D1 channel (20 ms symbols, PRN 20) and 500 for a D2 channel (2 ms
symbols, PRN 3), as floats (4 B an entry) and as tracking's epoch records (96 B an entry).  Every channel carries the same
noiseless built subframe stream; the inputs are made on the device, and a run is one call over all channels with no host
copy of the outputs, so real time needs one run per second.  The decoder is in state 2 from symbol 611 on (a decode every
300 symbols, the TOW stamped and counted in between), which is the steady state timed here.

Timed with HIP events on the context stream: warm-up runs, then the median of the timed runs.  One line per mode, input and
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

CHANNELS = (4096, 163_840)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("dnav_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import dnav_model as M
    import test_dnav_model as C
    from gnss_sim_receiver_amd import abi, engine

    out = {"lines": []}
    with engine.Context(0) as ctx:
        for name, prn, rounds in (("D1", 20, 50), ("D2", 3, 500)):
            timed_runs = args.warmup + max(5, args.runs)
            first = -(-611 // rounds) * rounds  # the first decode is at symbol 611: state 2 from there on
            total = first + timed_runs * rounds
            x = (C.d2_stream if name == "D2" else C.d1_stream)(0, total // 300 + 1, 100000)[:total]
            assert len(x) == total
            for n in args.channels:
                for records in (False, True):
                    dec = engine.BeidouDnavTelemetryDecoder(ctx, n, rounds, abi.DNAV_B3I)
                    for c in range(n):
                        dec.new_channel(c, prn)
                    if records:  # one round of records per sign, picked per round on the device
                        rows = np.zeros((2, n), abi.TRK_EPOCH_DTYPE)
                        rows["flags"] = 9
                        rows["prompt_i"][0], rows["prompt_i"][1] = -1.0, 1.0
                        rows_d = torch.from_numpy(rows.view(np.uint8).reshape(2, n, -1)).cuda()
                    ms = []
                    for k in range(0, total, rounds):
                        col = torch.from_numpy(np.ascontiguousarray(x[k:k + rounds])).cuda()
                        if records:
                            inp = rows_d[(col > 0).long()].contiguous()  # [rounds, n, 96]
                        else:
                            inp = col[:, None].expand(rounds, n).contiguous()
                        torch.cuda.synchronize()
                        ctx.event_record(0)
                        if records:
                            dec.run_records(inp.data_ptr(), on_device=True, n_rounds=rounds, host=False)
                        else:
                            dec.run_symbols(inp.data_ptr(), on_device=True, n_rounds=rounds, host=False)
                        ctx.event_record(1)
                        ctx.sync()
                        del inp
                        if k >= first + args.warmup * rounds:
                            ms.append(ctx.event_elapsed_ms(0, 1))
                    st = dec.state(n - 1)
                    assert st["stat"] == 2 and st["symbol_counter"] == total and st["valid_word"] == 1 and st["preamble_index"] > total - 300, st
                    med = statistics.median(ms)
                    entry = abi.TRK_EPOCH_DTYPE.itemsize if records else 4
                    line = {"mode": name, "input": "records" if records else "floats", "channels": n, "rounds_per_run": rounds, "ms_median": med,
                            "ms_min": min(ms), "ms_max": max(ms), "symbols_per_s": n * rounds / (med * 1e-3), "x_real_time": 1e3 / med,
                            "gb_per_s": (entry + 5) * n * rounds / (med * 1e-3) / 1e9}
                    out["lines"].append(line)
                    print(f"{name} {line['input']:7s} {n:7d} channels: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) per second of "
                          f"symbols = {line['symbols_per_s']:.3e} symbols/s, {line['gb_per_s']:.0f} GB/s, {1e3 / med:.0f}x real time", flush=True)
                    dec.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
