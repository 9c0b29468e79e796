#!/usr/bin/env python3
"""Throughput of the device GLONASS GNAV telemetry decoder (gnsship_gnav_run_symbols, gnsship_gnav_run_records): one second
of symbols — 1000 rounds, one symbol per 1 ms code period — of 12 channels (a receiver) and of 163 840 channels, as floats
(4 B an entry) and as tracking's epoch records (96 B an entry), in two cases:

  state 2   every channel carries the same noiseless built stream and is in state 2 (set there through
            gnsship_gnav_state_set from the model's state after 12 000 symbols): a decode every 2000 symbols, the half-bit
            sums and the stamp in between, no correlation.  The steady state of a tracked satellite.
  state 0   every channel is fed symbols that never form a time mark, with a full history: the 300-symbol correlation runs
            on every symbol.  The cost of a channel that has not found a mark.

The inputs are made on the device, and a run is one call over all channels with no host copy of the outputs, so real time
needs one run per second.  Timed with HIP events on the context stream: warm-up runs, then the median of the timed runs.
One line per case, input and channel count with the input and output bytes the call moves, and one JSON line at the end
with every figure.  DESIGN.md records the result of a run on an MI355X.

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

CHANNELS = (12, 163_840)
ROUNDS = 1000


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("gnav_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import gnav_model as M
    from gnss_sim_receiver_amd import abi, engine

    timed_runs = args.warmup + max(5, args.runs)
    rng = np.random.default_rng(1)
    strings = M.frame_strings(t_k_raw=1234, t_b_raw=20, n_t=800, n=3, n_4=7, tau_c=1000, tau_gps=-50, rng=rng, ids=tuple(1 + k % 5 for k in range(16)))
    x2 = M.stream(strings, lead=5)
    m = M.Decoder(0, 0)
    m.run(x2[:12000])
    assert m.stat == 2
    state2 = np.zeros(1, abi.GNAV_STATE_DTYPE)
    for k, v in m.state().items():
        state2[k][0] = v
    x2 = x2[12000:12000 + timed_runs * ROUNDS]
    x0 = np.where(np.arange(2000 + timed_runs * ROUNDS) % 7 < 3, 1.0, -1.0).astype(np.float32)  # period 7: never the mark
    assert len(x2) == timed_runs * ROUNDS

    out = {"lines": []}
    with engine.Context(0) as ctx:
        for case, x in (("state2", x2), ("state0", x0)):
            for n in args.channels:
                for records in (False, True):
                    dec = engine.glonass_l1_ca_telemetry(ctx, n, 2000 if case == "state0" else ROUNDS)
                    if case == "state2":
                        for c in range(n):
                            dec.set_state(c, state2[0])
                        todo = x
                    else:  # fill the history first, untimed
                        fill = torch.from_numpy(x[:2000]).cuda()[:, None].expand(2000, n).contiguous()
                        dec.run_symbols(fill.data_ptr(), on_device=True, n_rounds=2000, host=False)
                        ctx.sync()
                        del fill
                        todo = x[2000:]
                    if records:  # one round of records per sign, picked per round on the device
                        rows = np.zeros((2, n), abi.TRK_EPOCH_DTYPE)
                        rows["flags"] = 9
                        rows["prompt_i"][0], rows["prompt_i"][1] = -1.0, 1.0
                        rows_d = torch.from_numpy(rows.view(np.uint8).reshape(2, n, -1)).cuda()
                    ms = []
                    for k in range(0, len(todo), ROUNDS):
                        col = torch.from_numpy(np.ascontiguousarray(todo[k:k + ROUNDS])).cuda()
                        if records:
                            inp = rows_d[(col > 0).long()].contiguous()  # [rounds, n, 96]
                        else:
                            inp = col[:, None].expand(ROUNDS, n).contiguous()
                        torch.cuda.synchronize()
                        ctx.event_record(0)
                        if records:
                            dec.run_records(inp.data_ptr(), on_device=True, n_rounds=ROUNDS, host=False)
                        else:
                            dec.run_symbols(inp.data_ptr(), on_device=True, n_rounds=ROUNDS, host=False)
                        ctx.event_record(1)
                        ctx.sync()
                        del inp
                        if k >= args.warmup * ROUNDS:
                            ms.append(ctx.event_elapsed_ms(0, 1))
                    st = dec.state(n - 1)
                    want = (2, 12000 + len(todo)) if case == "state2" else (0, 2000 + len(todo))
                    assert (int(st["stat"]), int(st["symbol_counter"])) == want, st
                    assert case == "state0" or (st["tow_set"] == 1 and st["frame_sync"] == 1 and st["crc_error_counter"] == 0)
                    med = statistics.median(ms)
                    entry = abi.TRK_EPOCH_DTYPE.itemsize if records else 4
                    line = {"case": case, "input": "records" if records else "floats", "channels": n, "rounds_per_run": ROUNDS, "ms_median": med,
                            "ms_min": min(ms), "ms_max": max(ms), "symbols_per_s": n * ROUNDS / (med * 1e-3), "x_real_time": 1e3 / med,
                            "input_mb": entry * n * ROUNDS / 1e6, "output_mb": 5 * n * ROUNDS / 1e6, "gb_per_s": (entry + 5) * n * ROUNDS / (med * 1e-3) / 1e9}
                    out["lines"].append(line)
                    print(f"{case} {line['input']:7s} {n:7d} channels: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) per second of "
                          f"symbols = {line['symbols_per_s']:.3e} symbols/s, in {line['input_mb']:.1f} MB out {line['output_mb']:.1f} MB, "
                          f"{line['gb_per_s']:.0f} GB/s, {1e3 / med:.0f}x real time", flush=True)
                    dec.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
