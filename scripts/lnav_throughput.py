#!/usr/bin/env python3
"""Throughput of the device GPS L1 C/A telemetry decoder (gnsship_lnav_run_symbols, gnsship_lnav_run_records): 163 840
channels, one second of symbols each (50 rounds) resident on the device — what the headline channel count (README.md)
produces in one second, so real time needs one run per second.

Two states of the frame-sync machine:
  locked     every channel in state 1 on a noiseless built stream: an append per symbol, the TOW stamp of every entry, and
             one subframe (ten parities) per channel every sixth run;
  searching  every channel in state 0 on a full history of Gaussian noise: the preamble comparison after every symbol
             and a failed decode for about every 126 of them.
and both inputs: floats (4 B an entry) and tracking's epoch records (96 B an entry, of which the decoder needs 20).
A run is one call over all channels with the input on the device and no host copy of the outputs.  Timed with HIP events
on the context stream: warm-up runs, then the median of the timed runs.  The byte bound printed for run_records is what
the call must move — 96 B × channels × rounds read (whole records: the fields it needs lie in two different 32-byte
sectors of each), 5 B × channels × rounds of tow_ms / sflags written, 144 B of members per channel read and written —
over the HBM peak.  With --yardstick the Galileo I/NAV script (scripts/tlm_throughput.py) runs afterwards at the same
channel count, in its own process.  One JSON line at the end carries every figure.

Needs a GPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHANNELS = 163_840
ROUNDS = 50
HBM_PEAK = 8.0e12  # bytes per second, the MI355X specification; about 6.3e12 is what a copy kernel reaches


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=CHANNELS)
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick", action="store_true", help="run scripts/tlm_throughput.py at the same channel count afterwards")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("lnav_throughput: no GPU visible; this measurement has no CPU form", file=sys.stderr)
        return 2
    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import lnav_model as M
    from gnss_sim_receiver_amd import abi, engine

    n = args.channels
    timed_runs = args.warmup + max(5, args.runs)
    first = 300  # the seeded stream decodes its first subframe at counter 300: state 1 from there on
    total = first + timed_runs * ROUNDS
    x = M.build_stream(M.five_subframes(5)[0], total + 8, 0)[8:]  # what a tracker hands over: from the symbol after a preamble
    noise = np.random.default_rng(11).standard_normal(total).astype(np.float32)
    bytes_records = 96 * n * ROUNDS + 5 * n * ROUNDS + 2 * 144 * n
    bytes_symbols = 4 * n * ROUNDS + 5 * n * ROUNDS + 2 * 144 * n
    out = {"channels": n, "rounds_per_run": ROUNDS, "lines": [],
           "run_records_bytes": bytes_records, "run_records_bound_ms": 1e3 * bytes_records / HBM_PEAK,
           "run_symbols_bytes": bytes_symbols, "run_symbols_bound_ms": 1e3 * bytes_symbols / HBM_PEAK}
    with engine.Context(0) as ctx:
        sym_buf = engine.DeviceBuffer(ctx, 4 * ROUNDS * n)
        rec_buf = engine.DeviceBuffer(ctx, 96 * ROUNDS * n)
        rec = np.zeros((ROUNDS, n), abi.TRK_EPOCH_DTYPE)
        rec["flags"] = 9

        def upload(blk, records):
            if records:
                rec["prompt_i"] = blk[:, None]
                rec_buf.upload(rec.view(np.uint8).reshape(-1))
            else:
                sym_buf.upload(np.ascontiguousarray(np.repeat(blk[:, None], n, axis=1), np.float32))

        def launch(dec, records):
            if records:
                dec.run_records(rec_buf.ptr, on_device=True, n_rounds=ROUNDS, host=False)
            else:
                dec.run_symbols(sym_buf.ptr, on_device=True, n_rounds=ROUNDS, host=False)

        def timed(stream, label, records, check):
            dec = engine.gps_l1_ca_telemetry(ctx, n, ROUNDS)
            ms = []
            for k in range(0, total, ROUNDS):
                upload(stream[k:k + ROUNDS], records)
                ctx.event_record(0)
                launch(dec, records)
                ctx.event_record(1)
                ctx.sync()
                if k >= first + args.warmup * ROUNDS:
                    ms.append(ctx.event_elapsed_ms(0, 1))
            med, lo, hi = statistics.median(ms), min(ms), max(ms)
            st = dec.state(n - 1)
            check(st)
            bound = out["run_records_bound_ms" if records else "run_symbols_bound_ms"]
            name = "run_records" if records else "run_symbols"
            out["lines"].append({"state": label, "input": name, "ms_median": med, "ms_min": lo, "ms_max": hi, "x_real_time": 1e3 / med,
                                 "bound_ms": bound, "last_channel": st})
            print(f"{label:10s} {name:12s}: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) per second of symbols of {n} channels = "
                  f"{1e3 / med:.0f}x real time; byte bound {bound:.3f} ms; channel {n - 1}: stat {st['stat']}, tried {st['subframes_tried']}")
            dec.close()

        def locked(st):
            assert st["stat"] == 1 and st["frame_sync"] == 1 and st["crc_error_counter"] == 0 and st["tow_set"] == 1, st
            assert st["subframes_tried"] == (st["symbol_counter"] // 300), st

        def searching(st):
            assert st["stat"] == 0 and st["history_size"] == 300 and st["subframes_tried"] >= 1, st

        for records in (False, True):
            timed(x, "locked", records, locked)
            timed(noise, "searching", records, searching)
        sym_buf.free()
        rec_buf.free()
    print(json.dumps(out))
    if args.yardstick:
        sys.stdout.flush()
        return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "tlm_throughput.py"), "--channels", str(n), "--runs", str(args.runs),
                               "--warmup", str(args.warmup)]).returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
