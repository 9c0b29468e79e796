"""bench.py's command line: a plain run measures the headline alone and honours --steps; --dump-outputs
writes the last timed step's epoch records, identical from run to run; --full is off by default."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
STEPS, WARMUP, SECONDS = 2, 1, 0.05  # 50 epochs per step and channel


def test_full_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")


def run_bench(out_dir):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--seconds", str(SECONDS),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_dumps_last_step_reproducibly(built, tmp_path):
    from gnss_sim_receiver_amd import abi
    a, b = run_bench(tmp_path / "a"), run_bench(tmp_path / "b")
    n_ch, epochs = 12, int(SECONDS * 1000)
    for res in (a, b):
        assert res["steps"] == STEPS and res["warmup"] == WARMUP
        assert res["epoch_records_emitted"] == STEPS * n_ch * epochs  # --steps sets the timed steps
        assert res["ms_per_step"] > 0 and res["unit"] == "Msamples/s" and res["higher_is_better"] is True
        assert abs(res["value"] - SECONDS * 4e6 / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.001 * res["value"] + 0.1
        # a plain run carries no auxiliary line and no CPU baseline
        assert not {"channel_sweep", "cpu_baseline", "acquisition_c3", "open_loop_correlator", "c1_receiver"} & set(res)
    names = sorted(f for f in os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in abi.TRK_EPOCH_DTYPE.names if n != "pad")
    total = 0
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        total += x.nbytes
        assert x.dtype == np.float64 and x.shape == (epochs, n_ch) and np.isfinite(x).all()
        assert np.array_equal(x, y), f
    assert total <= 64e6
    # the last timed step: its sample counters lie in the last `SECONDS` of the timed span
    sc = np.load(tmp_path / "a" / "sample_counter.npy")
    t_end = int((11.0 + 0.5 + (WARMUP + STEPS) * SECONDS) * 4e6)
    assert sc.min() >= t_end - int(SECONDS * 4e6) - 4000 and sc.max() <= t_end + 4000
    assert (np.load(tmp_path / "a" / "state.npy") == 4).all()
