"""tools/gnsship_rx without the conditioner options behaves as before the conditioner stage existed: on
the c1 scenario of tests/test_gpu_receiver.py (GPS PRN 7 and 3 at 4 Msps, 0.5 s, three channels, one in
acquisition) its events.csv and records.bin equal, byte for byte, the files the tool of the commit before
the stage wrote on an MI355X (tests/golden/receiver_parent_c1/, recorded with exactly this command; two
runs of that tool gave identical files)."""
import os
import subprocess

import pytest

from gnss_sim_receiver_amd import signals as S

import test_gpu_receiver as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "receiver_parent_c1")


def test_optionless_receiver_reproduces_the_parent_commit(tmp_path):
    sats = S.c1_sky(extra=((3, -2400.0, 3001.0),))
    x = S.generate_if(R.FS, int(0.5 * R.FS), sats, seed=0x6E550001)
    path = tmp_path / "c1.dat"
    x.tofile(path)
    ev, rec = str(tmp_path / "events.csv"), str(tmp_path / "records.bin")
    cmd = [R.RX, "--file", str(path), "--item", "gr_complex", "--fs", str(R.FS), "--channels", "3", "--in-acquisition", "1", "--rotator", "avx",
           "--block-ms", "100", "--acq-piece", "8192", "--events", ev, "--records", rec]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for got, name in ((ev, "events.csv"), (rec, "records.bin")):
        with open(got, "rb") as a, open(os.path.join(GOLD, name), "rb") as b:
            mine, gold = a.read(), b.read()
        assert len(gold) > 0 and mine == gold, (name, len(mine), len(gold))
