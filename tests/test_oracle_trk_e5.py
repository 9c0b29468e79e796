"""The oracle loop on the Galileo E5a / E5b scenarios of tests/e5_scenarios.py: the conditions the device tests
(tests/test_gpu_trk_e5.py) rely on, asserted on the oracle alone so that a device test comparing against it
cannot hide a scenario that never synchronises.

Every scenario: state 4 by epoch 230, no loss-of-lock flag, at least 20 valid symbols; in pilot mode the
symbols (after the I/Q exchange) carry the data component on prompt_i.  The E5b scenarios run 260 epochs.  The
E5a ones run 530: with 20 code periods per symbol and the 100-entry sign buffer full at epoch 110 at the
earliest, 260 epochs can hold 7 symbols, and 20 need 510 (e5_scenarios.EPOCHS)."""
import numpy as np
import pytest

from oracle import trk as T

import e5_scenarios as E

CASES = [  # band, fs, pilot, prn, extra configuration
    ("a", 12.5e6, True, 11, {}), ("b", 12.5e6, True, 11, {}), ("a", 8.184e6, True, 36, {}), ("b", 8.184e6, True, 50, {}),
    ("a", 12.5e6, False, 11, {}), ("b", 12.5e6, False, 11, {}), ("a", 8.184e6, False, 36, {}),
    ("a", 12.5e6, True, 11, dict(extend_correlation_symbols=4)), ("b", 12.5e6, True, 11, dict(extend_correlation_symbols=4)),
    ("a", 12.5e6, False, 11, dict(extend_correlation_symbols=25)),
    ("a", 12.5e6, True, 11, dict(enable_fll_pull_in=1)), ("a", 12.5e6, True, 11, dict(rotator_avx=0)),
]


def case_id(c):
    return f"e5{c[0]}-{int(c[1] / 1e3)}k-{'pilot' if c[2] else 'data'}-prn{c[3]}" + "".join(f"-{k}={v}" for k, v in c[4].items())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_scenario_synchronises_and_stays_locked(case):
    band, fs, pilot, prn, kw = case
    kw = dict(kw)
    kw.setdefault("rotator_avx", 1)
    sat, k, x, stamp, first, delay, dop = E.sync(band, fs, prn=prn, pilot=pilot, **kw)
    epochs = E.EPOCHS[band]
    code, data = E.replicas(sat, pilot)
    raw = T.track(k, x, code, delay, dop, stamp, first, epochs, data_code=data, buffer_first=first)  # not exchanged
    ref = E.exchanged(raw, pilot)
    assert len(ref) == epochs
    assert not np.any(ref["flags"] & 2), "loss of lock"
    st = ref["state"]
    assert np.any(st[:230] == 4), "state 4 by epoch 230"
    valid = (ref["flags"] & 1) != 0
    assert np.count_nonzero(valid) >= 20
    if "extend_correlation_symbols" in kw:
        i_len = len(E.BAND[band][2])
        want = kw["extend_correlation_symbols"] if pilot else min(kw["extend_correlation_symbols"], i_len)
        assert k.extend_correlation_symbols == want and np.any(st == 3)
    # what exchanged() did: the valid symbols swapped in pilot mode, everything else untouched
    for f in ref.dtype.names:
        if f not in ("prompt_i", "prompt_q"):
            assert np.array_equal(ref[f], raw[f], equal_nan=ref[f].dtype.kind == "f"), f
    if pilot:
        assert np.array_equal(ref["prompt_i"][valid], raw["prompt_q"][valid]) and np.array_equal(ref["prompt_q"][valid], raw["prompt_i"][valid])
        assert np.array_equal(ref["prompt_i"][~valid], raw["prompt_i"][~valid])  # state 2's diagnostic prompt
        # with the pilot's phase tracked the data component lies on the quadrature arm of the data prompt: after the
        # exchange prompt_i carries the symbols (checked with the wide loops: the narrow 5 Hz carrier loop of extended
        # integration is still slewing the phase at the end of these runs)
        late = valid & (np.arange(len(ref)) > 230)
        assert "extend_correlation_symbols" in kw or np.all(np.abs(ref["prompt_i"][late]) > np.abs(ref["prompt_q"][late]))
    else:
        assert np.array_equal(ref["prompt_i"], raw["prompt_i"]) and np.array_equal(ref["prompt_q"], raw["prompt_q"])


def test_pilot_secondary_codes_differ_between_the_scenario_prns():
    assert len({E.BAND["a"][3](p) for p in (11, 36, 3, 29)}) == 4
    assert len({E.BAND["b"][3](p) for p in (11, 50, 3, 29)}) == 4


def test_first_epoch_is_code_period_990():
    """The timing the scenarios are built on: ten code periods of settling before the pattern's first chip."""
    for fs in (12.5e6, 8.184e6):
        sat = E.satellite("a")
        first = E.first_sample(fs)
        assert int(np.ceil(sat.chip_phase(np.float64(first), fs) / sat.code_len)) == 990
