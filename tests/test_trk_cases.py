"""The tracking-engine case table (tests/trk_cases.py) on the CPU: the dispatch restated, and what the table reaches.

(a) Census: every instantiation of trk_fast_kernel (48), trk_lane_kernel (12) and trk_persist_kernel (54) that the
    launch functions can pick is reached by a named case; so are both wave-role plans of trk_fast's latency form for
    every format and layout.  A failure names what is unreached.
(b) Each case's plan, recomputed from the restated dispatch, is the instantiation (and role plan) it was written
    for; no two cases are the same configuration.
(c) The shapes: the float 3-tap shape has a serial tail, a partial task and a partial product group; every slot-ring
    case's LDS budget is the largest whole KiB at which the plan is the ring (one more KiB and it is not); the
    throughput cases leave a wave's rows partly filled and one row idle.
(d) The references: every scenario's oracle loop runs all 40 epochs without losing lock in all three formats, and the
    planted extreme values (all four sign pairs) lie inside the first three epochs of every channel.
(e) Five taps have no trk_fast throughput plan whatever the budget — the forms taken out of launch_trk_fast.

The census table is in DESIGN.md ("Tracking engine coverage")."""
import numpy as np
import pytest

import trk_cases as C
from gnss_sim_receiver_amd import abi


def test_census_every_instantiation_is_reached():
    reached = {}
    for c in C.CASES:
        reached.setdefault(C.instantiation(c.layout, c.plan()), []).append(c.name)
    want = C.all_instantiations()
    assert len(want) == 48 + 12 + 54
    missing = sorted(want - set(reached))
    assert not missing, f"instantiations no case reaches: {missing}"
    assert set(reached) <= want, sorted(set(reached) - want)
    for key in sorted(reached):
        print(f"\ntrk-census {key}: {', '.join(reached[key])}")


def test_census_both_role_plans_of_the_latency_form():
    seen = set()
    for c in C.CASES:
        p = c.plan()
        if p["engine"] == abi.TRK_ENGINE_FAST_LATENCY:
            seen.add((c.fmt, C.instantiation(c.layout, p)[2], p["long_plan"]))
            assert p["long_plan"] == int(c.n >= C.LONG_EPOCH)
    missing = sorted(C.role_plan_axis() - seen)
    assert not missing, f"(format, layout, long role plan) no latency-form case reaches: {missing}"


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_case_plan_is_the_one_it_was_written_for(name):
    c = C.BY_NAME[name]
    p = c.plan()
    assert C.instantiation(c.layout, p) == c.want, (name, p)
    if c.want_long is not None:
        assert p["long_plan"] == c.want_long, (name, p)
    assert p["format"] == C.FMT_ID[c.fmt] and p["n_taps"] == c.layout.n_taps and p["data_prompt"] == int(c.layout.data)
    assert 0 < p["lds_bytes"] <= C.PERSIST_MAX_LDS
    if p["engine"] in (abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_FAST_THROUGHPUT):
        s = max(1, (c.n // 16 + 7) // 8)
        assert p["sring"] == int(p["rs"] < s) and p["rs"] == (64 if p["sring"] else s) and 2 <= p["rg"] <= (s + 3) // 4
        if p["thru"]:
            assert p["lds_bytes"] <= 72 * C.KIB
    if p["engine"] == abi.TRK_ENGINE_LANES:
        assert p["lane_waves"] == 1  # nine channels on 256 compute units: one wave (four rows) per workgroup


def test_no_case_is_a_duplicate():
    seen = {}
    for c in C.CASES:
        key = (c.scenario, c.fs, c.fmt, c.n_chans, c.avx, tuple(sorted(c.env.items())))
        assert key not in seen, (c.name, seen[key])
        seen[key] = c.name
    assert len(C.BY_NAME) == len(C.CASES)


def test_float_three_tap_shape_has_a_tail_a_partial_task_and_a_partial_group():
    n = C.vector_length("gps", C.RATES["gps"]["short"])
    assert n == 4300 and n % 16 == 12 and (n // 16) % 8 != 0 and -(-n // 128) % 4 != 0
    assert max(1, (n // 16 + 7) // 8) == 34
    for sc, r in C.RATES.items():  # every latency shape but the GLONASS one (generic rotator) and the ring's has a tail
        for which in ("short", "long"):
            if which in r:
                assert C.vector_length(sc, r[which]) % 16 != 0, (sc, which)
        assert C.vector_length(sc, r["short"]) < C.LONG_EPOCH <= C.vector_length(sc, r.get("long", 1e9))


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.want[0] == "trk_fast" and c.want[3] == "ring"])
def test_slot_ring_budget_is_the_largest_that_gives_the_ring(name):
    c = C.BY_NAME[name]
    kib = int(c.env["GNSSHIP_TRK_FAST_LDS"])
    cap = C.code_cap_floats(c.layout.code_len)
    f = C.fast_plan(c.layout, c.n, cap, c.n_chans, True, c.env)
    assert f["rs"] == 64 < f["S"] and f["bytes"] <= kib * C.KIB
    more = C.fast_plan(c.layout, c.n, cap, c.n_chans, True, dict(c.env, GNSSHIP_TRK_FAST_LDS=str(kib + 1)))
    assert more is not None and more["rs"] == more["S"]  # the whole epoch's slots again
    if C.PERIOD_S[c.scenario] == 1e-3:  # the smallest rate (in steps of 10 kHz) at which any whole-KiB budget gives the ring
        for n in range(c.n - 10, 8192, -10):
            assert C.ring_budget_kib(c.layout, n, c.want[4] == "thru") == 0, (name, n)


def test_throughput_cases_fill_a_wave_partly():
    for c in C.CASES:
        p = c.plan()
        if p["thru"] or p["engine"] == abi.TRK_ENGINE_LANES:
            assert c.n_chans == C.THRU_CHANNELS <= 9 and C.THRU_CHANNELS % C.LANE_ROWS != 0
            assert C.IDLE_CHANNEL[c.n_chans] in range(c.n_chans) and len(C.started_channels(c.n_chans)) == c.n_chans - 1
        else:
            assert c.n_chans == 2


def test_five_taps_have_no_throughput_plan():
    """What was taken out of launch_trk_fast.  A plan needs two product groups once the epoch has two (S ≥ 5 tasks,
    N ≥ 528) beside the replicas and at least min(S, 64) ≥ 5 phasor slots; the throughput form's budget is 72 KiB
    at the most: with the 8184-float E1 replica that never fits, with one replica or two."""
    for sc in ("e1d", "e1"):
        lay = C.SCENARIOS[sc]
        ntt = lay.n_taps + int(lay.data)
        group_b = 2 * ntt * 16 * (4 * C.FAST_G + 4) * 4 + 8
        codes = (2 if lay.data else 1) * C.code_cap_floats(lay.code_len) * 4
        assert 72 * C.KIB - codes - 5 * 128 < 2 * group_b
        for n in (528, 9800, 25000, 100000):
            assert C.fast_plan(lay, n, C.code_cap_floats(lay.code_len), 9, True, {"GNSSHIP_TRK_THRU": "1"}) is None
            assert C.fast_plan(lay, n, C.code_cap_floats(lay.code_len), 9, True, {"GNSSHIP_TRK_THRU": "0"}) is not None


SIGNALS = sorted({(c.scenario, c.fs) for c in C.CASES})


@pytest.mark.parametrize("scenario,fs", SIGNALS)
def test_references_hold_lock_and_see_the_planted_values(built, scenario, fs):
    s = C.signal(scenario, fs)
    n = C.vector_length(scenario, fs)
    avx = scenario != "glo"
    for fmt in C.FMTS:
        ref = C.reference(scenario, fs, fmt, avx, 1)
        assert len(ref) == C.EPOCHS and not np.any(ref["flags"] & 2) and np.all(ref["state"] >= 2), (fmt, np.bincount(ref["state"]))
        assert abs(int(ref["sample_counter"][0]) - s.first - C.first_epoch_offset(scenario, fs)) <= 1
    pos = np.array(C.planted_positions(scenario, fs))
    for fmt in ("ci16", "ci8"):
        raw = C.planted(scenario, fs, fmt)
        lo, hi = C.EXTREMES[fmt]
        got = raw.reshape(-1, 2)[pos]
        assert {tuple(v) for v in got.tolist()} == {(lo, hi), (hi, lo), (lo, lo), (hi, hi)}
        for ch in (1, 8):  # inside the first three epochs of the earliest- and latest-starting channels
            ref = C.reference(scenario, fs, fmt, avx, ch)
            start = int(ref["sample_counter"][0]) - s.first
            assert np.all((pos >= start) & (pos < start + 3 * n - 8))
    assert C.planted(scenario, fs, "cf32") is s.x
