"""The correlator case table (tests/corr_cases.py) on the CPU: what the GPU test's reference and bound are worth.

(a) Headroom: the reference's own float sums stay within a quarter of the 1e-5 bound of the double-accumulation
    oracle the device is compared with, for every job of every case — the reference's rounding does not use
    up the budget.
(b) Sensitivity: on a job whose prompt tap carries signal (|ref| > ‖x‖₂), the oracle with the start phase moved
    by 3e-5 rad, or with that tap moved by one chip, leaves the bound by a factor of 2 or more; every tap class
    and format (and rotator form) keeps at least one such case.
(c) Census: the 48 instantiations of corr_batch_kernel (3 formats × 4 tap classes × in margin or not × anchored
    generic or AVX) are each reached by a case, with chunk_class and in_margin recomputed here from
    derive_job's formulas; the item shapes the cases are written for follow from plan_chunks' rules, and the
    kernel's XCD item order is a permutation for every grid.

The figures are tabulated in DESIGN.md ("Batched correlator coverage")."""
import numpy as np
import pytest

import corr_cases as C
from gnss_sim_receiver_amd import abi
from oracle import oracle as O


@pytest.mark.parametrize("name", C.CASE_IDS)
def test_reference_headroom(name):
    c, r = C.BY_NAME[name], C.reference(name)
    e = C.job_errs(r.ref_f32, r.ref, r.norms, c.jobs)
    print(f"\ncorr-headroom {name}: float sums vs double {e.max():.3e}")
    assert e.max() <= C.TOL / 4, (name, e)
    for k, j in enumerate(c.jobs):
        assert np.all(r.ref[k, j["n_taps"]:] == 0)
        if j["n_samples"] == 0:
            assert np.all(r.ref[k] == 0)


def _perturbed(c, r, field_name, delta):
    """Per job: the error figure of the oracle with one argument moved, against the unmoved reference."""
    jobs = c.jobs.copy()
    if field_name == "shift":  # the strongest tap, one chip
        for k, j in enumerate(jobs):
            t = int(np.argmax(np.abs(r.ref[k, : j["n_taps"]])))
            jobs["shifts_chips"][k, t] += np.float32(delta)
    else:
        jobs[field_name] += np.float32(delta)
    out = O.corr_batch(C.samples_as_float(c.fmt), jobs, list(C.codes()), accum_f64=True)
    return C.job_errs(out, r.ref, r.norms, c.jobs)


def test_sensitivity_of_the_signal_cases():
    seen, worst = {}, {}
    for c in C.CASES:
        r = C.reference(c.name)
        if not r.signal.any():
            continue
        by_phase = _perturbed(c, r, "rem_carrier_phase_rad", 3e-5)
        by_chip = _perturbed(c, r, "shift", 1.0)
        for k in np.flatnonzero(r.signal):
            shows = max(by_phase[k], by_chip[k]) >= 2 * C.TOL
            if not shows:
                continue  # neither shows: not a signal case
            key = (C.kernel_taps(int(c.jobs[k]["n_taps"])), c.fmt, c.form)
            seen.setdefault(key, []).append(c.name)
            w = worst.setdefault(key, [np.inf, np.inf])
            w[0], w[1] = min(w[0], by_phase[k]), min(w[1], by_chip[k])
    for key in sorted(worst):
        print(f"\ncorr-sensitivity {key}: {len(seen[key])} signal jobs, least phase figure {worst[key][0]:.2e}, least chip figure {worst[key][1]:.2e}")
    missing = [(nt, fmt, form) for nt in C.KERNEL_TAPS for fmt in C.FMTS for form in C.FORMS if (nt, fmt, form) not in seen]
    assert not missing, missing


def test_census_all_48_instantiations():
    reached = {}
    for c in C.CASES:
        live = c.jobs[(c.jobs["n_samples"] > 0) & ((c.jobs["flags"] & C.ROTATOR_FLAGS) != 0)]
        got = set()
        for j in live:
            cls = C.chunk_class(j, C.CODE_LENS[j["code_id"]])
            avx, tc, m = cls >> 3, (cls >> 1) & 3, cls & 1
            assert avx == (c.form == "avx") == bool(j["flags"] & abi.JOB_ROTATOR_AVX)
            assert bool(j["flags"] & abi.JOB_ROTATOR_TREE) == (c.form == "tree")  # never the serial kernel
            got.add((C.KERNEL_TAPS[tc], bool(m), bool(avx)))
            if c.want_margin is not None:
                assert bool(m) == c.want_margin, (c.name, j)
        assert got == set(c.reaches), c.name  # what the table records
        for key in got:
            reached.setdefault((c.fmt,) + key, []).append(c.name)
    want = {(fmt, nt, m, avx) for fmt in C.FMTS for nt in C.KERNEL_TAPS for m in (False, True) for avx in (False, True)}
    assert len(want) == 48 and set(reached) == want, sorted(want - set(reached))
    for key in sorted(reached):
        print(f"\ncorr-census {key}: {len(reached[key])} cases, e.g. {reached[key][0]}")


def test_surplus_taps_are_part_of_the_margin_proof():
    """Tap counts 2, 4, 6, 7 run the next wider kernel with the surplus shifts zeroed: with the taps at 40 chips and
    rem_code 40 the job's own indices are in the margin and shift 0 is not, so the job takes the wrapping path."""
    for k in range(1, 9):
        j = C.BY_NAME[f"taps{k}-tree-cf32"].jobs[0]
        own = j.copy()
        own["shifts_chips"][k:] = own["shifts_chips"][0]  # the proof over the job's own taps alone
        own["n_taps"] = 8
        assert C.in_margin(own, C.L_MAIN)
        assert C.in_margin(j, C.L_MAIN) == (k in C.KERNEL_TAPS)


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.want_items])
def test_item_shapes(name):
    c = C.BY_NAME[name]
    cpi = int(c.env.get("GNSSHIP_CHUNKS_PER_ITEM", 4))
    plan = C.plan_items(c.jobs, cpi)
    assert len(plan) == 1  # one class
    (items,) = plan.values()
    assert tuple(len(it) for it in items) == c.want_items
    flat = [p for it in items for p in it]
    chunks = [(k, m) for k, j in enumerate(c.jobs) for m in range(max(1, (int(j["n_samples"]) + 4095) // 4096))]
    assert sorted(flat) == chunks  # every chunk once
    for it in items:
        assert len({int(c.jobs[k]["code_id"]) for k, _ in it}) == 1  # one replica per item


def test_single_job_plan_of_the_reference_class():
    """pair_by_code = false (gnsship_corr_run): 4097 samples are one item of 2 chunks, 16385 an item of 4 and one of 1."""
    for n, shape in ((4097, (2,)), (16385, (4, 1))):
        (items,) = C.plan_items(C.BY_NAME[f"len{n}-avx-cf32"].jobs, 4, pair_by_code=False).values()
        assert tuple(len(it) for it in items) == shape


def test_xcd_item_order_is_a_permutation():
    for n in range(1, 200):
        assert sorted(C.xcd_item_order(n)) == list(range(n)), n
    for n in (1, 7, 9, 17):  # the class sizes of the table
        c = C.BY_NAME[f"class-items{n}-tree-cf32"]
        assert len(C.plan_items(c.jobs)[C.chunk_class(c.jobs[0], C.L_MAIN)]) == n
