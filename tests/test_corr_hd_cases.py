"""The high-dynamics correlator's case table (tests/corr_hd_cases.py) on the CPU: what the GPU test's cases, reference
and bound are worth.

(a) Census: the table reaches the three hd_corr_kernel<FMT> instantiations, tap counts 1 to 8, jobs of 1, 2 and more
    than 2 chunks, the circular-shift wrap taken and not taken within one job, sample 0, renormalised samples
    (n0 % 256 == 0), k·k ≥ 2³², chip indices below 0 and below −L before the wrap, S_t == N, the code-length limit,
    and the four code lengths, the three standard forms and the integer extremes in every dense batch.
(b) The plain float32 model agrees with the oracle to 1e-6 on every impulse entry (measured: 9.4e-8 at the worst), and
    chip for chip with the oracle's resampler.
(c) Teeth: each mutation of the model leaves the 1e-5 bound by a factor of ten or more on some impulse entry of the
    sweep named for it.  One mutation cannot: the sample-0 phasor left unnormalised moves one sample by 4e-8, since
    |(cosf r, −sinf r)| is 1 to a few 2⁻²⁴ for every float r (test_sample0_normalisation_is_beneath_the_contract).
(d) The refusals of the table are exactly what the oracle refuses.
"""
import numpy as np
import pytest

import corr_hd_cases as H
from gnss_sim_receiver_amd import abi


def _hd(jobs):
    return jobs[jobs["flags"] == abi.JOB_HIGH_DYN]


def _raw_index(s, m):
    """floor of tap 0's float32 code phase at buffer positions m, before the wrap to [0, L)."""
    m = np.asarray(m, np.uint64)
    F = np.float32
    v = F(s.step) * m.astype(np.float32) + F(s.code_rate) * ((m * m) & np.uint64(0xFFFFFFFF)).astype(np.float32)
    return np.floor(((v + F(s.shifts[0])) - F(s.rem_code)).astype(np.float64)).astype(np.int64)


def test_census_formats_taps_chunks():
    assert {s.fmt for s in H.SWEEPS.values()} == set(H.FMTS) == {c.fmt for c in H.DENSE}
    for c in H.DENSE:
        hd = _hd(c.jobs)
        assert set(hd["n_taps"][hd["n_samples"] > 0]) == set(range(1, 9)), c.name
        assert set(hd["n_samples"]) == set(H.DENSE_LENGTHS), c.name
        assert list(hd["n_taps"][hd["n_samples"] == 0]) == [1, 1], c.name
        assert np.all(c.jobs["sample_offset"] % 2 == 1), c.name
        assert set(hd["code_id"]) == {0, 1, 2, 3} and max(H.DENSE_CODE_LENS) == H.MAX_CODE_LEN, c.name
        assert c.jobs[0]["flags"] == c.jobs[-1]["flags"] == abi.JOB_HIGH_DYN, c.name  # pins the out_index mapping
        assert set(c.jobs["flags"]) == {abi.JOB_HIGH_DYN, abi.JOB_ROTATOR_TREE, abi.JOB_ROTATOR_AVX, 0}, c.name
        assert 20 <= len(c.jobs) <= 48
        assert np.all(c.jobs["sample_offset"] + c.jobs["n_samples"] <= H.DENSE_N_BUF)
        chunks = {min(H.n_chunks(int(n)), 3) for n in hd["n_samples"]}
        assert chunks == {0, 1, 2, 3}, c.name
    by_chunks = {}
    for s in H.SWEEPS.values():
        for n, _ in s.entries:
            by_chunks.setdefault(min(H.n_chunks(n), 3), set()).add(s.name)
    assert by_chunks[1] >= {"S3-ci16", "S3-ci8", "S5"} and "S1" in by_chunks[2] and "S2" in by_chunks[2] and "S4" in by_chunks[3]
    assert H.n_chunks(H.S4_N) == 18 and H.SWEEPS["S4"].L == H.MAX_CODE_LEN
    assert {n for n, _ in H.SWEEPS["S5"].entries} == {1, 2, 3}


def test_census_sample_positions():
    for name in ("S1", "S2", "S3-ci16", "S3-ci8", "S5"):     # every n0 of every length
        s = H.SWEEPS[name]
        assert sorted(s.entries) == [(n, n0) for n in sorted({n for n, _ in s.entries}) for n0 in range(n)], name
    for name in ("S1", "S2", "S3-ci16", "S4"):
        n0 = np.array([e[1] for e in H.SWEEPS[name].entries])
        assert 0 in n0 and np.any((n0 > 0) & (n0 % H.RENORM == 0)), name
        assert np.any(n0 % H.RENORM == 1) and np.any(n0 % H.RENORM == H.RENORM - 1), name
    n0 = np.array(H.S4_N0, np.uint64)
    k = n0[n0 > 0] - np.uint64(1)
    assert np.any(k * k >= 2 ** 32) and np.any(k * k < 2 ** 32)       # the rotator's (n − 1)²
    assert 65536 in n0 and 65537 in n0 and 65535 in n0                # both sides of the wrap, for n and for n − 1
    assert np.any(n0 % H.CHUNK == 0) and np.any(n0 % H.CHUNK == 1) and np.any(n0 % H.CHUNK == H.CHUNK - 1)
    assert H.S4_N - 1 in n0


def test_census_wrap_branch_and_negative_indices():
    for name in ("S1", "S2", "S3-ci16", "S3-ci8", "S4"):
        s = H.SWEEPS[name]
        n = s.n_max
        S = s.S(n)
        n0 = np.array([e[1] for e in s.entries])
        taken = {t for t in range(1, s.n_taps) if np.any(n0 + S[t] >= n)}
        not_taken = {t for t in range(1, s.n_taps) if np.any(n0 + S[t] < n)}
        assert taken & not_taken, name           # within one job: every impulse job of a sweep is the same job
    s2 = H.SWEEPS["S2"]
    assert tuple(s2.S(H.N12)) == H.S2_SAMPLE_SHIFTS and H.S2_SAMPLE_SHIFTS[-1] == H.N12   # the identity S = N
    assert s2.step > 1.0
    raw = _raw_index(s2, np.arange(H.N12))
    assert np.all(raw < 0) and np.any(raw < -s2.L) and np.any(raw >= -s2.L)
    assert np.any(_raw_index(H.SWEEPS["S1"], np.arange(H.N12)) < 0) and np.any(_raw_index(H.SWEEPS["S1"], np.arange(H.N12)) >= 0)
    for c in H.DENSE:     # dense: a short job whose last taps sit at S_t == N, long ones with 0 < S_t < N
        hd = _hd(c.jobs)
        all_S = [(int(j["n_samples"]), H.sample_shifts(j["shifts_chips"][: j["n_taps"]], j["code_phase_step_chips"], int(j["n_samples"])))
                 for j in hd]
        assert all(S is not None for _, S in all_S)
        assert any(n > 0 and S[-1] == n and len(S) > 1 for n, S in all_S), c.name
        assert any(0 < S[-1] < n for n, S in all_S), c.name
        assert any(S[-1] > H.CHUNK for _, S in all_S), c.name


def test_s2_taps_are_rolls_of_tap_0():
    """With the oracle's resampler: tap t is tap 0 rolled by exactly S_t samples (and by nothing at S_t == N)."""
    s = H.SWEEPS["S2"]
    idx = H.oracle_chip_indices(s, H.N12)
    assert len(np.unique(idx[0])) > 4000     # a roll by one sample off would show
    for t, S in enumerate(H.S2_SAMPLE_SHIFTS):
        assert np.array_equal(idx[t], np.roll(idx[0], -S)), (t, S)
    assert np.array_equal(idx[-1], idx[0])


def test_integer_extremes():
    for fmt in ("ci16", "ci8"):
        lo, hi = H.EXTREMES[fmt]
        x = H.dense_samples(fmt).reshape(-1, 2)
        assert x.dtype == H.INT_DTYPE[fmt]
        seen = set()
        for j in H.DENSE_BY_NAME[f"len-{fmt}"].jobs:
            o = int(j["sample_offset"])
            for p in range(o, o + min(3, int(j["n_samples"]))):
                assert x[p, 0] in (lo, hi) and x[p, 1] in (lo, hi), (fmt, p)
                seen.add((int(x[p, 0]), int(x[p, 1])))
        assert {(lo, hi), (hi, lo), (lo, lo)} <= seen, fmt
        assert H.SWEEPS[f"S3-{fmt}"].v == (lo, hi)
        b = H.sweep_buffer(H.SWEEPS[f"S3-{fmt}"])
        assert b.dtype == H.INT_DTYPE[fmt] and np.count_nonzero(b) == 2 and (b[1200], b[1201]) == (lo, hi)


@pytest.mark.parametrize("name", H.SWEEP_IDS)
def test_sweep_reference_is_finite_and_never_zero(name):
    s, ref = H.SWEEPS[name], H.sweep_reference(name)
    assert np.all(np.isfinite(ref.view(np.float32)))
    assert np.all(np.abs(ref[:, : s.n_taps]) > 0) and np.all(ref[:, s.n_taps:] == 0)
    assert np.min(np.abs(H.ramp_code(s.L))) >= 1.0   # no zero chip
    # the reference's phasor modulus, |ref| / (|v|·|chip|): not 1, so |out| says nothing about the chip
    chip = np.array([H.ramp_code(s.L)[H.oracle_chip_indices(s, n)[0, n0]] for n, n0 in s.entries])
    mod = np.abs(ref[:, 0].astype(np.complex128)) / (abs(complex(*s.v)) * np.abs(chip))
    print(f"\ncorr-hd reference {name}: {len(s.entries)} jobs, phasor modulus {mod.min():.6f} to {mod.max():.6f}")


@pytest.mark.parametrize("name", H.SWEEP_IDS)
def test_model_agrees_with_the_oracle(name):
    s, ref = H.SWEEPS[name], H.sweep_reference(name)
    for n in sorted({n for n, _ in s.entries}):
        assert np.array_equal(H.model_chip_indices(s, n), H.oracle_chip_indices(s, n)), (name, n)
    out = H.model_impulse(s)
    e = H.impulse_errs(out, ref, s.n_taps)
    print(f"\ncorr-hd model {name}: worst |model − oracle|/|oracle| {e.max():.3e}")
    assert e.max() <= H.MODEL_TOL, H.describe_failures(s, out, ref, H.MODEL_TOL)


@pytest.mark.parametrize("mut", list(H.MUTATIONS))
def test_bound_has_teeth(mut):
    s = H.SWEEPS[H.MUTATIONS[mut]]
    e = H.impulse_errs(H.model_impulse(s, mut), H.sweep_reference(s.name), s.n_taps)
    frac = float(np.mean(e > H.TEETH))
    print(f"\ncorr-hd mutation {mut} on {s.name}: worst {e.max():.3e}, {100 * frac:.2f} % of entries beyond {H.TEETH:g}")
    assert e.max() > H.TEETH, mut
    if mut == "chip_late":   # step 0.25575: about a quarter of the samples start a new chip; the rest share their neighbour's
        assert 0.2 < frac < 0.3
    if mut == "wrap_gt":     # only m == N differs: one sample per shifted tap
        assert int(np.sum(e > H.TEETH)) == s.n_taps - 1


def test_sample0_normalisation_is_beneath_the_contract():
    """The mutation `p0_unnorm` (sample 0's phasor phase_offset left unnormalised) cannot reach 1e-4, nor the 1e-5
    contract itself, at any input: phase_offset = (cosf r, −sinf r) has modulus 1 to within a few 2⁻²⁴ for every
    float r, so dividing by it moves sample 0 by ~1e-7 at the most and no other sample at all.  Measured over the
    start phases below: 4.1e-8 at rem_carrier = 1.0 (|p0| ≠ 1 in float), exactly 0 where |p0| rounds to 1.  What the
    test holds: the mutation is confined to n0 = 0 and stays below 2⁻²²; the device's sample-0 branch is held to the
    oracle by the impulse sweeps' n0 = 0 entries like any other sample."""
    s = H.SWEEPS["S1"]
    worst = 0.0
    for rc in (0.4, 1.0, 2.2, 3.3, 5.0, 100.0):
        a, b = H.model_impulse(s, None, rem_carrier=rc), H.model_impulse(s, "p0_unnorm", rem_carrier=rc)
        e = H.impulse_errs(b, a, s.n_taps)
        n0 = np.array([x[1] for x in s.entries])
        assert np.all(e[n0 != 0] == 0)
        worst = max(worst, e.max())
    print(f"\ncorr-hd mutation p0_unnorm: worst {worst:.3e}")
    assert 0 < worst < 2.0 ** -22


@pytest.mark.parametrize("name", H.DENSE_IDS)
def test_dense_reference_headroom(name):
    """The reference's own float sums against the double accumulation the device is compared with: within the bound,
    so the double sum is no stricter a yardstick than the reference can meet itself."""
    c, r = H.DENSE_BY_NAME[name], H.dense_reference(name)
    assert np.all(np.isfinite(r.ref.view(np.float32)))
    f32 = H.O.corr_batch(H.as_float(H.dense_samples(c.fmt)), c.jobs, H.dense_codes())
    e = H.dense_errs(f32, r, c.jobs)
    print(f"\ncorr-hd dense headroom {name}: float sums vs double {e.max():.3e}")
    assert e.max() <= H.TOL
    for k, j in enumerate(c.jobs):
        assert np.all(r.ref[k, j["n_taps"]:] == 0)
        if j["n_samples"] == 0:
            assert np.all(r.ref[k] == 0)
        else:
            assert np.all(np.abs(r.ref[k, : j["n_taps"]]) > 0)


def test_reuse_batches_grow_and_shrink():
    """hd_plan_upload's three capacities: the second batch needs less of each than the first, the third more than any."""
    def needs(jobs):
        hd = _hd(jobs)
        return (len(hd), sum(H.n_chunks(int(n)) for n in hd["n_samples"]), sum((int(n) + H.RENORM - 1) // H.RENORM for n in hd["n_samples"]))
    (_, a), (_, b), (_, c), (_, d) = H.reuse_batches()
    assert all(y < x for x, y in zip(needs(a), needs(b))) and all(y > 0 for y in needs(b))
    assert all(z > x for x, z in zip(needs(a), needs(c)))
    assert needs(d) == (0, 0, 0) and len(d) > 0


@pytest.mark.parametrize("name", H.REFUSAL_IDS)
def test_refusals_are_the_oracles(name):
    job, refused = H.REFUSALS[name]
    j = job[0]
    x, code = H.refusal_samples(), H.ramp_code(H.REFUSAL_L)
    assert int(j["sample_offset"]) + int(j["n_samples"]) <= H.REFUSAL_N_BUF
    if refused:
        with pytest.raises(ValueError):
            H.oracle_single(j, x, code)
    else:
        assert np.all(np.isfinite(H.oracle_single(j, x, code).view(np.float32)))
    t = int(j["n_taps"])
    if 1 <= t <= H.MAX_TAPS:   # the restated derive_hd_job agrees
        assert (H.sample_shifts(j["shifts_chips"][:t], j["code_phase_step_chips"], int(j["n_samples"])) is None) == refused
    else:
        assert refused
