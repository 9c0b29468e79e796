"""The numpy model of the acquisition FFT (tests/acq_fft_model.py) on the CPU: it equals numpy.fft in complex128 at
every size the GPU coverage test runs, its chooser gives the layouts that test is written for, the inputs of that
test have a unique grid maximum, and — the check that the GPU test would fail on a subtly wrong kernel — one
constant of the model off by 2.5e-5 moves the float32 grid well beyond the GPU test's bound."""
import numpy as np
import pytest

import acq_fft_model as A

CASE_IDS = [c.id for c in A.CASES]


def test_case_table_is_complete():
    assert len(A.CASES) == 47 and len(set(CASE_IDS)) == 47
    assert sorted(c.id for c in A.CASES if c.planted) == ["1920-huge32", "300-huge5", "60", "600-big", "62500"]
    # every four-step and huge register-point count, every radix of the runtime plans
    assert {c.layout.P for c in A.CASES if c.layout.kind == "four_step"} == set(A.BIG_P)
    assert {c.layout.P for c in A.CASES if c.layout.kind == "huge"} == set(A.HUGE_P)
    # (the huge layout's runtime rows run fft_lds, the one-workgroup layout's passes: radix 2 is covered there)
    for kind, radices in (("lds", {2, 3, 4, 5, 8}), ("four_step", {2, 3, 4, 5, 8}), ("huge", {3, 4, 5, 8})):
        assert {r for c in A.CASES if c.layout.kind == kind and not c.layout.ct_rows for r in c.layout.radix} == radices, kind


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_model_equals_numpy_fft_in_complex128(case):
    lay = A.choose_layout(case.n, case.force, case.huge_p)
    assert lay == case.layout
    assert int(np.prod(lay.radix)) == lay.row_len and (lay.P or 1) * lay.row_len == case.n
    rng = np.random.default_rng(case.n)
    x = rng.standard_normal((2, case.n)) + 1j * rng.standard_normal((2, case.n))
    ref = np.fft.fft(x, axis=1)
    XT = A.transform(x, lay, -1, np.complex128)
    assert np.abs(A.natural_order(XT, lay) - ref).max() <= 1e-12 * np.abs(ref).max()
    back = A.transform(XT, lay, +1, np.complex128)  # unnormalised, natural order out of the transposed storage
    assert np.abs(back - case.n * x).max() <= 1e-12 * case.n * np.abs(x).max()


def test_chooser_limits():
    assert A.choose_layout(4000) == A.Layout("four_step", 16, 250, (5, 5, 5, 2), True)
    assert A.choose_layout(4000, 1) == A.Layout("four_step", 16, 250, (5, 5, 5, 2), True)
    assert A.choose_layout(4000, 2) == A.Layout("huge", 4, 1000, (8, 5, 5, 5), False)
    assert A.choose_layout(50000) == A.Layout("huge", 5, 10000, (8, 5, 5, 5, 5, 2), True)   # 10000-point rows before 12500
    assert A.choose_layout(100000) == A.Layout("huge", 10, 10000, (8, 5, 5, 5, 5, 2), True)
    assert A.choose_layout(16000, 1) == A.Layout("four_step", 16, 1000, (8, 5, 5, 5), True)
    assert A.choose_layout(4001) is None and A.choose_layout(40001) is None and A.choose_layout(600000) is None
    assert A.ct_plan(250) == (10, 5, 5) and A.ct_plan(1000) == (10, 10, 10)
    assert A.ct_plan(10000) == (10,) * 4 and A.ct_plan(12500) == (10, 10, 5, 5, 5)
    assert [p for p in A.BIG_P if not A.two_factor(p)] == [18, 27, 30]


# ---- inputs ------------------------------------------------------------------------------------------------

def _margin(g):
    flat = np.sort(g.ravel().astype(np.float64))
    return (flat[-1] - flat[-2]) / flat[-1]


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_inputs_have_a_unique_grid_maximum(built, case):
    """Noise-only and planted-peak inputs: the complex128 reference grid's maximum exceeds the runner-up by more
    than 1e-3 relative, so the float32 device grid orders them the same way."""
    assert _margin(A.reference(case.n).ref) > 1e-3
    if case.planted:
        for d in A.planted_delays(case, A.samples_per_chip(case.n)):
            r = A.reference(case.n, d)
            assert _margin(r.ref) > 1e-3, d
            assert np.argmax(r.ref) % case.n == d, d  # at the planted delay (in either bin: −250 Hz loses only 10 % amplitude)
            # about 20× the noise cells' mean at the 0 Hz bin (the mean of exponential cells is 1.44 × their median)
            assert 5.0 < r.ref[1, d] / (1.44 * np.median(r.ref[1])) < 50.0, d


# ---- sensitivity -------------------------------------------------------------------------------------------

def _rel_rms(g, ref):
    g, ref = g.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((g - ref) ** 2) / np.mean(ref ** 2)))


def _sens_cases():
    """(size, force, huge_p) per layout family: two small sizes whose runtime plans hold every radix between them,
    and the smallest size with compile-time rows (radix 10)."""
    out = []
    for n, force, hp in [(480, 0, 0), (30, 0, 0), (7680, 1, 0), (480, 1, 0), (4000, 0, 0), (1920, 2, 4), (120, 2, 4), (40000, 0, 0),
                         (270, 1, 0), (480, 2, 16)]:
        lay = A.choose_layout(n, force, hp)
        rows = A.ct_plan(lay.row_len) if lay.ct_rows else lay.radix
        ps = [A.Perturb("butterfly", radix=R, index=p, part="rows") for p, R in enumerate(rows)]
        if len(rows) > 1 and n < 10000:
            ps.append(A.Perturb("pass_tw", index=lay.row_len // (rows[0] * rows[1])))  # read by pass 1 at k = 1, r = 1
        if lay.P and n < 1000:  # one column of M: the smallest size of the family
            ps.append(A.Perturb("col_tw", index=1))
        if lay.P and n < 10000:
            cols = (A.first_radix(lay.P), lay.P // A.first_radix(lay.P)) if lay.kind == "four_step" and A.two_factor(lay.P) \
                else A._radices(lay.P, A.first_radix)
            ps += [A.Perturb("butterfly", radix=R, index=p, part="cols") for p, R in enumerate(cols)]
            if len(cols) > 1:
                ps.append(A.Perturb("reg_tw", index=1))
        out += [pytest.param(n, force, hp, p, id=f"{n}-{force}-{hp}-{p.kind}-{p.part}-r{p.radix}-i{p.index}") for p in ps]
    return out


def test_sensitivity_covers_every_kind_radix_and_family():
    seen = {}
    for prm in _sens_cases():
        n, force, hp, p = prm.values
        kind = A.choose_layout(n, force, hp).kind
        seen.setdefault(kind, set()).add((p.kind, p.part, p.radix))
    for kind in ("lds", "four_step", "huge"):
        assert {r for k, part, r in seen[kind] if k == "butterfly" and part == "rows"} >= {2, 3, 4, 5, 8}, kind
        assert ("pass_tw", "rows", 0) in seen[kind]
    for kind in ("four_step", "huge"):
        assert {(k, part) for k, part, r in seen[kind]} >= {("col_tw", "rows"), ("reg_tw", "rows"), ("butterfly", "cols")}, kind
        assert ("butterfly", "rows", 10) in seen[kind]


@pytest.mark.parametrize("n, force, hp, perturb", _sens_cases())
def test_one_wrong_constant_exceeds_the_gpu_bound(built, n, force, hp, perturb):
    """One constant off by 2.5e-5 (the error of a literal cut to four digits): the float32 model's grid error,
    RMS(grid − ref)/RMS(ref) on noise-only input, is then more than 4× the GPU test's bound, which is itself 4×
    the unperturbed float32 model's error."""
    lay = A.choose_layout(n, force, hp)
    r = A.reference(n)
    base = _rel_rms(A.grid(r.sig, r.code, r.wipe, lay, np.complex64), r.ref)
    assert 2e-8 < base < 1e-6, base  # a float32 pipeline
    err = _rel_rms(A.grid(r.sig, r.code, r.wipe, lay, np.complex64, perturb), r.ref)
    print(f"{lay} {perturb}: float32 baseline {base:.2e}, bound {4 * base:.2e}, perturbed {err:.2e} = {err / (4 * base):.1f} x bound")
    assert err > 4.0 * (4.0 * base)
