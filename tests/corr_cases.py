"""One case table for the batched correlator (corr_batch_kernel and the host plan around it), shared by
tests/test_corr_cases.py (CPU: reference headroom, sensitivity, instantiation census, plan model) and
tests/test_gpu_corr_coverage.py (the device against the oracle).

Inputs, all seeded: one 80 000-sample IF record at 16.368 Msps (exactly 1/16 chip of a 1.023 Mcps code per
sample) holding one planted signal — a seeded ±1 1023-chip code at amplitude 4 over unit-variance noise, zero
Doppler, carrier step −0.9 rad/sample — and seeded ±1 codes of 3, 1023 (the planted one), 2046, 4092, 10230,
16383 and 16384 chips.  The integer records are the same samples scaled by 256 (ci16) and 8 (ci8); the oracle
reads them converted without scaling, as the device does.

A job on the planted code is placed where the record's code phase matches its rem_code_phase_chips (to within
one sample, 1/16 chip), so its prompt tap carries signal whatever rem_code it is given: rem_code values whole
periods away (the out-of-margin cases) stay aligned.

The error figure of both test files, per job:  max over taps |out − ref| / max(|ref|, ‖x‖₂),  ref = the oracle
with double accumulation (accum_f64), ‖x‖₂ over the job's own samples; bound 1e-5 (BASELINE.json north star).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from gnss_sim_receiver_amd import abi, signals
from oracle import oracle as O

TOL = 1e-5
FS = 16.368e6
N_BUF = 80000
STEP = np.float32(1.023e6 / FS)          # 0.0625 chip per sample, exact
PHASE_STEP = np.float32(-0.9)            # the planted carrier, rad per sample (7.0 would be 0.18 from +0.9)
OFF_CARRIER = np.float32(0.9)            # jobs that are not meant to carry signal: 1.8 rad per sample off it
COHERENT_MAX = 4097                      # longest job placed on the planted carrier (see job())
AMPLITUDE = 4.0                          # of the planted signal, over complex noise of variance 2
DELAY = 17.0 / 32.0                      # chips: the record's code phase sits between the job grids
L_MAIN = 1023
CODE_LENS = (3, 1023, 2046, 4092, 10230, 16383, 16384)  # code id = position
MAIN, SECOND = 1, 2                      # the planted code; the other id of the two-code item cases
FORMS = {"tree": abi.JOB_ROTATOR_TREE, "avx": abi.JOB_ROTATOR_AVX}
ROTATOR_FLAGS = abi.JOB_ROTATOR_TREE | abi.JOB_ROTATOR_AVX  # jobs without either do not run corr_batch_kernel
FMTS = ("cf32", "ci16", "ci8")
MARGIN = 32                              # engine.h kCodeMargin
KERNEL_TAPS = (1, 3, 5, 8)               # the compiled tap classes
LENGTHS = (1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 511, 512, 1023, 1024, 1025, 1280, 4095, 4096, 4097, 8192, 8193,
           16384, 16385, 16400)
PHASE_STEPS = (0.0, 1e-4, -1e-4, 0.9, -0.9, 3.1, -3.1, 7.0)
REM_CARRIERS = (0.0, 3.0, -3.0, 100.0)
SHIFTS = {1: [0.0], 3: [-0.5, 0.0, 0.5], 5: [-1.0, -0.5, 0.0, 0.5, 1.0], 8: [-2.0, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0]}
TAP_OFFSETS = [0.0, -0.5, 0.5, -0.25, 0.25, -1.0, 1.0, -0.75]  # around 40 chips, first k of them


@functools.lru_cache(maxsize=None)
def codes():
    rng = np.random.default_rng(0xC0DE5)
    return tuple(np.where(rng.random(n) > 0.5, 1.0, -1.0).astype(np.float32) for n in CODE_LENS)


def _sat():
    return signals.Satellite(prn=1, doppler_hz=0.0, code_delay_chips=DELAY, carrier_phase_rad=0.7, system="GPS",
                             cn0_dbhz=10.0 * np.log10(AMPLITUDE ** 2 * FS / 2.0), f_if_hz=float(PHASE_STEP) * FS / (2.0 * np.pi),
                             code=codes()[MAIN])


@functools.lru_cache(maxsize=None)
def samples(fmt: str) -> np.ndarray:
    """The record in one format (complex64, or interleaved int16 / int8)."""
    if fmt == "cf32":
        return signals.generate_if(FS, N_BUF, [_sat()], seed=0x5EED)
    return signals.to_ishort(samples("cf32")) if fmt == "ci16" else signals.to_ibyte(samples("cf32"))


@functools.lru_cache(maxsize=None)
def samples_as_float(fmt: str) -> np.ndarray:
    """What the correlator computes on: the integers converted without scaling."""
    x = samples(fmt)
    return x if fmt == "cf32" else x.astype(np.float32).view(np.complex64)


def aligned_offset(rem_code: float, n: int, center: float = 0.0) -> int:
    """First sample s with s + n inside the record whose code phase ≡ center − rem_code (mod 1023) to within one
    sample: a tap at shift `center` of a job starting there with this rem_code is prompt."""
    want = (center - float(np.float32(rem_code)) + DELAY) % L_MAIN
    s = int(np.ceil(want / float(STEP)))
    assert s + n <= N_BUF, (rem_code, n)
    return s


def carrier_at(s: int) -> float:
    return float(np.mod(_sat().carrier_phase(np.float64(s), FS), 2.0 * np.pi))


def job(n, shifts, form, code=MAIN, rem_code=0.25, code_step=STEP, phase_step=None, rem_carr=None, offset=None,
        center=0.0):
    """One job; offset None: where the planted code is aligned with (rem_code, center); rem_carr None: the
    record's carrier phase at the offset.  phase_step None: the planted carrier for an aligned job of up to
    COHERENT_MAX samples, OFF_CARRIER otherwise.  Off the carrier the planted signal (amplitude 4, constant over
    the 16 samples of a chip) rotates by 1.8 rad per sample and sums to nothing, so a tap's partial sums are those
    of the noise alone: on the carrier they grow by up to 64 per chip on every misaligned tap, and linearly on an
    aligned one, and past 8192 samples the reference's own float sum of such a job is then 2.6e-6 or more from
    the double one — over the quarter of the bound that test_corr_cases.py grants it."""
    j = np.zeros(1, abi.JOB_DTYPE)[0]
    if phase_step is None:
        phase_step = PHASE_STEP if offset is None and n <= COHERENT_MAX else OFF_CARRIER
    if offset is None:
        offset = aligned_offset(rem_code, n, center)
    j["sample_offset"] = offset
    j["n_samples"] = n
    j["code_id"] = code
    j["n_taps"] = len(shifts)
    j["flags"] = FORMS.get(form, 0)  # "serial": no rotator flag, the reference-order kernel (corr_serial.hip)
    j["rem_carrier_phase_rad"] = carrier_at(offset) if rem_carr is None else rem_carr
    j["phase_step_rad"] = phase_step
    j["rem_code_phase_chips"] = rem_code
    j["code_phase_step_chips"] = code_step
    s = np.zeros(abi.MAX_TAPS, np.float32)
    s[: len(shifts)] = shifts
    j["shifts_chips"] = s
    return j


# ---- derive_job / plan_chunks / the kernel's item order, restated ---------------------------------------------
def kernel_taps(n_taps: int) -> int:
    """The tap class a job of n_taps runs in (engine.h chunk_class)."""
    return 1 if n_taps <= 1 else 3 if n_taps <= 3 else 5 if n_taps <= 5 else 8


def in_margin(j, code_len: int) -> bool:
    """derive_job's proof that every chip index the kernel forms lies in the padded replica — the kernel's
    surplus taps (shift 0 when n_taps is below its tap class) included."""
    t = int(j["n_taps"])
    sh = [float(v) for v in j["shifts_chips"][:t]] + ([0.0] if t < kernel_taps(t) else [])
    n = int(j["n_samples"])
    span = float(j["code_phase_step_chips"]) * float(n - 1 if n > 0 else 0)
    rem = float(j["rem_code_phase_chips"])
    lo = min(0.0, span) + min(sh) - rem - 2.0
    hi = max(0.0, span) + max(sh) - rem + 2.0
    return bool(np.isfinite(lo) and np.isfinite(hi) and lo >= -MARGIN and hi < code_len + MARGIN)


def chunk_class(j, code_len: int) -> int:
    tc = KERNEL_TAPS.index(kernel_taps(int(j["n_taps"])))
    return 8 * int(bool(j["flags"] & abi.JOB_ROTATOR_AVX)) + 2 * tc + int(in_margin(j, code_len))


def plan_items(jobs, chunks_per_item: int = 4, pair_by_code: bool = True) -> dict:
    """plan_chunks: class → its work items in launch order, each a tuple of (job, chunk) pairs."""
    out = {}
    for c in range(16):
        items, pending = [], {}
        for k, j in enumerate(jobs):
            if chunk_class(j, CODE_LENS[j["code_id"]]) != c:
                continue
            n = int(j["n_samples"])
            nch = 1 if n <= 0 else (n + 4095) // 4096
            if nch == 1 and pair_by_code and chunks_per_item > 1:
                p = pending.setdefault(int(j["code_id"]), [])
                p.append((k, 0))
                if len(p) == chunks_per_item:
                    items.append(tuple(p))
                    p.clear()
                continue
            for c0 in range(0, nch, chunks_per_item):
                items.append(tuple((k, m) for m in range(c0, min(c0 + chunks_per_item, nch))))
        for code_id in sorted(pending):
            if pending[code_id]:
                items.append(tuple(pending[code_id]))
        if items:
            out[c] = items
    return out


def xcd_item_order(n_items: int) -> list:
    """corr_batch_kernel: the item workgroup b of a grid of n_items takes (no prefetch workgroups)."""
    q, rmd = n_items >> 3, n_items & 7
    return [(b & 7) * q + min(b & 7, rmd) + (b >> 3) for b in range(n_items)]


# ---- the table -------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    group: str                      # len, taps, margin, carrier, items
    form: str
    fmt: str
    jobs: np.ndarray
    env: dict = field(default_factory=dict)   # read by set_jobs
    want_margin: bool = None        # the margin state every live job of the case is written for
    want_items: tuple = None        # chunks per item, per class in launch order, where the case is about that
    reaches: frozenset = None       # {(tap class, in margin, avx)} of its live jobs — × fmt = the instantiations

    def __post_init__(self):
        self.jobs = np.array(self.jobs, abi.JOB_DTYPE)
        self.reaches = frozenset((kernel_taps(int(j["n_taps"])), in_margin(j, CODE_LENS[j["code_id"]]), self.form == "avx")
                                 for j in self.jobs if j["n_samples"] > 0 and j["flags"] & ROTATOR_FLAGS)


def _build():
    cases = []

    def add(name, group, form, fmt, jobs, **kw):
        cases.append(Case(f"{name}-{form}-{fmt}", group, form, fmt, jobs, **kw))

    for form in FORMS:
        for fmt in FMTS:
            # lengths: one job, E-P-L, in margin up to 16400 samples (1025 chips from −0.25)
            for n in LENGTHS:
                add(f"len{n}", "len", form, fmt, [job(n, SHIFTS[3], form)], want_margin=True)
            # tap counts 1..8 around 40 chips with rem_code 40: the taps stay in the margin, shift 0 (the kernel's
            # surplus taps of counts 2, 4, 6, 7) is 40 chips below it
            for k in range(1, 9):
                sh = [40.0 + d for d in TAP_OFFSETS[:k]]
                add(f"taps{k}", "taps", form, fmt, [job(4097, sh, form, rem_code=40.0, center=40.0)], want_margin=k in KERNEL_TAPS)
            # margin: each tap class in and out (rem_code whole periods away), aligned with the planted code
            for nt, rem in zip(KERNEL_TAPS, (-1022.5, L_MAIN + 0.25, -3 * L_MAIN - 0.5, 5 * L_MAIN + 0.75)):
                add(f"mar-nt{nt}-in", "margin", form, fmt, [job(4097, SHIFTS[nt], form)], want_margin=True)
                add(f"mar-nt{nt}-out", "margin", form, fmt, [job(4097, SHIFTS[nt], form, rem_code=rem)], want_margin=False)
            add("mar-negstep-in", "margin", form, fmt, [job(4097, SHIFTS[3], form, rem_code=-300.25, code_step=-STEP, offset=1000)],
                want_margin=True)
            add("mar-negstep-out", "margin", form, fmt, [job(4097, SHIFTS[3], form, rem_code=0.25, code_step=-STEP, offset=1000)],
                want_margin=False)
            add("mar-L3-in", "margin", form, fmt, [job(300, SHIFTS[3], form, code=0, offset=777)], want_margin=True)
            add("mar-L3-out", "margin", form, fmt, [job(300, SHIFTS[3], form, code=0, rem_code=-40.5, offset=777)], want_margin=False)
            for code, nt in ((3, 3), (4, 5), (5, 3), (6, 5)):  # 4092, 10230, 16383, 16384 chips
                L = CODE_LENS[code]
                add(f"mar-L{L}-in", "margin", form, fmt, [job(4097, SHIFTS[nt], form, code=code, offset=2049)], want_margin=True)
                add(f"mar-L{L}-out", "margin", form, fmt, [job(4097, SHIFTS[nt], form, code=code, rem_code=-(L - 100.5), offset=2049)],
                    want_margin=False)  # runs over the code's end: indices L − 101 … L + 156
        fmt = "cf32"
        # carrier: every phase step at one and two chunks, the four start phases as four jobs
        for n in (4096, 4097):
            for i, ps in enumerate(PHASE_STEPS):
                add(f"car-N{n}-s{i}", "carrier", form, fmt, [job(n, SHIFTS[3], form, phase_step=ps, rem_carr=rc) for rc in REM_CARRIERS])
        # item shapes: k single-chunk jobs of 1000 samples (4 blocks, the last partial) on one code id, on two
        for k in range(1, 6):
            shape = ((4, 1) if k == 5 else (k,))
            add(f"items-k{k}", "items", form, fmt, [job(1000, SHIFTS[3], form, offset=3000 * i + 11) for i in range(k)], want_items=shape)
            both = [job(1000, SHIFTS[3], form, code=(MAIN, SECOND)[i & 1], offset=1500 * i + 7) for i in range(2 * k)]
            add(f"items2-k{k}", "items", form, fmt, both, want_items=((4, 4, 1, 1) if k == 5 else (k, k)))
        z = [job(1000, SHIFTS[3], form, offset=3000 * i + 11) for i in range(4)]
        z[1]["n_samples"] = 0
        add("items-zero-mid", "items", form, fmt, z, want_items=(4,))
        # a job without a rotator flag keeps an empty slot in the plan, with its own code: here the longest code beside
        # a live job on the shortest (the LDS replica is sized for the longest code of the launch, empty slots included)
        add("items-serial-slot", "items", form, fmt, [job(300, SHIFTS[3], form, code=0, offset=777),
                                                       job(1000, SHIFTS[5], "serial", code=6, offset=4000)])
        add("items-1-4096", "items", form, fmt, [job(1, SHIFTS[3], form, offset=501), job(4096, SHIFTS[3], form)], want_items=(2,))
        for n_items in (1, 7, 9, 17):  # one class of that many items: 4 jobs of 257 samples each, the last item 1
            nj = 4 * (n_items - 1) + 1
            add(f"class-items{n_items}", "items", form, fmt, [job(257, SHIFTS[3], form, offset=997 * i + 3) for i in range(nj)],
                want_items=(4,) * (n_items - 1) + (1,))
        for cpi, shape in ((1, (1, 1, 1, 1, 1)), (2, (2, 2, 1)), (3, (3, 2)), (4, (4, 1))):
            add(f"cpi{cpi}", "items", form, fmt, [job(16385, SHIFTS[3], form)], env={"GNSSHIP_CHUNKS_PER_ITEM": str(cpi)}, want_items=shape)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_IDS = [c.name for c in CASES]


# ---- references ------------------------------------------------------------------------------------------------
def job_norms(x: np.ndarray, jobs) -> np.ndarray:
    """‖x‖₂ over each job's own samples."""
    p = np.concatenate([[0.0], np.cumsum(np.abs(x.astype(np.complex128)) ** 2)])
    o, n = jobs["sample_offset"].astype(np.int64), jobs["n_samples"].astype(np.int64)
    return np.sqrt(p[o + n] - p[o])


def job_errs(out: np.ndarray, ref: np.ndarray, norms: np.ndarray, jobs) -> np.ndarray:
    """Per job: max over its taps of |out − ref| / max(|ref|, ‖x‖₂); 0 for an empty job."""
    e = np.zeros(len(jobs))
    for k, j in enumerate(jobs):
        t = int(j["n_taps"])
        if j["n_samples"] > 0:
            d = np.abs(out[k, :t].astype(np.complex128) - ref[k, :t].astype(np.complex128))
            e[k] = np.max(d / np.maximum(np.abs(ref[k, :t].astype(np.complex128)), norms[k]))
    return e


@dataclass
class Reference:
    ref: np.ndarray        # accum_f64 oracle, complex64[n_jobs, 8]
    ref_f32: np.ndarray    # the reference's own float sums
    norms: np.ndarray      # ‖x‖₂ per job
    signal: np.ndarray     # per job: some tap has |ref| > ‖x‖₂


@functools.lru_cache(maxsize=None)
def reference(name: str) -> Reference:
    c = BY_NAME[name]
    x = samples_as_float(c.fmt)
    ref = O.corr_batch(x, c.jobs, list(codes()), accum_f64=True)
    ref_f32 = O.corr_batch(x, c.jobs, list(codes()))
    norms = job_norms(x, c.jobs)
    sig = np.array([j["n_samples"] > 0 and np.max(np.abs(ref[k, : j["n_taps"]])) > norms[k] for k, j in enumerate(c.jobs)], bool)
    for a in (ref, ref_f32, norms, sig):
        a.setflags(write=False)
    return Reference(ref, ref_f32, norms, sig)
