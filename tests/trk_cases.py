"""One case table for the three persistent closed-loop kernels (trk_fast_kernel, trk_lane_kernel, trk_persist_kernel)
and the host dispatch around them, shared by tests/test_trk_cases.py (CPU: the instantiation census and the plan
model) and tests/test_gpu_trk_coverage.py (the device against the oracle loop, bit for bit).

The dispatch is restated here from trk_abi.hip (trk_enqueue), trk_fast.hip (fast_thru, fast_packed_layout, fast_plan,
trk_fast_supported, launch_trk_fast), trk_lane.hip (trk_lane_supported, launch_trk_lane) and trk_persist.hip
(persist_lds, launch_trk_persist): plan() returns what gnsship_trk_last_plan reports for a configuration, and
instantiation() the template arguments that plan launches.

Instantiations (the census of test_trk_cases.py):
  trk_fast     3 formats × 5 layouts (3 taps float; 3 taps packed; 3 taps + data, packed; 5 taps; 5 taps + data)
               × whole-epoch slots / slot ring × latency / throughput form, less the throughput form of the two
               five-tap layouts = 48 (beside Galileo E1's 8184-float replica the throughput form's 72 KiB hold one
               product group and a plan needs two: fast_plan has no plan, launch_trk_fast no instantiation), and
               per format and layout the latency form's wave-role plan of long epochs (N ≥ 10000, a run-time
               branch) beside the short one
  trk_lane     3 formats × {3, 3 + data, 5, 5 + data} = 12
  trk_persist  3 formats × 9 layouts ({3, 3 + data, 5, 5 + data} × {generic, AVX}, GLONASS) × THRU = 54.  Every AVX
               layout runs chains_avx (u_avx's sixteen chains on sixteen lanes): the task-tree form that 3, 5 and
               5 + data used to run summed in another order than the reference and is no longer launched, so the
               3-tap chains_avx instantiation of the 10230-chip signals is the 3-tap AVX one (the B3I cases stay:
               same function, another replica length)

Signals, one per layout and rate, cached (signal()): GPS L1 C/A (3 taps, float replica), BeiDou B3I (3 taps, sign-bit
replica; float with GNSSHIP_TRK_FAST_PACKED=0 is the GPS layout again), GPS L5 (3 taps + data), Galileo E1 with
track_pilot = 0 (5 taps) and 1 (5 taps + data), GLONASS L1 C/A.  Every case runs 40 epochs.  The integer formats are
the same samples through signals.to_ishort / to_ibyte with the type's extreme values planted in the first three
epochs (planted()); the oracle reads the integers converted to float, as the device does.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from gnss_sim_receiver_amd import abi, signals

EPOCHS = 40
FMTS = ("cf32", "ci16", "ci8")
FMT_ID = {"cf32": abi.FMT_CF32, "ci16": abi.FMT_CI16, "ci8": abi.FMT_CI8}
SAMPLE_BYTES = {"cf32": 8, "ci16": 4, "ci8": 2}
CUS = 256                       # compute units of the MI355X: no case comes near it, so the forms are set by the knobs
KIB = 1024
PERSIST_MAX_LDS = 150 * KIB     # trk_engine.h kTrkPersistMaxLds
AVX_LANES, FAST_G = 16, 8
LONG_EPOCH = 10000              # trk_fast.hip kLongEpoch
SLOT_RING_GROUPS, MIN_RING_GROUPS, MAX_SLOT_BYTES = 16, 4, 48 * KIB
LANE_ROWS, LANE_WAVES = 4, 4    # trk_lane.hip kLRows, kLWaves
SIZEOF_TRK_CHANNEL = 928        # trk_engine.h TrkChannel (trk_lane.hip's write-back comment states it too)


# ---- the signal scenarios -------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Layout:
    """What the dispatch reads of TrkParams (build_params, trk_abi.hip)."""
    n_taps: int
    data: bool
    single_code_bits: bool = False
    glo: bool = False
    code_len: int = 1023       # floats of one replica in the code bank (E1: 2 per chip)


SCENARIOS = {
    # name: layout, the rates used (Msps → N = one code period)
    "gps": Layout(3, False, code_len=1023),
    "b3i": Layout(3, False, single_code_bits=True, code_len=10230),
    "l5": Layout(3, True, code_len=10230),
    "e1d": Layout(5, False, code_len=8184),    # Galileo E1, track_pilot = 0: the data component alone
    "e1": Layout(5, True, code_len=8184),
    "glo": Layout(3, False, glo=True, code_len=511),
}
PERIOD_S = {"gps": 1e-3, "b3i": 1e-3, "l5": 1e-3, "e1d": 4e-3, "e1": 4e-3, "glo": 1e-3}


def vector_length(scenario: str, fs: float) -> int:
    return int(round(fs * PERIOD_S[scenario]))


# ---- the dispatch, restated -----------------------------------------------------------------------------------
def padded_code_quads(n: int) -> int:
    return (n + 2 * 32 + 3) // 4


def code_cap_floats(max_code_len: int) -> int:
    """trk_enqueue: LDS floats per replica, from the longest code of the context's bank."""
    return padded_code_quads(max_code_len) * 4


def lane_code_words(cap: int) -> int:
    return (cap + 31) // 32


def fast_code_stride(packed: bool, cap: int) -> int:
    return (lane_code_words(cap) + 3) // 4 * 4 if packed else cap


def env_flag(env: dict, name: str):
    """None when unset, else whether the value starts with '1' (how every knob is read)."""
    v = env.get(name)
    return None if v is None else v[:1] == "1"


def fast_thru(n_chans: int, env: dict) -> bool:
    f = env_flag(env, "GNSSHIP_TRK_THRU")
    return n_chans > CUS if f is None else f


def fast_packed_layout(lay: Layout, binary: bool, env: dict) -> bool:
    if lay.n_taps == 3 and lay.data:
        return True
    if not lay.single_code_bits or not binary or lay.n_taps != 3 or lay.data:
        return False
    return env.get("GNSSHIP_TRK_FAST_PACKED", "1")[:1] != "0"


def fast_plan(lay: Layout, n: int, cap: int, n_chans: int, binary: bool, env: dict):
    """FastPlan of fast_plan(): dict(bytes, rs, rg, packed, S), or None when no plan fits."""
    packed = fast_packed_layout(lay, binary, env)
    if lay.n_taps == 5 and fast_thru(n_chans, env):
        return None     # five taps have no throughput form
    m = n // AVX_LANES
    s = max(1, (m + FAST_G - 1) // FAST_G)
    n_groups = (s + 3) // 4
    ntt = lay.n_taps + (1 if lay.data else 0)
    codes = (2 if lay.data else 1) * fast_code_stride(packed, cap) * 4
    slot_b = AVX_LANES * 8
    group_b = 2 * ntt * AVX_LANES * (4 * FAST_G + 4) * 4 + 8
    budget = 72 * KIB if fast_thru(n_chans, env) else PERSIST_MAX_LDS
    if "GNSSHIP_TRK_FAST_LDS" in env:
        budget = min(budget, int(env["GNSSHIP_TRK_FAST_LDS"]) * KIB)

    def fit(rs):
        used = codes + rs * slot_b
        if used >= budget:
            return 0
        rg = min((budget - used) // group_b, n_groups)
        return rg if rg >= min(2, n_groups) else 0

    rs, rg = s, (fit(s) if s * slot_b <= MAX_SLOT_BYTES else 0)
    if rg < min(n_groups, MIN_RING_GROUPS) and s > 4 * SLOT_RING_GROUPS:
        rg2 = min(fit(4 * SLOT_RING_GROUPS), SLOT_RING_GROUPS)
        if rg2 > rg:
            rs, rg = 4 * SLOT_RING_GROUPS, rg2
    if rg == 0:
        return None
    return dict(bytes=codes + rs * slot_b + rg * group_b, rs=rs, rg=rg, packed=packed, S=s)


def fast_supported(lay: Layout, n: int, cap: int, n_chans: int, binary: bool, env: dict) -> bool:
    if lay.n_taps not in (3, 5) or lay.glo:       # (GLONASS refuses the AVX rotator at create)
        return False
    if lay.n_taps == 3 and lay.data and not binary:
        return False
    if env.get("GNSSHIP_TRK_FAST", "")[:1] == "0":
        return False
    return fast_plan(lay, n, cap, n_chans, binary, env) is not None


def lane_supported(lay: Layout, cap: int, n_chans: int, fmt: str, buf_len: int, binary: bool, env: dict) -> bool:
    if lay.n_taps not in (3, 5) or lay.glo or not binary:
        return False
    if buf_len < 0 or buf_len * SAMPLE_BYTES[fmt] >= 1 << 31:
        return False
    chans = LANE_ROWS * LANE_WAVES
    lds = chans * (2 if lay.data else 1) * lane_code_words(cap) * 4
    if lds + chans * (SIZEOF_TRK_CHANNEL + (2 * 8 + 2) * 4) > 64 * KIB:
        return False
    f = env_flag(env, "GNSSHIP_TRK_LANE")
    return fast_thru(n_chans, env) if f is None else f


def serial_ring_bytes(rc: int, na: int) -> int:
    return rc * (64 * 2 * 4 + na * (64 + 4) * 4)


def persist_lds(lay: Layout, n: int, cap: int, avx: bool) -> int:
    codes = (2 if lay.data else 1) * cap * 4
    if not avx:
        na = 2 * (lay.n_taps + (1 if lay.data else 0))
        for rc in (16, 8, 4):
            b = codes + serial_ring_bytes(rc, na)
            if b <= PERSIST_MAX_LDS:
                break
        return b
    return codes     # chains_avx keeps its chains in registers: the replicas alone


PLAN_FIELDS = ("engine", "format", "n_taps", "data_prompt", "packed", "sring", "rs", "rg", "lds_bytes", "thru", "long_plan", "avx", "lane_waves")


def plan(lay: Layout, n: int, fmt: str, n_chans: int, max_code_len: int, buf_len: int, avx: bool, env: dict, binary: bool = True) -> dict:
    """gnsship_trk_plan of a run, as trk_enqueue and the launch function it picks fill it."""
    p = dict.fromkeys(PLAN_FIELDS, 0)
    p.update(format=FMT_ID[fmt], n_taps=lay.n_taps, data_prompt=int(lay.data))
    cap = code_cap_floats(max_code_len)
    assert persist_lds(lay, n, cap, avx) <= PERSIST_MAX_LDS, "the round-based loop: not a case of this table"
    no_fast = env.get("GNSSHIP_TRK_FAST", "")[:1] == "0"
    lanes = avx and not no_fast and lane_supported(lay, cap, n_chans, fmt, buf_len, binary, env)
    fast = avx and not lanes and fast_supported(lay, n, cap, n_chans, binary, env)
    if lanes:
        nw = max(1, min(LANE_WAVES, (n_chans + LANE_ROWS * CUS - 1) // (LANE_ROWS * CUS)))
        p.update(engine=abi.TRK_ENGINE_LANES, lane_waves=nw,
                 lds_bytes=nw * LANE_ROWS * (2 if lay.data else 1) * lane_code_words(cap) * 4)
    elif fast:
        f = fast_plan(lay, n, cap, n_chans, binary, env)
        thru = fast_thru(n_chans, env)
        p.update(engine=abi.TRK_ENGINE_FAST_THROUGHPUT if thru else abi.TRK_ENGINE_FAST_LATENCY, packed=int(f["packed"]),
                 sring=int(f["rs"] < f["S"]), rs=f["rs"], rg=f["rg"], lds_bytes=f["bytes"], thru=int(thru),
                 long_plan=int(not thru and n >= LONG_EPOCH))
    else:
        f = env_flag(env, "GNSSHIP_TRK_THRU")
        thru = n_chans > 256 if f is None else f
        p.update(engine=abi.TRK_ENGINE_PERSIST, lds_bytes=persist_lds(lay, n, cap, avx), thru=int(thru), avx=int(avx))
    return p


def instantiation(lay: Layout, p: dict) -> tuple:
    """The kernel instantiation a plan launches, as the census names it."""
    fmt = {v: k for k, v in FMT_ID.items()}[p["format"]]
    taps = f"{p['n_taps']}{'+data' if p['data_prompt'] else ''}"
    if p["engine"] == abi.TRK_ENGINE_LANES:
        return ("trk_lane", fmt, taps)
    if p["engine"] in (abi.TRK_ENGINE_FAST_LATENCY, abi.TRK_ENGINE_FAST_THROUGHPUT):
        return ("trk_fast", fmt, taps + (" packed" if p["packed"] else ""), "ring" if p["sring"] else "whole", "thru" if p["thru"] else "latency")
    assert p["engine"] == abi.TRK_ENGINE_PERSIST
    form = "glo" if lay.glo else "avx" if p["avx"] else "generic"
    return ("trk_persist", fmt, "glo" if lay.glo else taps, "" if lay.glo else form, "thru" if p["thru"] else "plain")


FAST_LAYOUTS = ("3", "3 packed", "3+data packed", "5", "5+data")
LANE_LAYOUTS = ("3", "3+data", "5", "5+data")
PERSIST_LAYOUTS = tuple((t, f) for t in LANE_LAYOUTS for f in ("generic", "avx")) + (("glo", ""),)


def all_instantiations() -> set:
    want = {("trk_fast", f, lay, ring, form) for f in FMTS for lay in FAST_LAYOUTS for ring in ("whole", "ring") for form in ("latency", "thru")
            if not (form == "thru" and lay.startswith("5"))}
    want |= {("trk_lane", f, lay) for f in FMTS for lay in LANE_LAYOUTS}
    want |= {("trk_persist", f, t, form, thru) for f in FMTS for t, form in PERSIST_LAYOUTS for thru in ("plain", "thru")}
    return want


def role_plan_axis() -> set:
    """Per format and trk_fast layout: the latency form with the short and with the long wave-role plan."""
    return {(f, lay, long) for f in FMTS for lay in FAST_LAYOUTS for long in (0, 1)}


# ---- the table -------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    scenario: str
    fs: float
    fmt: str
    n_chans: int
    avx: bool
    env: dict = field(default_factory=dict)
    want: tuple = None            # the instantiation the case is written for
    want_long: int = None         # trk_fast latency form: the wave-role plan it is written for

    @property
    def layout(self) -> Layout:
        return SCENARIOS[self.scenario]

    @property
    def n(self) -> int:
        return vector_length(self.scenario, self.fs)

    def buffer_samples(self) -> int:
        return signal_samples(self.scenario, self.fs)

    def plan(self) -> dict:
        return plan(self.layout, self.n, self.fmt, self.n_chans, self.layout.code_len, self.buffer_samples(), self.avx, self.env)


# Rates (Msps).  short: N < 10000, N mod 16 ≠ 0 where the scenario allows it, (N/16) mod 8 ≠ 0, ⌈N/128⌉ mod 4 ≠ 0
# (a serial tail, a partial task, a partial product group); long: N ≥ 10000; ring: the smallest rate of the scenario
# with S = ⌈⌊N/16⌋/8⌉ > 64, with the LDS budget that leaves the whole-epoch slots fewer than four product groups.
# The ring replaces the whole-epoch slots only where it leaves room for more product groups, and 64 slots against
# S = 65 save 128 bytes: the smallest epoch at which some whole-KiB budget gives the ring has S = 66 (3 taps) or
# 68 (3 taps + data) — found by ring_budget_kib over the rates in steps of 10 kHz.
#   gps  4.3 → N = 4300 (tail 12, M = 268, S = 34); 10.3 → 10300 (tail 12); 8.34 → 8340 (tail 4, S = 66)
#   b3i  8.184 → 8184 (tail 8, M = 511, S = 64); 12.5 → 12500 (tail 4, S = 98); ring at 8.34 → 8340
#   l5   as b3i, ring at 8.6 → 8600 (tail 8, S = 68)
#   e1   2.45 → 9800 (tail 8, M = 612, S = 77); 6.25 → 25000 (tail 8, M = 1562, S = 196)
RATES = {
    "gps": dict(short=4.3e6, long=10.3e6, ring=8.34e6),
    "b3i": dict(short=8.184e6, long=12.5e6, ring=8.34e6),
    "l5": dict(short=8.184e6, long=12.5e6, ring=8.6e6),
    "e1d": dict(short=2.45e6, long=6.25e6, ring=2.45e6),
    "e1": dict(short=2.45e6, long=6.25e6, ring=2.45e6),
    "glo": dict(short=4.3e6),
}
FAST_SCENARIO = {"3": "gps", "3 packed": "b3i", "3+data packed": "l5", "5": "e1d", "5+data": "e1"}
LANE_SCENARIO = {"3": "gps", "3+data": "l5", "5": "e1d", "5+data": "e1"}
THRU_CHANNELS = 9   # three waves' rows on trk_lane, the last wave with one row filled; nine workgroups elsewhere


def ring_budget_kib(lay: Layout, n: int, thru: bool) -> int:
    """The largest GNSSHIP_TRK_FAST_LDS (KiB) at which the plan is the slot ring: found on the restated plan."""
    cap = code_cap_floats(lay.code_len)
    env = {"GNSSHIP_TRK_THRU": "1" if thru else "0"}
    for kib in range(150, 0, -1):
        f = fast_plan(lay, n, cap, 1, True, dict(env, GNSSHIP_TRK_FAST_LDS=str(kib)))
        if f is not None and f["rs"] < f["S"]:
            return kib
    return 0


def _build():
    cases = []
    for fmt in FMTS:
        for lay_name, sc in FAST_SCENARIO.items():
            r = RATES[sc]
            lat = {"GNSSHIP_TRK_THRU": "0", "GNSSHIP_TRK_LANE": "0"}
            thr = {"GNSSHIP_TRK_THRU": "1", "GNSSHIP_TRK_LANE": "0"}
            cases.append(Case(f"fast-{sc}-short-{fmt}", sc, r["short"], fmt, 2, True, dict(lat), ("trk_fast", fmt, lay_name, "whole", "latency"), 0))
            cases.append(Case(f"fast-{sc}-long-{fmt}", sc, r["long"], fmt, 2, True, dict(lat), ("trk_fast", fmt, lay_name, "whole", "latency"), 1))
            n = vector_length(sc, r["ring"])
            kib = ring_budget_kib(SCENARIOS[sc], n, False)
            cases.append(Case(f"fast-{sc}-ring-{fmt}", sc, r["ring"], fmt, 2, True, dict(lat, GNSSHIP_TRK_FAST_LDS=str(kib)),
                              ("trk_fast", fmt, lay_name, "ring", "latency"), int(n >= LONG_EPOCH)))
            if SCENARIOS[sc].n_taps == 5:
                continue    # no throughput form
            cases.append(Case(f"fast-{sc}-thru-{fmt}", sc, r["short"], fmt, THRU_CHANNELS, True, dict(thr), ("trk_fast", fmt, lay_name, "whole", "thru")))
            kib = ring_budget_kib(SCENARIOS[sc], n, True)
            cases.append(Case(f"fast-{sc}-thru-ring-{fmt}", sc, r["ring"], fmt, THRU_CHANNELS, True, dict(thr, GNSSHIP_TRK_FAST_LDS=str(kib)),
                              ("trk_fast", fmt, lay_name, "ring", "thru")))
        for lay_name, sc in LANE_SCENARIO.items():
            cases.append(Case(f"lane-{sc}-{fmt}", sc, RATES[sc]["short"], fmt, THRU_CHANNELS, True, {"GNSSHIP_TRK_LANE": "1"}, ("trk_lane", fmt, lay_name)))
        for thru in ("plain", "thru"):
            env = {"GNSSHIP_TRK_THRU": "1" if thru == "thru" else "0"}
            nch = THRU_CHANNELS if thru == "thru" else 2
            for lay_name, sc in LANE_SCENARIO.items():
                cases.append(Case(f"persist-{sc}-generic-{thru}-{fmt}", sc, RATES[sc]["short"], fmt, nch, False, dict(env),
                                  ("trk_persist", fmt, lay_name, "generic", thru)))
                cases.append(Case(f"persist-{sc}-avx-{thru}-{fmt}", sc, RATES[sc]["short"], fmt, nch, True, dict(env, GNSSHIP_TRK_FAST="0"),
                                  ("trk_persist", fmt, lay_name, "avx", thru)))
            cases.append(Case(f"persist-b3i-chains-{thru}-{fmt}", "b3i", RATES["b3i"]["short"], fmt, nch, True, dict(env, GNSSHIP_TRK_FAST="0"),
                              ("trk_persist", fmt, "3", "avx", thru)))
            cases.append(Case(f"persist-glo-{thru}-{fmt}", "glo", RATES["glo"]["short"], fmt, nch, False, dict(env),
                              ("trk_persist", fmt, "glo", "", thru)))
    return cases


# ---- signals ---------------------------------------------------------------------------------------------------
def signal_samples(scenario: str, fs: float) -> int:
    """Samples of signal()'s buffer (trk_scenarios.sync's length; the 10230-chip modules' and GLONASS' own)."""
    n = vector_length(scenario, fs)
    if scenario in ("gps", "e1", "e1d"):
        return int(round(fs)) // 4 + n * (EPOCHS + 3)
    if scenario == "glo":
        return n * (EPOCHS + 3)
    return n * (2 + EPOCHS + 3)


@dataclass
class Signal:
    sat: object
    k: object               # the oracle's configuration (oracle_conf() sets the rotator variant); None for GLONASS
    x: np.ndarray           # complex64, x[0] = absolute sample `first`
    stamp: int
    first: int
    delay: float
    dop: float
    code: np.ndarray
    data_code: np.ndarray


@functools.lru_cache(maxsize=None)
def signal(scenario: str, fs: float) -> Signal:
    import b3i_l2c_scenarios as B
    import l5_scenarios as L5
    import trk_scenarios as S
    if scenario == "gps":
        sat, k, x, stamp, first, delay, dop = S.sync("GPS", fs, EPOCHS)
    elif scenario == "e1":
        sat, k, x, stamp, first, delay, dop = S.sync("GAL", fs, EPOCHS)
    elif scenario == "e1d":
        sat, k, x, stamp, first, delay, dop = S.sync("GAL", fs, EPOCHS, track_pilot=0)
    elif scenario == "b3i":
        sat, k, x, stamp, first, delay, dop = B.b3i_sync(fs, EPOCHS)
    elif scenario == "l5":
        sat, k, x, stamp, first, delay, dop = L5.sync(fs, EPOCHS)
    elif scenario == "glo":
        sat = signals.Satellite(prn=24, doppler_hz=1830.0, code_delay_chips=207.3, carrier_phase_rad=0.9, cn0_dbhz=50.0, system="GLO_L1",
                                bits="0100111010110001", symbols_per_bit=10)
        x = signals.generate_if(fs, signal_samples(scenario, fs), [sat], seed=102)
        k, stamp, first = None, 0, 0
        delay, dop = signals.acq_delay_samples(sat, fs, 0, 0) + 0.3, sat.doppler_hz + 25.0
    else:
        raise KeyError(scenario)
    assert len(x) == signal_samples(scenario, fs), (scenario, fs, len(x), signal_samples(scenario, fs))
    x = np.ascontiguousarray(x, np.complex64)
    x.setflags(write=False)
    if scenario == "e1d":     # the data component alone: the E1-B replica is the tracking code
        code, data = sat.code_data, None
    else:
        code, data = sat.code, (sat.code_data if SCENARIOS[scenario].data else None)
    return Signal(sat, k, x, stamp, first, delay, dop, code, data)


EXTREMES = {"ci16": (-32768, 32767), "ci8": (-128, 127)}


@functools.lru_cache(maxsize=None)
def planted(scenario: str, fs: float, fmt: str) -> np.ndarray:
    """The scenario's samples in one format.  Integer formats: quantised (signals.to_ishort / to_ibyte), then twelve
    samples overwritten with (min, max), (max, min), (min, min) and (max, max) of the type — the most negative value
    is the one a wrong sign extension, or a negation in the wrong width, turns into something else.  The positions are
    spread over the first three epochs of the run (planted_positions)."""
    s = signal(scenario, fs)
    if fmt == "cf32":
        return s.x
    raw = (signals.to_ishort(s.x) if fmt == "ci16" else signals.to_ibyte(s.x)).copy()
    lo, hi = EXTREMES[fmt]
    for pos, (re, im) in zip(planted_positions(scenario, fs), 3 * ((lo, hi), (hi, lo), (lo, lo), (hi, hi))):
        raw[2 * pos], raw[2 * pos + 1] = re, im
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def first_epoch_offset(scenario: str, fs: float) -> int:
    """Where channel 1's first epoch starts in x: start_tracking's alignment to the next code start, which depends on
    the start arguments alone (the other channels' hand-over errors move theirs by a sample at the most)."""
    from oracle import trk as T
    s = signal(scenario, fs)
    delay, dop = start_args(scenario, fs, 1)
    if scenario == "glo":
        import glonass_model as M
        m = M.GlonassTracking("1G", int(fs), s.sat.freq_channel, prn=s.sat.prn)
        m.start_tracking(delay, dop, s.stamp, s.first)
        return int(m.sample_counter) - s.first
    ref = T.track(oracle_conf(scenario, fs, True), s.x, s.code, delay, dop, s.stamp, s.first, 1, data_code=s.data_code, buffer_first=s.first)
    return int(ref["sample_counter"][0]) - s.first


def planted_positions(scenario: str, fs: float) -> list:
    """Twelve positions in x, four in each of the first three epochs (16 samples clear of their ends)."""
    n = vector_length(scenario, fs)
    start = first_epoch_offset(scenario, fs)
    return [start + 16 + (i * (3 * n - 64)) // 12 + 7 * i for i in range(12)]


def as_float(raw: np.ndarray) -> np.ndarray:
    """What the loop computes on: the integers converted without scaling."""
    return raw if raw.dtype == np.complex64 else raw.astype(np.float32).view(np.complex64)


# ---- channels and references -----------------------------------------------------------------------------------
IDLE_CHANNEL = {2: 0, THRU_CHANNELS: 5}     # per channel count: the channel that is never started


def started_channels(n_chans: int) -> list:
    return [ch for ch in range(n_chans) if ch != IDLE_CHANNEL[n_chans]]


def start_args(scenario: str, fs: float, ch: int) -> tuple:
    """(acq_delay_samples, acq_doppler_hz) of channel ch: every channel tracks the scenario's one satellite from its
    own hand-over error (up to 0.2 samples, 6 Hz), so the channels of a case run different loops."""
    s = signal(scenario, fs)
    return s.delay + 0.1 * (ch % 5 - 2), s.dop + 2.0 * (ch % 7 - 3)


def oracle_conf(scenario: str, fs: float, avx: bool):
    k = signal(scenario, fs).k
    k = type(k).from_buffer_copy(k)
    k.rotator_avx = 1 if avx else 0
    return k


@functools.lru_cache(maxsize=None)
def reference(scenario: str, fs: float, fmt: str, avx: bool, ch: int, epochs: int = EPOCHS) -> np.ndarray:
    """The oracle loop's records of channel ch (oracle/trk.py; GLONASS: tests/glonass_model.py), computed once."""
    from oracle import trk as T
    s = signal(scenario, fs)
    xf = as_float(planted(scenario, fs, fmt))
    delay, dop = start_args(scenario, fs, ch)
    if scenario == "glo":
        import glonass_model as M
        m = M.GlonassTracking("1G", int(fs), s.sat.freq_channel, prn=s.sat.prn)
        m.start_tracking(delay, dop, s.stamp, s.first)
        ref = m.run(xf, 0, epochs)
    else:
        ref = T.track(oracle_conf(scenario, fs, avx), xf, s.code, delay, dop, s.stamp, s.first, epochs, data_code=s.data_code,
                      buffer_first=s.first, prn=s.sat.prn)
    ref.setflags(write=False)
    return ref


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
CASE_IDS = [c.name for c in CASES]
