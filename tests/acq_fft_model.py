"""A numpy model of the acquisition engine's hand-written FFT (csrc/acq_kernel.hip, csrc/acq_abi.hip),
written from the kernels' code and comments — never a call to numpy.fft.

What it mirrors, pass by pass (each pass vectorised over its butterflies and over a batch of rows):

* make_fft_plan / choose_acq_layout: the radices {8, 5, 4, 3, 2} largest first, the 4000 = 16 × 250
  special case, the four-step P ∈ BIG_P with M ≤ 1024, the huge layout's preference for 10000- and
  12500-point rows, the GNSSHIP_ACQ_FORCE_BIG / _FORCE_HUGE / _HUGE_P knobs (arguments here).
* the Stockham autosort pass (stockham_pass, wave_pass, fft_lds_ct*, wave_fft_row_ct): butterfly j reads
  buf[j + r·n/R], twiddled by W^{k·r·tstep} (k = j mod Ns), and writes buf[(j/Ns)·Ns·R + k + r·Ns];
  dft_small<R> with the kernels' operation order for R ∈ {2, 3, 4, 5, 8, 10}.
* for N = P·M (the block comment "Large transforms" of acq_kernel.hip): thread t owns column t,
  x[t + M·q]; forward = register P-point DFT, twiddle W_N^{t·kq}, M-point rows, stored TRANSPOSED
  XT[kq·M + k] = X[kq + P·k]; inverse = rows, conjugate twiddle, register DFT, natural order out.
* where each twiddle comes from: the N-entry table rounded once from double (gnsship_acq_create); the
  four-step row table tw[m·P]; the huge layout's own M-entry row table; the compile-time rows' pass
  twiddles as powers of one table read by a balanced product tree (and, in the huge layout, the quarter
  table's symmetry where the tree does not apply); the column twiddles as a product tree of tw[t]; the
  register DFT's literal twiddles, with the two-factor in-place form for the four-step P that have one.

What it does not reproduce: FMA contraction inside complex products and butterflies, and the order of the
reductions.  In complex128 the model is an exact-arithmetic check of the index algebra (against numpy.fft to
1e-12 in the tests); in complex64 its error against a complex128 reference is the float32 baseline that the
GPU test's bound is derived from.

`Perturb` changes ONE constant of the model, to show on the CPU that the GPU test's bound would catch a
kernel with that constant subtly wrong.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

MAX_N = 16384            # kMaxAcqN: the LDS-resident transform
MAX_PASSES = 16          # kMaxPasses
MAX_BIG_N = 32768        # kMaxAcqBigN
MAX_BIG_M = 1024         # kAcqThreads: four-step rows
MAX_HUGE_N = 32 * MAX_N  # kMaxAcqHugeN
BIG_P = (16, 18, 20, 24, 25, 27, 30, 32)   # GNSSHIP_BIG_P_LIST
HUGE_P = (4, 5, 8, 10, 16, 20, 25, 32)     # GNSSHIP_HUGE_P_LIST
BIG_CT_ROWS = (250, 1000)                  # acq_fft_big_rows_kernel<MC>
BIG_CT_SEARCH = ((16, 250), (25, 1000))    # acq_search_big_kernel<P, MC>: the inverse rows
HUGE_CT_ROWS = (10000, 12500)              # huge_ct_rows


class Layout(NamedTuple):
    """Field for field engine.AcqLayout (so the two compare equal)."""
    kind: str
    P: int
    row_len: int
    radix: tuple
    ct_rows: bool


class Perturb(NamedTuple):
    """One constant off by `eps` (added to the constant; to its real part for a complex one).

    kind "butterfly": the constant of dft_small<radix> — R = 3: sin 60°, R = 5 (and the 5-point halves of
                      R = 10): cos 72°, R = 8: √½, R = 2 and 4 (which have no literal): the unit weight of
                      the subtracted input / of the ±j rotation — in pass `index` of the row transform
                      (part "rows") or of the register DFT (part "cols");
         "pass_tw":   entry `index` of the row transform's twiddle table;
         "col_tw":    entry `index` of the column twiddles W_N^t (four-step / huge);
         "reg_tw":    the k·r = 1 literal twiddle of register-DFT pass `index` (the n2·k1 = 1 twiddle of the
                      two-factor in-place form).
    The same constant serves the forward, the code and the inverse transform, as it would in the kernels."""
    kind: str
    radix: int = 0
    index: int = 0
    part: str = "rows"
    eps: float = 2.5e-5


def make_plan(n):
    """make_fft_plan: radices, or None."""
    if n < 2 or n > MAX_N:
        return None
    rad, m = [], n
    for r in (8, 5, 4, 3, 2):
        while m % r == 0:
            if len(rad) >= MAX_PASSES:
                return None
            rad.append(r)
            m //= r
    return tuple(rad) if m == 1 else None


def choose_layout(n, force=0, huge_p=0):
    """choose_acq_layout: force 1 = GNSSHIP_ACQ_FORCE_BIG, 2 = GNSSHIP_ACQ_FORCE_HUGE; huge_p =
    GNSSHIP_ACQ_HUGE_P.  None where gnsship_acq_create rejects the size."""
    if force == 0 and n == 4000:
        return Layout("four_step", 16, 250, make_plan(250), True)
    if force == 0 and make_plan(n):
        return Layout("lds", 0, n, make_plan(n), False)
    if force != 2 and 2 <= n <= MAX_BIG_N:
        for p in BIG_P:
            if n % p:
                continue
            m = n // p
            if m > MAX_BIG_M or m < 2:
                continue
            if make_plan(m):
                return Layout("four_step", p, m, make_plan(m), m in BIG_CT_ROWS)
    if n < 8 or n > MAX_HUGE_N:
        return None
    for mc in HUGE_CT_ROWS:
        p = n // mc
        if n % mc or p not in HUGE_P or (huge_p and p != huge_p):
            continue
        return Layout("huge", p, mc, make_plan(mc), True)
    for p in HUGE_P:
        if (huge_p and p != huge_p) or n % p:
            continue
        if make_plan(n // p):
            return Layout("huge", p, n // p, make_plan(n // p), (n // p) in HUGE_CT_ROWS)
    return None


def first_radix(m):
    return 8 if m % 8 == 0 else 5 if m % 5 == 0 else 4 if m % 4 == 0 else 3 if m % 3 == 0 else 2


def ct_radix(m):
    return 10 if m % 10 == 0 else 5 if m % 5 == 0 else 3 if m % 3 == 0 else 8 if m % 8 == 0 else 4 if m % 4 == 0 else 2


def _radices(m, pick):
    rad = []
    while m > 1:
        rad.append(pick(m))
        m //= rad[-1]
    return tuple(rad)


def ct_plan(m):
    """Pass radices of the compile-time rows (ct_radix order)."""
    return _radices(m, ct_radix)


def two_factor(p):
    r1 = first_radix(p)
    return p // r1 in (2, 3, 4, 5, 8)


def twiddle_table(n, dtype):
    """exp(−2πi t/n), t < n, rounded once from double (gnsship_acq_create)."""
    ang = -2.0 * math.pi * np.arange(n, dtype=np.float64) / float(n)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(dtype)


def _mulj(z, sign):
    """z · (sign·j), exactly."""
    out = np.empty_like(z)
    if sign > 0:
        out.real, out.imag = -z.imag, z.real
    else:
        out.real, out.imag = z.imag, -z.real
    return out


def dft_small(v, R, sign, rt, eps=0.0):
    """dft_small<R, SIGN> on a list of R arrays, in the kernels' operation order; rt = the real dtype."""
    if R == 2:
        a, b = v
        return [a + b, a - (rt(1.0 + eps) * b if eps else b)]
    if R == 3:
        c1, s1 = rt(-0.5), rt(math.sqrt(3.0) / 2.0 + eps)
        a, b, c = v
        t, d = b + c, b - c
        m = a + c1 * t
        jd = _mulj(s1 * d, sign)
        return [a + t, m + jd, m - jd]
    if R == 4:
        a, b, c, d = v
        s0, d0, s1, d1 = a + c, a - c, b + d, b - d
        jd1 = _mulj(rt(1.0 + eps) * d1 if eps else d1, sign)
        return [s0 + s1, d0 + jd1, s0 - s1, d0 - jd1]
    if R == 5:
        c1, c2 = rt(math.cos(2.0 * math.pi / 5.0) + eps), rt(math.cos(4.0 * math.pi / 5.0))
        s1, s2 = rt(math.sin(2.0 * math.pi / 5.0)), rt(math.sin(4.0 * math.pi / 5.0))
        a = v[0]
        t1, t2, d1, d2 = v[1] + v[4], v[2] + v[3], v[1] - v[4], v[2] - v[3]
        m1 = a + c1 * t1 + c2 * t2
        m2 = a + c2 * t1 + c1 * t2
        n1 = _mulj(s1 * d1 + s2 * d2, sign)
        n2 = _mulj(s2 * d1 - s1 * d2, sign)
        return [a + t1 + t2, m1 + n1, m2 + n2, m2 - n2, m1 - n1]
    if R == 8:
        e = dft_small([v[0], v[2], v[4], v[6]], 4, sign, rt)
        o = dft_small([v[1], v[3], v[5], v[7]], 4, sign, rt)
        h = rt(math.sqrt(0.5) + eps)
        ct = e[0].dtype.type
        t = [o[0], o[1] * ct(complex(h, sign * h)), _mulj(o[2], sign), o[3] * ct(complex(-h, sign * h))]
        return [e[k] + t[k] for k in range(4)] + [e[k] - t[k] for k in range(4)]
    if R == 10:  # Good-Thomas 2 × 5: in n = (5·n1 + 2·n2) mod 10, out k = (5·k1 + 6·k2) mod 10
        a = [dft_small([v[(5 * n1 + 2 * n2) % 10] for n2 in range(5)], 5, sign, rt, eps) for n1 in range(2)]
        out = [None] * 10
        for k2 in range(5):
            out[(6 * k2) % 10] = a[0][k2] + a[1][k2]
            out[(5 + 6 * k2) % 10] = a[0][k2] - a[1][k2]
        return out
    raise ValueError(R)


def stockham_pass(buf, R, Ns, w, sign, rt, eps=0.0):
    """One autosort pass over the last axis.  w: None, or (R, Ns) twiddles (w[0] = w[:, 0] = 1)."""
    n = buf.shape[-1]
    nb = n // R
    x = buf.reshape(buf.shape[:-1] + (R, nb // Ns, Ns))  # [r, j / Ns, j % Ns] = buf[j + r·nb]
    if w is not None:
        x = x * w[:, None, :]
    v = dft_small([x[..., r, :, :] for r in range(R)], R, sign, rt, eps)
    return np.stack(v, axis=-2).reshape(buf.shape)       # [(j / Ns), r, j % Ns]


def _tree(w1, R):
    """W^r as a balanced product tree of W = w1: w[r] = w[r / 2] · w[r − r / 2]."""
    w = [np.ones_like(w1), w1]
    for r in range(2, R):
        w.append(w[r // 2] * w[r - r // 2])
    return np.stack(w[:R])


def _quarter(tq, Q, t, sign):
    """tw[t] (conjugated for sign > 0) from the quarter table tq[u] = tw[u], u < Q: tq[u]·(−j)^q, t = q·Q + u
    (ctq_bfly)."""
    q, u = t // Q, t % Q
    w0 = tq[u]
    wx = np.where(q & 1, w0.imag, w0.real)
    wy = np.where(q & 1, -w0.real, w0.imag)
    wx, wy = np.where(q & 2, -wx, wx), np.where(q & 2, -wy, wy)
    out = np.empty(t.shape, tq.dtype)
    out.real, out.imag = wx, (-wy if sign > 0 else wy)
    return out


def fft_rows(buf, radices, sign, dtype, table, stride=1, mode="direct", perturb=None, trace=None):
    """The row transform over the last axis (length M = prod(radices)).  table: the twiddle table, read at
    index·stride.  mode "direct": tw[k·r·tstep] (stockham_pass, wave_pass); "tree": powers of tw[k·tstep]
    (wave_fft_row_ct); "quarter": fft_lds_ct_q — the tree while (Ns − 1)·tstep < M/4, else every entry from
    the quarter table."""
    rt = np.float32 if np.dtype(dtype) == np.complex64 else np.float64
    M = buf.shape[-1]
    tab = table[::stride][:M].copy() if stride > 1 else table[:M].copy()
    if perturb is not None and perturb.kind == "pass_tw":
        tab[perturb.index] += rt(perturb.eps)
    tabs = np.conj(tab) if sign > 0 else tab
    Ns = 1
    for p, R in enumerate(radices):
        w = None
        if Ns > 1:
            tstep = M // (Ns * R)
            k = np.arange(Ns)
            if mode == "tree" or (mode == "quarter" and (Ns - 1) * tstep < M // 4):
                w = _tree(tabs[k * tstep], R)
            elif mode == "quarter":
                w = _quarter(tab[: M // 4], M // 4, k[None, :] * np.arange(R)[:, None] * tstep, sign)
            else:
                w = tabs[k[None, :] * np.arange(R)[:, None] * tstep]
        eps = perturb.eps if (perturb is not None and perturb.kind == "butterfly" and perturb.part == "rows"
                              and perturb.index == p and perturb.radix == R) else 0.0
        buf = stockham_pass(buf, R, Ns, w, sign, rt, eps)
        if trace is not None:
            trace.append((f"rows pass {p} radix {R} sign {sign:+d}", buf.copy()))
        Ns *= R
    return buf


def _literal(m, L, sign, dtype):
    """The register DFT's literal twiddle exp(sign·2πi·m/L), the angle reduced into (−π, π] (ct_angle)."""
    mm = m % L
    ms = mm - L if 2 * mm > L else mm
    ang = 2.0 * math.pi * ms / L
    return np.dtype(dtype).type(complex(math.cos(ang), sign * math.sin(ang)))


def reg_dft(x, P, sign, dtype, inplace, perturb=None):
    """The column P-point DFT over the last axis, natural order in and out: dft_reg_inplace's two-factor form
    where `inplace` and P has one, else dft_reg's Stockham passes with first_radix order."""
    rt = np.float32 if np.dtype(dtype) == np.complex64 else np.float64

    def beps(p, R):
        return perturb.eps if (perturb is not None and perturb.kind == "butterfly" and perturb.part == "cols"
                               and perturb.index == p and perturb.radix == R) else 0.0

    def weps(p):
        return rt(perturb.eps) if (perturb is not None and perturb.kind == "reg_tw" and perturb.index == p) else rt(0)

    if inplace and two_factor(P):
        R1 = first_radix(P)
        R2 = P // R1
        a = x.reshape(x.shape[:-1] + (R1, R2))  # [n1, n2] = x[R2·n1 + n2]
        a = dft_small([a[..., n1, :] for n1 in range(R1)], R1, sign, rt, beps(0, R1))  # [k1][..., n2]
        w = np.array([[_literal(n2 * k1, P, sign, dtype) for n2 in range(R2)] for k1 in range(R1)], dtype)
        w[1, 1] += weps(1)
        b = [a[k1] * w[k1] for k1 in range(R1)]
        out = [dft_small([bk[..., n2] for n2 in range(R2)], R2, sign, rt, beps(1, R2)) for bk in b]  # [k1][k2]
        # X[k1 + R1·k2]
        return np.stack([np.stack(o, axis=-1) for o in out], axis=-1).reshape(x.shape)
    Ns = 1
    for p, R in enumerate(_radices(P, first_radix)):
        w = None
        if Ns > 1:
            w = np.array([[_literal(k * r, Ns * R, sign, dtype) for k in range(Ns)] for r in range(R)], dtype)
            w[1, 1] += weps(p)
        x = stockham_pass(x, R, Ns, w, sign, rt, beps(p, R))
        Ns *= R
    return x


def transform(x, layout, sign, dtype=np.complex64, perturb=None, trace=None):
    """The engine's transform of every row of x (…, N) in `dtype` arithmetic.

    sign −1: forward; the result is in natural order for the one-workgroup layout and TRANSPOSED,
    XT[kq·M + k] = X[kq + P·k], for the four-step and huge layouts.  sign +1: inverse (unnormalised) of a
    spectrum in that same storage, natural order out."""
    kind, P, M, radix, ct = layout
    x = np.asarray(x).astype(dtype)
    if kind == "lds":
        return fft_rows(x, radix, sign, dtype, twiddle_table(M, dtype), perturb=perturb, trace=trace)
    N = P * M
    twN = twiddle_table(N, dtype)
    if kind == "four_step":
        row_ct = ct if sign < 0 else (P, M) in BIG_CT_SEARCH
        rows = dict(radices=ct_plan(M) if row_ct else radix, table=twN, stride=P, mode="tree" if row_ct else "direct")
        col_tree = sign < 0 or row_ct   # acq_fft_big_cols_kernel always; acq_search_big_kernel for MC > 0
    else:
        rows = dict(radices=ct_plan(M) if ct else radix, table=twiddle_table(M, dtype), stride=1, mode="quarter" if ct else "direct")
        col_tree = True                 # col_twiddles
    t = np.arange(M)
    w1 = twN[:M].copy()
    if perturb is not None and perturb.kind == "col_tw":
        w1[perturb.index] += (np.float32 if np.dtype(dtype) == np.complex64 else np.float64)(perturb.eps)
    if col_tree:
        wcol = _tree(w1, P).T                                   # [t, kq] = (W_N^t)^kq
    else:
        wcol = twN[t[:, None] * np.arange(P)[None, :]]          # tw[t·kq]
        wcol[:, 1] = w1
    if sign < 0:
        cols = x.reshape(x.shape[:-1] + (P, M)).swapaxes(-1, -2)            # [t, q] = x[t + M·q]
        X = reg_dft(cols, P, -1, dtype, kind == "four_step", perturb) * wcol  # [t, kq]
        if trace is not None:
            trace.append(("columns forward", X.copy()))
        T = np.ascontiguousarray(X.swapaxes(-1, -2))                          # rows kq, m
        XT = fft_rows(T, sign=-1, dtype=dtype, perturb=perturb, trace=trace, **rows)
        return XT.reshape(x.shape)
    U = fft_rows(x.reshape(x.shape[:-1] + (P, M)), sign=+1, dtype=dtype, perturb=perturb, trace=trace, **rows)  # [kq, t]
    V = np.ascontiguousarray(U.swapaxes(-1, -2)) * np.conj(wcol)             # [t, kq]
    y = reg_dft(V, P, +1, dtype, kind == "four_step", perturb)               # [t, q] = y[t + M·q]
    return np.ascontiguousarray(y.swapaxes(-1, -2)).reshape(x.shape)


def natural_order(XT, layout):
    """A forward result of `transform` in natural order: X[kq + P·k] = XT[kq·M + k]."""
    if layout.kind == "lds":
        return XT
    return np.ascontiguousarray(XT.reshape(XT.shape[:-1] + (layout.P, layout.row_len)).swapaxes(-1, -2)).reshape(XT.shape)


def grid(sig, code, wipeoffs, layout, dtype=np.complex64, perturb=None):
    """|IFFT(FFT(sig ⊙ w_b) ⊙ conj(FFT(code)))|², unnormalised, one row per wipeoff row; the wipeoff product
    in float32 (volk_32fc_x2_multiply_32fc) whatever `dtype`, as the oracle's acquisition_grid."""
    n = wipeoffs.shape[1]
    sig = np.ascontiguousarray(sig[:n], np.complex64)
    code = np.ascontiguousarray(code[:n], np.complex64)
    wiped = (sig[None, :] * wipeoffs).astype(np.complex64)
    X = transform(wiped, layout, -1, dtype, perturb)
    C = np.conj(transform(code[None, :], layout, -1, dtype, perturb))
    Y = transform(X * C, layout, +1, dtype, perturb)
    return (Y.real * Y.real + Y.imag * Y.imag).astype(np.float32)


# ---- the cases of tests/test_gpu_acq_fft_coverage.py, shared with tests/test_acq_fft_model.py -------------

class Case(NamedTuple):
    n: int          # fft_size
    force: int      # 0, 1 = GNSSHIP_ACQ_FORCE_BIG, 2 = GNSSHIP_ACQ_FORCE_HUGE
    huge_p: int     # GNSSHIP_ACQ_HUGE_P (0: unset)
    layout: Layout  # the layout the case is written for
    planted: bool   # also a planted-peak case (one per layout family)

    @property
    def id(self):
        return f"{self.n}" + ("-big" if self.force == 1 else f"-huge{self.huge_p}" if self.force == 2 else "")

    @property
    def env(self):
        e = {}
        if self.force == 1:
            e["GNSSHIP_ACQ_FORCE_BIG"] = "1"
        if self.force == 2:
            e["GNSSHIP_ACQ_FORCE_HUGE"] = "1"
            e["GNSSHIP_ACQ_HUGE_P"] = str(self.huge_p)
        return e


def _lds(n, radix, planted=False):
    return Case(n, 0, 0, Layout("lds", 0, n, tuple(radix), False), planted)


def _big(n, force, p, radix, planted=False):
    return Case(n, force, 0, Layout("four_step", p, n // p, tuple(radix), (n // p) in BIG_CT_ROWS), planted)


def _huge(n, p, radix, force=0, planted=False):
    return Case(n, force, p if force else 0, Layout("huge", p, n // p, tuple(radix), (n // p) in HUGE_CT_ROWS), planted)


CASES = [
    # one-workgroup LDS
    _lds(2, [2]), _lds(3, [3]), _lds(4, [4]), _lds(5, [5]), _lds(6, [3, 2]), _lds(30, [5, 3, 2]), _lds(60, [5, 4, 3], True),
    _lds(960, [8, 8, 5, 3]), _lds(4096, [8] * 4), _lds(4320, [8, 5, 4, 3, 3, 3]), _lds(13122, [3] * 8 + [2]),
    _lds(15552, [8, 8] + [3] * 5), _lds(15625, [5] * 6), _lds(16384, [8] * 4 + [4]),
    # four-step
    _big(32, 1, 16, [2]), _big(96, 1, 16, [3, 2]), _big(135, 1, 27, [5]), _big(270, 1, 18, [5, 3]),
    _big(600, 1, 20, [5, 3, 2], True), _big(675, 1, 25, [3, 3, 3]), _big(12288, 1, 16, [8, 8, 4, 3]),
    _big(15552, 1, 16, [4] + [3] * 5), _big(18432, 0, 18, [8, 8, 8, 2]), _big(20000, 0, 20, [8, 5, 5, 5]),
    _big(24576, 0, 24, [8, 8, 8, 2]), _big(27000, 0, 27, [8, 5, 5, 5]), _big(30000, 0, 30, [8, 5, 5, 5]),
    _big(30720, 0, 30, [8, 8, 8, 2]), _big(32000, 0, 32, [8, 5, 5, 5]),
    # huge, small: p × 60
    *[_huge(p * 60, p, [5, 4, 3], force=2, planted=p in (5, 32)) for p in HUGE_P],
    # huge, natural
    _huge(36000, 4, [8, 5, 5, 5, 3, 3]), _huge(62500, 5, [5] * 5 + [4], planted=True), _huge(98304, 8, [8] * 4 + [3]),
    _huge(125000, 10, [5] * 5 + [4]), _huge(131072, 8, [8] * 4 + [4]), _huge(200000, 20, [8, 5, 5, 5, 5, 2]),
    _huge(262144, 16, [8] * 4 + [4]), _huge(312500, 25, [5] * 5 + [4]), _huge(320000, 32, [8, 5, 5, 5, 5, 2]),
    _huge(524288, 32, [8] * 4 + [4]),
]

DOPPLER_MAX = DOPPLER_STEP = 250  # two bins: −250 Hz and 0 Hz
SEED_NOISE, SEED_PLANT = 0x6E55A002, 0x6E55B008  # chosen so that every case's reference grid has a unique maximum


def noise_inputs(n, seed=SEED_NOISE):
    """Noise-only input of a case: sig and code complex64 standard normal, no satellite."""
    rng = np.random.default_rng([seed, n])
    z = rng.standard_normal((2, n, 2)).astype(np.float32)
    return np.ascontiguousarray(z[0]).view(np.complex64).ravel(), np.ascontiguousarray(z[1]).view(np.complex64).ravel()


def planted_inputs(n, d, seed=SEED_PLANT):
    """sig = A·roll(code, d)·w₀⁻¹ + noise with a random ±1 code; w₀, the 0 Hz wipeoff, is all ones.  The
    correlation peak (A·n)² stands 20× over the noise cells' mean 2n: A = √(40/n)."""
    rng = np.random.default_rng([seed, n])
    code = (2.0 * rng.integers(0, 2, n) - 1.0).astype(np.complex64)
    z = rng.standard_normal((n, 2)).astype(np.float32)
    noise = np.ascontiguousarray(z).view(np.complex64).ravel()
    sig = (np.float32(math.sqrt(40.0 / n)) * np.roll(code, d) + noise).astype(np.complex64)
    return sig, code


def planted_delays(case, spc):
    """The code delays of a planted-peak case: the edges of the row, of the second-peak window's wrap, of the
    first column pair and, in the huge layout, of the 256-column tiles and the last register point."""
    n, lay = case.n, case.layout
    if lay.kind == "lds":
        return sorted({0, 1, spc - 1, n - spc, n - 1} & set(range(n)))
    M, P = lay.row_len, lay.P
    d = {0, 1, spc - 1, n - spc, n - 1, M - 1, M, M + 1}
    if lay.kind == "huge":
        d |= {255, 256, M * (P - 1)}
    return sorted(x for x in d if 0 <= x < n)


def samples_per_chip(n):
    """Acq_Conf::SetDerivedParams at fs = 1000·n and the GPS L1 C/A chip rate, as engine.PcpsAcquisition."""
    return int(np.ceil(np.float32(1000 * n) / np.float32(1023000.0)))


def samples_per_code(n):
    return float(np.float32(np.float32(1000 * n) * np.float32(0.001)))


class Reference(NamedTuple):
    sig: np.ndarray
    code: np.ndarray
    wipe: np.ndarray   # the two wipeoff rows, complex64
    ref: np.ndarray    # the complex128 grid, float32[2, n]


@functools.lru_cache(maxsize=None)
def reference(n, d=None):
    """Inputs (noise-only, or the planted peak at delay d) and the oracle's complex128 grid of a case at
    fs = 1000·n, computed once per process and shared read-only."""
    from oracle import oracle as O
    sig, code = noise_inputs(n) if d is None else planted_inputs(n, d)
    wipe = O.doppler_wipeoff_grid(2, n, DOPPLER_MAX, DOPPLER_STEP, 0, 1000 * n)
    ref = O.acquisition_grid(sig, code, wipe)
    for a in (sig, code, wipe, ref):
        a.flags.writeable = False
    return Reference(sig, code, wipe, ref)
