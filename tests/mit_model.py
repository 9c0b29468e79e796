"""Model of the interference-mitigation blocks (gnss_sim_receiver_amd/csrc/mit_filter.hip): pulse_blanking_cc.cc:57-98,
notch_cc.cc:63-121 and notch_lite_cc.cc:71-138 restated in numpy, float32 scalars in the reference's order.

Each block is defined on the stream: segments of `length` samples from the first sample, through the block's
state machine in order; a run emits every complete segment not yet emitted.  The notch keeps the block's
`in++` without history (output k from input k + 1, input k the previous sample: a segment is complete once
input sample (s + 1)·length has arrived); the lite form has set_history(2) (output k from input k, zero
before the stream).

sinf / cosf / atan2f come from the host's libm (glibc's, which the device headers restate): require_glibc()
skips where that is another glibc.  The notches' estimation phase (direct DFT, VOLK's generic power spectrum
10·log10f(|X|² + 1e-20) and spectral noise floor, pow(10, dB/10)/(2·length)) is evaluated in float32 in the
device's order and, beside it, in float64 (noise64): the device's estimate is compared with the float64 one.

Given chunk_samples and warmup_samples the model also emulates the speculative chain form and counts the
chunks whose predicted start state is refuted.
"""
import ctypes
import ctypes.util

import numpy as np

PULSE_BLANKING, NOTCH, NOTCH_LITE = 0, 1, 2
F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _k in (("sinf", 1), ("cosf", 1), ("atan2f", 2), ("log10f", 1), ("powf", 2)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k

RESTATED_GLIBC = "2.35"


def host_glibc():
    fn = ctypes.CDLL(None).gnu_get_libc_version
    fn.restype = ctypes.c_char_p
    return fn().decode()


def require_glibc():
    """The skip of tests/test_glibc_sincosf.py: the device restates glibc 2.35's FMA build of the float libm."""
    import pytest
    if host_glibc() != RESTATED_GLIBC:
        pytest.skip(f"host glibc {host_glibc()}: the device headers restate glibc {RESTATED_GLIBC}'s float libm")
    with open("/proc/cpuinfo") as f:
        if " fma" not in f.read():
            pytest.skip("host without FMA: glibc runs its non-FMA sinf/cosf build, which the device does not restate")


def _vec(fn, *arrs):
    f = getattr(_libm, fn)
    return np.array([f(*t) for t in zip(*[np.asarray(a, F).reshape(-1).tolist() for a in arrs])], F).reshape(np.shape(arrs[0]))


def cmul(ar, ai, br, bi):
    """std::complex<float> product (libgcc __mulsc3, finite values): (ac − bd, ad + bc), every op rounded."""
    return (ar * br - ai * bi).astype(F), (ar * bi + ai * br).astype(F)


def angle(x, p):
    """volk_32fc_x2_multiply_conjugate_32fc + volk_32fc_s32f_atan2_32f: atan2f of x·conj(p)."""
    cr, ci = cmul(x.real.astype(F), x.imag.astype(F), p.real.astype(F), (-p.imag).astype(F))
    return _vec("atan2f", ci, cr)


def z0_of(ang):
    """std::exp(gr_complex(0, 1)·angle) as glibc's cexpf evaluates it."""
    return _vec("cosf", ang), _vec("sinf", ang)


def energy(seg):
    """Serial float32 sum of re·re + im·im over the rows of seg."""
    re, im = seg.real.astype(F), seg.imag.astype(F)
    m = (re * re).astype(F) + (im * im).astype(F)
    return np.cumsum(m.astype(F), axis=-1, dtype=F)[..., -1]


def twiddles(L):
    ph = 2.0 * np.pi * np.arange(L, dtype=np.float64) / L
    return np.cos(ph).astype(F), (-np.sin(ph)).astype(F)


def noise_floor(p, excl, dt):
    """volk_32f_s32f_calc_spectral_noise_floor_32f, generic."""
    s = dt(0)
    for v in p:
        s = dt(s + v)
    mean = dt(dt(s / dt(len(p))) + dt(excl))
    cnt = len(p)
    for v in p:
        if v > mean:
            s = dt(s - v)
            cnt -= 1
    return mean if cnt == 0 else dt(s / dt(cnt))


def estimate32(seg):
    """sig2lin of one estimation segment, float32, the device's order (direct DFT, serial sums)."""
    L = len(seg)
    wr, wi = twiddles(L)
    idx = (np.arange(L)[:, None] * np.arange(L)[None, :]) % L
    xr, xi = seg.real.astype(F)[None, :], seg.imag.astype(F)[None, :]
    pr, pi = cmul(xr, xi, wr[idx], wi[idx])
    re = np.cumsum(pr, axis=1, dtype=F)[:, -1]
    im = np.cumsum(pi, axis=1, dtype=F)[:, -1]
    mag = ((re * re).astype(F) + (im * im).astype(F)).astype(F)
    p = (mag.astype(np.float64) + 1e-20).astype(F)
    db = (F(10.0) * _vec("log10f", p)).astype(F)
    nf = noise_floor(db, 15.0, F)
    return F(F(_libm.powf(F(10.0), F(nf / F(10.0)))) / F(2 * L))


def estimate64(seg):
    """The same formula in float64."""
    L = len(seg)
    X = np.fft.fft(seg.astype(np.complex128))
    db = 10.0 * np.log10(X.real ** 2 + X.imag ** 2 + 1e-20)
    nf = noise_floor(db, 15.0, np.float64)
    return 10.0 ** (nf / 10.0) / (2 * L)


class Model:
    def __init__(self, kind, thres, length, n_est, n_reset, p_c=0.9, n_coeff=1, chunk_samples=None, warmup_samples=None):
        self.kind, self.L, self.thres = kind, int(length), F(thres)
        self.n_est, self.n_reset, self.n_coeff_reset = n_est, n_reset, n_coeff
        self.p_c = F(p_c)
        self.off = 2 if kind == NOTCH else 1
        self.chunk_segs = chunk_samples // self.L if chunk_samples else None
        self.warm_segs = warmup_samples // self.L if warmup_samples else None
        self.reset()

    def reset(self):
        self.carry = np.zeros(1, np.complex64)  # [0]: the sample before the first unemitted output position
        self.noise, self.noise64 = F(0), 0.0
        self.n_segments, self.flag, self.n_coeff = 0, False, 0
        self.z0 = (F(0), F(0))
        self.last = (F(0), F(0))
        self.samples_in = self.samples_out = 0
        self.chunks_speculated = self.chunks_replayed = 0
        self.codes, self.ratios = [], []  # per segment since reset: code, E/(noise·thres) of detection segments
        self.n_trace = []                 # per segment since reset: n_segments_ on entry
        self.est_err = 0.0                # largest relative error of the float32 noise estimate against float64

    @property
    def pending(self):
        return len(self.carry) - 1

    def state(self):
        return dict(n_segments=self.n_segments, filter_state=int(self.flag), n_segments_coeff=self.n_coeff,
                    samples_in=self.samples_in, samples_out=self.samples_out, pending_samples=self.pending)

    def run(self, x):
        x = np.asarray(x, np.complex64)
        L, off = self.L, self.off
        V = np.concatenate([self.carry, x])
        avail = len(V) - 1
        nseg = (max(avail - 1, 0) // L if avail >= 1 else 0) if off == 2 else avail // L
        self.samples_in += len(x)
        self.samples_out += nseg * L
        self.carry = V[nseg * L:].copy()
        if nseg == 0:
            return np.zeros(0, np.complex64)
        cur = V[off: off + nseg * L].reshape(nseg, L)
        prev = V[off - 1: off - 1 + nseg * L].reshape(nseg, L)
        E = energy(cur)
        notch = self.kind != PULSE_BLANKING
        deg = F(2 * L)
        code = np.zeros(nseg, np.int8)
        zseg = [None] * nseg
        for s in range(nseg):
            n = self.n_segments
            self.n_trace.append(n)
            if n < self.n_est and not self.flag:
                if notch:
                    lin, lin64 = estimate32(cur[s]), estimate64(cur[s])
                else:
                    lin = F(E[s] / deg)
                    lin64 = float(lin)
                self.noise = F(F(F(n) * self.noise + lin) / F(n + 1))
                self.noise64 = (n * self.noise64 + lin64) / (n + 1)
                if notch and self.noise64 > 0:
                    self.est_err = max(self.est_err, abs(float(self.noise) - self.noise64) / self.noise64)
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = F(E[s] / self.noise)
                    self.ratios.append(float(r) / float(self.thres))
                if r > self.thres:
                    if notch:
                        code[s] = 1 if self.flag else 2
                        if not self.flag:
                            self.n_coeff = 0
                        if self.kind == NOTCH_LITE:
                            if self.n_coeff == 0:
                                a1 = angle(cur[s][1:2], cur[s][0:1])[0]
                                a2 = angle(cur[s][L - 1:L], cur[s][L - 2:L - 1])[0]
                                zr, zi = z0_of(np.array([F(F(a1 + a2) / F(2.0))], F))
                                self.z0 = (zr[0], zi[0])
                            zseg[s] = self.z0
                            self.n_coeff = (self.n_coeff + 1) % self.n_coeff_reset
                    else:
                        code[s] = 1
                    self.flag = True
                else:
                    self.flag = False
                    if self.n_segments > self.n_reset:
                        self.n_segments = 0
            self.n_segments += 1
        self.codes.extend(int(c) for c in code)
        out = cur.copy()
        if not notch:
            out[code != 0] = 0
            return out.reshape(-1)
        # a = p_c·z0, b = x − z0·prev on the filtered segments
        f = np.nonzero(code)[0]
        ar = np.zeros((nseg, L), F)
        ai, br, bi = ar.copy(), ar.copy(), ar.copy()
        if len(f):
            xc, xp = cur[f], prev[f]
            if self.kind == NOTCH:
                zr, zi = z0_of(angle(xc, xp))
            else:
                zr = np.array([[zseg[s][0]] * L for s in f], F)
                zi = np.array([[zseg[s][1]] * L for s in f], F)
            tr, ti = cmul(zr, zi, xp.real.astype(F), xp.imag.astype(F))
            br[f], bi[f] = (xc.real.astype(F) - tr).astype(F), (xc.imag.astype(F) - ti).astype(F)
            ar[f], ai[f] = cmul(np.full_like(zr, self.p_c), np.zeros_like(zr), zr, zi)
        coef = (ar.reshape(-1).tolist(), ai.reshape(-1).tolist(), br.reshape(-1).tolist(), bi.reshape(-1).tolist())
        y_before = [None] * nseg  # the true state entering each segment
        y = self.last
        flat = out.reshape(-1)
        for s in range(nseg):
            y_before[s] = y
            y = self._chain(coef, code, s, s + 1, y, flat)
        self.last = y
        if self.chunk_segs:
            self._speculate(coef, code, y_before)
        return flat

    def _chain(self, coef, code, s_from, s_to, y, flat=None):
        ar, ai, br, bi = coef
        L = self.L
        yr, yi = y
        for s in range(s_from, s_to):
            if code[s] == 0:
                continue
            if code[s] == 2:
                yr, yi = F(0), F(0)
            for j in range(s * L, (s + 1) * L):
                a_r, a_i = F(ar[j]), F(ai[j])
                tr = F(F(a_r * yr) - F(a_i * yi))
                ti = F(F(a_r * yi) + F(a_i * yr))
                yr, yi = F(F(br[j]) + tr), F(F(bi[j]) + ti)
                if flat is not None:
                    flat[j] = complex(yr, yi)
        return yr, yi

    def _speculate(self, coef, code, y_before):
        """mit_chain_spec_kernel / mit_chain_fix_kernel: which chunks start from a prediction, which are refuted."""
        nseg, cs, ws = len(code), self.chunk_segs, self.warm_segs
        for c in range(1, (nseg + cs - 1) // cs):
            s0 = c * cs
            if code[s0] != 1:
                continue
            sb = max(s0 - ws, 0)
            if sb == 0 or any(code[s] != 1 for s in range(sb, s0)):
                continue
            self.chunks_speculated += 1
            y = self._chain(coef, code, sb, s0, (F(0), F(0)))
            t = y_before[s0]
            if y[0].tobytes() != t[0].tobytes() or y[1].tobytes() != t[1].tobytes():
                self.chunks_replayed += 1


def run_cut(model, x, cuts):
    """The stream in runs of the given lengths (the rest in one last run); returns the concatenated output."""
    outs, pos = [], 0
    for n in list(cuts) + [None]:
        end = len(x) if n is None else min(pos + n, len(x))
        outs.append(model.run(x[pos:end]))
        pos = end
        if pos >= len(x) and n is not None:
            break
    return np.concatenate(outs)
