"""The interference-mitigation model (tests/mit_model.py) on its own: the reference's quirks it must hold, its cut
invariance, the conditions the GPU scenarios rely on (tests/mit_scenarios.py), and gnsship_mit_threshold against
scipy.  No GPU."""
import numpy as np
import pytest
from scipy.stats import chi2

import mit_model as M
import mit_scenarios as S

F = np.float32


def tone(n, amp=8.0, f=0.05):
    return (S.noise(n, 3) + amp * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)


def test_notch_forms_output_k_from_input_k_plus_1():
    """notch_cc.cc:72: `in++` without history.  Copied (estimation) segments show the advance directly; a
    segment is emitted only once the sample after it has arrived."""
    L = 4
    x = S.noise(3 * L + 1, 1)
    m = M.Model(M.NOTCH, 1e9, L, 100, 1000)
    assert len(m.run(x[:L])) == 0            # segment 0 needs x[L]
    y = m.run(x[L:])
    assert np.array_equal(y, x[1:3 * L + 1])
    # filtered: sample k from x[k + 1] with x[k] the previous sample, last_out = 0 on entry
    m = M.Model(M.NOTCH, 1e-9, L, 1, 1000, p_c=0.5)
    y = m.run(x)
    k = L  # first sample of the first filtered segment
    ang = M.angle(x[k + 1:k + 2], x[k:k + 1])
    zr, zi = M.z0_of(ang)
    tr, ti = M.cmul(zr, zi, x[k:k + 1].real, x[k:k + 1].imag)
    assert y[k] == np.complex64(complex(F(x[k + 1].real - tr[0]), F(x[k + 1].imag - ti[0])))


def test_notch_lite_has_a_zero_sample_before_the_stream():
    """notch_lite_cc.cc:61 set_history(2): output k from input k; the previous sample of input 0 is zero."""
    L = 4
    x = tone(4 * L)
    m = M.Model(M.NOTCH_LITE, 1e9, L, 100, 1000)
    assert np.array_equal(m.run(x), x)      # emitted as soon as the segment itself is complete
    # first filtered sample at stream start is impossible (segment 0 always estimates); check the previous sample
    # of the first filtered segment is the stream's, and that a zero-length history would change the output
    m = M.Model(M.NOTCH_LITE, 1e-9, L, 1, 1000, p_c=0.5, n_coeff=100)
    assert m.carry[0] == 0 and m.pending == 0
    y = m.run(x)
    zr, zi = m.z0
    tr, ti = M.cmul(F(zr), F(zi), x[L - 1].real, x[L - 1].imag)
    assert y[L] == np.complex64(complex(F(x[L].real - tr), F(x[L].imag - ti)))
    assert m.carry[0] == x[-1]


def test_pulse_blanking_restarts_the_estimate_at_n_segments_1():
    """pulse_blanking_cc.cc:85-94: the reset sets n_segments_ = 0 and the loop's increment makes it 1, so the new
    window has n_segments_est − 1 segments, the first weighted against the old estimate."""
    L, n_est, n_reset = 4, 3, 5
    x = S.noise(12 * L, 5)
    m = M.Model(M.PULSE_BLANKING, 1e9, L, n_est, n_reset)
    trace = []
    for s in range(12):
        m.run(x[s * L:(s + 1) * L])
        trace.append((m.n_segments, float(m.noise)))
    assert [t[0] for t in trace] == [1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6]
    # segments 7, 8 (n_segments_ 1, 2) estimate; 9.. do not
    assert trace[6][1] == trace[5][1] and trace[7][1] != trace[6][1] and trace[8][1] != trace[7][1] and trace[9][1] == trace[8][1]
    e7 = M.energy(x[7 * L:8 * L])
    assert F(trace[7][1]) == F(F(F(1) * F(trace[6][1]) + F(e7 / F(2 * L))) / F(2))


@pytest.mark.parametrize("kind", [M.NOTCH, M.NOTCH_LITE])
def test_last_out_is_cleared_on_entering_the_filter_state(kind):
    L = 8
    n = 40 * L
    x = S.noise(n, 9)
    t = np.arange(n)
    on = ((t >= 4 * L) & (t < 12 * L)) | ((t >= 20 * L) & (t < 30 * L))
    x = (x + on * 30.0 * np.exp(2j * np.pi * 0.11 * t)).astype(np.complex64)
    th = S.thres_pfa(1e-6, L) * 4
    m = M.Model(kind, th, L, 2, 10**6, p_c=0.9)
    y = m.run(x)
    c = np.array(m.codes)
    twos = np.nonzero(c == 2)[0]
    assert len(twos) >= 2 and c[twos[1] - 1] == 0
    # the second run equals a fresh block's output on it, given the same noise estimate: its first sample is b alone
    s = twos[1]
    m2 = M.Model(kind, th, L, 2, 10**6, p_c=0.9)
    m2.noise, m2.n_segments = m.noise, 100
    m2.carry = x[s * L - 1:s * L].copy() if kind == M.NOTCH_LITE else np.concatenate([x[s * L - 1:s * L], x[s * L:s * L + 1]])
    lo = s * L if kind == M.NOTCH_LITE else s * L + 1
    y2 = m2.run(x[lo:lo + 3 * L])
    assert np.array_equal(y2[:2 * L].view(np.uint32), y[s * L:(s + 2) * L].view(np.uint32))


@pytest.mark.parametrize("kind,length", [(k, L) for k in (M.PULSE_BLANKING, M.NOTCH, M.NOTCH_LITE) for L in (5, 32)])
def test_model_cut_invariance(kind, length):
    M.require_glibc()
    x = S.pulsed(length) if kind == M.PULSE_BLANKING else S.cw_gated(length, S.NOTCH_SEEDS[(kind, length)])
    x = x[:60 * length + 3]
    th = S.thres_pfa(0.04, length) if kind == M.PULSE_BLANKING else S.notch_thres(length)
    whole = M.Model(kind, th, length, S.N_EST, S.N_RESET, n_coeff=3)
    yw = whole.run(x)
    cutm = M.Model(kind, th, length, S.N_EST, S.N_RESET, n_coeff=3)
    cuts = [1, length - 1, length, length + 1, 7 * length + 3, 0] + [1] * (3 * length)
    yc = M.run_cut(cutm, x, cuts)
    assert np.array_equal(yw.view(np.uint32), yc.view(np.uint32))
    assert whole.state() == cutm.state() and whole.noise.tobytes() == cutm.noise.tobytes()
    assert whole.codes == cutm.codes


@pytest.mark.parametrize("pfa,length", [(0.04, 32), (0.001, 32), (0.04, 2), (0.001, 2), (0.04, 1024), (0.001, 1024)])
def test_threshold_matches_scipy(built, pfa, length):
    """One float rounding of a double result, doubled: 2^-23 relative.  (0.04, 32) is the pulse-blanking default,
    (0.001, 32) the default of both notches."""
    from gnss_sim_receiver_amd import abi, engine
    t = engine.mit_threshold(abi.load(), pfa, length)
    ref = chi2.isf(pfa, 2 * length)
    assert abs(t - ref) <= 2.0 ** -23 * ref, (t, ref)


def test_threshold_rejects_bad_arguments(built):
    from gnss_sim_receiver_amd import abi, engine
    for pfa, length in [(0.0, 32), (1.0, 32), (-0.1, 32), (0.01, 1), (0.01, 1025)]:
        with pytest.raises(abi.GnssHipError):
            engine.mit_threshold(abi.load(), pfa, length)


@pytest.mark.parametrize("kind", [M.NOTCH, M.NOTCH_LITE])
@pytest.mark.parametrize("length", S.LENGTHS)
def test_notch_scenarios_keep_clear_of_the_threshold(kind, length):
    """Every detection-phase segment of the GPU scenarios has E/(noise·thres) outside [1 − 1e-3, 1 + 1e-3] (three
    orders above the float32 rounding of the estimate), so the device's decisions cannot differ from the model's
    through the estimate's tolerance; both decisions, entries into the filter state and several estimation
    windows occur."""
    M.require_glibc()
    x, th, m, y = S.notch_case(kind, length)
    r = np.array(m.ratios)
    assert len(r) + np.sum(np.array(m.codes) == 0) >= len(m.codes)  # every segment estimated or decided
    assert np.all(np.abs(r - 1.0) > 1e-3), np.abs(r - 1.0).min()
    c = np.bincount(np.array(m.codes), minlength=3)
    assert c[0] > S.N_EST and c[1] > 0 and c[2] >= 3
    print(f"kind {kind} length {length}: float32 noise estimate against float64, largest relative error {m.est_err:.3e}")
    assert m.est_err < 1e-4


def test_speculation_prediction_on_the_continuous_cw_stream():
    """The emulated speculative form over one unbroken filtered run of at least 20 chunks: nothing refuted at
    p_c_factor 0.9, refutations at 1.0 (no decay: a chain from the zero state never meets the true one)."""
    M.require_glibc()
    chunk, warm = S.chain_geometry(0.9)
    x, th, m, y = S.chain_case(0.9, chunk, warm)
    c = np.array(m.codes)
    assert np.all(c[S.N_EST + 1:] == 1) and c[S.N_EST] == 2
    assert m.chunks_speculated >= 20 and m.chunks_replayed == 0
    chunk, warm = S.chain_geometry(1.0)
    x, th, m, y = S.chain_case(1.0, chunk, warm)
    assert m.chunks_speculated > 0 and m.chunks_replayed > 0
