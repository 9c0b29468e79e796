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


# ---- the coverage scenarios of tests/test_gpu_mit_coverage.py ----

def runs_of(codes):
    """Maximal runs [a, b) of filtered segments."""
    c = np.concatenate([[0], (np.asarray(codes) != 0).astype(np.int8), [0]])
    d = np.diff(c)
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


@pytest.mark.parametrize("kind", [M.NOTCH, M.NOTCH_LITE])
@pytest.mark.parametrize("length", S.COV_LENGTHS)
def test_coverage_lengths_keep_clear_of_the_threshold(kind, length):
    """As test_notch_scenarios_keep_clear_of_the_threshold, for the lengths 2, 13, 255, 257; the cut of the two-run test
    lies inside a filtered run; the thresholds at 255 and 257 lie between noise alone and the tone."""
    M.require_glibc()
    x, th, m, y = S.cov_length_case(kind, length)
    r = np.array(m.ratios)
    c = np.bincount(np.array(m.codes), minlength=3)
    print(f"kind {kind} length {length} threshold {th:.1f} seed {S.COV_NOTCH_SEEDS[(kind, length)]}: codes {c.tolist()}, "
          f"smallest |ratio - 1| {np.abs(r - 1.0).min():.3e}, est_err {m.est_err:.3e}")
    assert np.all(np.abs(r - 1.0) > 1e-3), np.abs(r - 1.0).min()
    assert c[0] > S.N_EST and c[1] > 0 and c[2] >= 3
    assert m.est_err < 1e-4
    cs = (S.run_cut_sample(length, len(x)) - m.off) // length   # the segment the cut falls in
    assert m.codes[cs - 1] != 0 and m.codes[cs] != 0 and m.codes[cs + 1] != 0
    if length >= 255:
        assert S.thres_pfa(0.001, length) < 700 < th                      # the pfa threshold: below noise alone
        assert np.median(r[r < 1.0]) * th > S.thres_pfa(0.001, length)        # noise alone sits above the pfa threshold
        assert np.median(r[r < 1.0]) < 0.5 and r[r < 1.0].max() < 0.8 and r[r > 1.0].min() > 1.2   # the two decisions, well apart


@pytest.mark.parametrize("length", S.COV_LENGTHS)
def test_coverage_lengths_pulse_blanking_decides_both_ways(length):
    x, th, m, y = S.cov_length_case(M.PULSE_BLANKING, length)
    c = np.bincount(np.array(m.codes), minlength=2)
    assert c[0] > S.N_EST and c[1] >= 3
    assert max(m.n_trace) > S.N_RESET and m.n_trace.count(1) >= 2         # resets and new estimation windows


@pytest.mark.parametrize("length", S.COV_CHAIN_LENGTHS)
def test_coverage_chain_is_one_unbroken_run(length):
    M.require_glibc()
    chunk, warm = S.chain_geometry(0.9, length)
    assert chunk % length == 0 and warm % length == 0 and chunk >= 2048
    x, th, m, y = S.cov_chain_case(length, 0.9, chunk, warm)
    c = np.array(m.codes)
    assert np.all(c[S.N_EST + 1:] == 1) and c[S.N_EST] == 2
    assert np.all(np.abs(np.array(m.ratios) - 1.0) > 1e-3)
    assert m.chunks_speculated >= 10 and m.chunks_replayed == 0
    chunk, warm = S.chain_geometry(1.0, length)
    x, th, m, y = S.cov_chain_case(length, 1.0, chunk, warm)
    assert m.chunks_speculated > 0 and m.chunks_replayed > 0


@pytest.mark.parametrize("which", sorted(S.EDGE_RUNS))
@pytest.mark.parametrize("kind,n_coeff", [(M.PULSE_BLANKING, 1), (M.NOTCH, 1), (M.NOTCH_LITE, 3), (M.NOTCH_LITE, 5000)])
def test_tile_edge_runs_are_exactly_the_gating(kind, n_coeff, which):
    """The model filters exactly the gated segments: a run that is one scan tile of 1024, one across a tile edge, a
    single segment last (a) or first (b) in a tile, and one with two tiles wholly inside it; no reset, so every tile
    past the first is decided at once."""
    M.require_glibc()
    x, th, m, y = S.edge_case(kind, n_coeff, which)
    assert len(m.codes) == 8192 - (1 if kind == M.NOTCH else 0)
    assert tuple(runs_of(m.codes)) == S.EDGE_RUNS[which]
    runs = S.EDGE_RUNS[which]
    assert (1024, 2048) in runs and (3071, 3073) in runs
    assert ((4095, 4096) in runs) != ((4096, 4097) in runs)
    a, b = runs[-1]
    assert b - a > 2048 and sum(a <= t and t + 1024 <= b for t in range(0, 8192, 1024)) >= 2
    assert np.all(np.abs(np.array(m.ratios) - 1.0) > 1e-3)
    assert m.n_trace == list(range(len(m.codes)))                         # never reset
    # the cut form: runs of 1023, 1025, 2049 segments and the rest, equal to the whole
    mc = M.Model(kind, th, S.LONG_LENGTH, S.N_EST, 5000000, p_c=0.9, n_coeff=n_coeff)
    emitted, outs, pos = [], [], 0
    for n in S.segs_to_samples(kind, S.EDGE_CUT_SEGS) + [len(x)]:
        outs.append(mc.run(x[pos:pos + n]))
        emitted.append(len(outs[-1]) // S.LONG_LENGTH)
        pos += n
    assert tuple(emitted[:3]) == S.EDGE_CUT_SEGS and sum(emitted) == len(m.codes)
    assert np.array_equal(np.concatenate(outs).view(np.uint32), y.view(np.uint32)) and mc.codes == m.codes


def tile_kinds(n_trace, run_starts, n_est, n_reset, tile=1024):
    """(base within the run, absolute first segment, decided at once?) for every scan tile of every run."""
    out = []
    bounds = list(run_starts) + [len(n_trace)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        for base in range(0, b - a, tile):
            ln = min(tile, b - a - base)
            n = n_trace[a + base]
            out.append((base, a + base, ln, n, n >= n_est and n <= n_reset - ln))
    return out


@pytest.mark.parametrize("kind", [M.PULSE_BLANKING, M.NOTCH, M.NOTCH_LITE])
def test_reset_falls_among_the_tiles(kind):
    """From the model's n_segments trace: in one whole run tiles of both kinds occur past the first, and a reset with
    its new estimation window falls in a walked tile with base >= 2048.  In the cut form one run starts with n_segments
    == n_reset − nseg exactly (decided at once) and one with one more (walked)."""
    M.require_glibc()
    x, th, m, y = S.reset_case(kind)
    tr = m.n_trace
    tiles = tile_kinds(tr, [0], S.N_EST, S.RESET_N_RESET)
    past_first = [t for t in tiles if t[0] > 0]
    assert any(t[4] for t in past_first) and any(not t[4] for t in past_first)
    resets = [s for s in range(1, len(tr)) if tr[s] == 1 and tr[s - 1] > S.RESET_N_RESET]   # first segment of a new window
    assert len(resets) >= 2
    hit = 0
    for s in resets:
        base = (s // 1024) * 1024
        walked = not [t for t in tiles if t[0] == base][0][4]
        window = tr[s: s + S.N_EST - 1] == list(range(1, S.N_EST))
        if base >= 2048 and walked and window and base + 1024 >= s + S.N_EST:
            hit += 1
            assert all(c == 0 for c in m.codes[s - 1: s + S.N_EST - 1])          # the reset segment and the window are copied
    assert hit >= 1
    if kind != M.PULSE_BLANKING:
        assert np.all(np.abs(np.array(m.ratios) - 1.0) > 1e-3)
    c = np.bincount(np.array(m.codes), minlength=3)
    assert c[0] > 2000 and c[1] + c[2] > 4000
    # the cut form
    mc = M.Model(kind, th, S.LONG_LENGTH, S.N_EST, S.RESET_N_RESET, p_c=0.9, n_coeff=S.COV_N_COEFF)
    starts, outs, pos, sides = [], [], 0, []
    for n in S.segs_to_samples(kind, S.RESET_CUT_SEGS) + [len(x)]:
        n_before, seg0 = mc.n_segments, len(mc.codes)
        outs.append(mc.run(x[pos:pos + n]))
        nseg = len(mc.codes) - seg0
        starts.append(seg0)
        sides.append((n_before - (S.RESET_N_RESET - nseg), nseg))
        pos += n
    assert np.array_equal(np.concatenate(outs).view(np.uint32), y.view(np.uint32)) and mc.n_trace == tr
    assert [s[1] for s in sides[:4]] == list(S.RESET_CUT_SEGS)
    assert sides[1] == (1, 1000) and sides[3] == (0, 1000)                # one more, and exactly; both single tiles
    assert starts[2] in resets or starts[2] + 1 in resets                  # run 3 starts where the reset falls
    cut_tiles = tile_kinds(tr, starts, S.N_EST, S.RESET_N_RESET)
    assert [t[4] for t in cut_tiles if t[1] == starts[1]] == [False] and [t[4] for t in cut_tiles if t[1] == starts[3]] == [True]


@pytest.mark.parametrize("kind", [M.PULSE_BLANKING, M.NOTCH, M.NOTCH_LITE])
def test_leading_zeros_give_a_zero_or_floor_estimate(kind):
    M.require_glibc()
    x, th, m, y = S.leading_zeros_case(kind)
    L = S.ZERO_LENGTH
    assert not np.any(x[:3 * S.N_EST * L]) and np.any(x[3 * S.N_EST * L:])
    r = np.array(m.ratios)
    c = np.bincount(np.array(m.codes), minlength=3)
    if kind == M.PULSE_BLANKING:
        assert m.noise == 0.0
        assert np.isnan(r).sum() >= 2 * S.N_EST - 1 and np.isinf(r).sum() > 250   # 0/0 on the zeros, x/0 after them
        assert c[0] >= 3 * S.N_EST and c[1] > 250
        assert not np.any(y)                                                       # copies of zeros, then blanked
    else:
        assert 0.0 < float(m.noise) < 1e-20 and m.noise64 > 0.0
        assert np.all((r == 0.0) | (r > 1e6))
        assert c[0] >= 3 * S.N_EST - 1 and c[1] > 250 and c[2] == 1
        assert m.est_err < 1e-4


def test_coverage_estimate_tolerance_is_taken_over_the_new_streams():
    M.require_glibc()
    worst = max(m.est_err for m in S.cov_notch_models())
    print(f"largest float32-against-float64 error of the noise estimate over the coverage streams {worst:.3e}")
    assert 0.0 < worst < 1e-4
