"""Interference mitigation on the GPU (mit_filter.hip) against the model of tests/mit_model.py
(pulse_blanking_cc.cc:57-98, notch_cc.cc:63-121, notch_lite_cc.cc:71-138 restated on the stream).

Contract: output, counters and (pulse blanking) the noise estimate bit-equal to the model; the notches' noise
estimate within four times the model's own float32-against-float64 error over the test streams; the serial and
speculative chain forms bit-equal, with the replay count the model predicts; the same stream cut into runs
anywhere bit-identical to one run; every rejected call leaves output and state untouched.
"""
import numpy as np
import pytest

import mit_model as M
import mit_scenarios as S
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

COUNTERS = ("n_segments", "filter_state", "samples_in", "samples_out", "pending_samples")
KIND_NAMES = {M.PULSE_BLANKING: "pulse-blanking", M.NOTCH: "notch", M.NOTCH_LITE: "notch-lite"}


def bits(y):
    return np.ascontiguousarray(y, np.complex64).view(np.uint32)


def same_counters(st, m, lite=False):
    ms = m.state()
    keys = COUNTERS + (("n_segments_coeff",) if lite else ())
    assert {k: st[k] for k in keys} == {k: ms[k] for k in keys}


def estimate_tolerance():
    """Four times the largest relative error the model's float32 estimate shows against its float64 one over the
    notch test streams."""
    worst = max(S.notch_case(k, L)[2].est_err for k in (M.NOTCH, M.NOTCH_LITE) for L in S.LENGTHS)
    return 4.0 * worst


@pytest.mark.parametrize("length", S.LENGTHS)
def test_pulse_blanking_matches_the_model(ctx, length):
    x, th, m, y = S.pulse_case(length)
    f = engine.InterferenceMitigation(ctx, "pulse-blanking", len(x), threshold=th, length=length, n_segments_est=S.N_EST,
                                      n_segments_reset=S.N_RESET)
    assert len(f.run(x[:length - 1])) == 0 and f.state()["pending_samples"] == length - 1  # shorter than one segment
    out = f.run(x[length - 1:])
    st = f.state()
    f.close()
    assert np.array_equal(bits(out), bits(y))
    assert np.float32(st["noise_power"]).tobytes() == m.noise.tobytes()
    same_counters(st, m)
    c = np.array(m.codes)
    assert np.any(c == 1) and np.any(c == 0)


@pytest.mark.parametrize("length", S.LENGTHS)
@pytest.mark.parametrize("kind,n_coeff", [(M.NOTCH, 1), (M.NOTCH_LITE, 1), (M.NOTCH_LITE, 3)])
def test_notch_matches_the_model(ctx, kind, n_coeff, length):
    M.require_glibc()
    x, th, m, y = S.notch_case(kind, length, n_coeff)
    tol = estimate_tolerance()
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=length,
                                      n_segments_est=S.N_EST, n_segments_reset=S.N_RESET, n_segments_coeff=n_coeff)
    scale = min(1.0, (len(x) / length) / 300.0)
    cut = int(S.RUN_CUT_SEG * scale * length)  # inside a tone span: the run boundary falls in a filtered run
    out = np.concatenate([f.run(x[:cut]), f.run(x[cut:])])
    st = f.state()
    f.close()
    err = abs(st["noise_power"] - m.noise64) / m.noise64
    print(f"kind {kind} length {length}: device noise estimate against the float64 model, relative error {err:.3e} (allowed {tol:.3e})")
    assert np.array_equal(bits(out), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    assert err <= tol


@pytest.mark.parametrize("kind,n_coeff", [(M.NOTCH, 1), (M.NOTCH_LITE, 1), (M.NOTCH_LITE, 3), (M.NOTCH_LITE, 5000)])
def test_tiles_decided_at_once_match_the_model(ctx, kind, n_coeff):
    """8192 segments with the reset out of reach: every scan tile past the first is decided by all lanes at once, the
    lite form's z0 in force included (runs that start in a tile, are carried into it, and span several)."""
    M.require_glibc()
    x, th, m, y = S.long_case(kind, n_coeff)
    r = np.array(m.ratios)
    assert np.all(np.abs(r - 1.0) > 1e-3)
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=S.LONG_LENGTH,
                                      n_segments_est=S.N_EST, n_segments_reset=5000000, n_segments_coeff=n_coeff)
    cut = S.LONG_LENGTH * 1324 + 3  # inside a filtered run, inside a tile
    out = np.concatenate([f.run(x[:cut]), f.run(x[cut:])])
    st = f.state()
    f.close()
    assert np.array_equal(bits(out), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)


@pytest.mark.parametrize("p_c", [0.9, 1.0])
def test_chain_forms_agree_and_replay_as_predicted(ctx, p_c):
    M.require_glibc()
    outs, states = {}, {}
    for form in ("serial", "speculative"):
        f = engine.InterferenceMitigation(ctx, "notch", S.CHAIN_N, threshold=S.thres_pfa(0.001, 32), p_c_factor=p_c, length=32,
                                          n_segments_est=S.N_EST, n_segments_reset=5000000, chain_form=form)
        outs[form] = f.run(S.cw_continuous(S.CHAIN_N, S.CHAIN_SEED))
        states[form] = f.state()
        f.close()
    sp = states["speculative"]
    assert (sp["chunk_samples"], sp["warmup_samples"]) == S.chain_geometry(p_c)
    x, th, m, y = S.chain_case(p_c, sp["chunk_samples"], sp["warmup_samples"])
    print(f"p_c {p_c}: chunk {sp['chunk_samples']} warm-up {sp['warmup_samples']} speculated {sp['chunks_speculated']} "
          f"replayed {sp['chunks_replayed']} (model {m.chunks_speculated}, {m.chunks_replayed})")
    assert np.array_equal(bits(outs["serial"]), bits(y))
    assert np.array_equal(bits(outs["speculative"]), bits(y))
    assert states["serial"]["chunks_speculated"] == 0 and states["serial"]["chunks_replayed"] == 0
    assert sp["chunks_speculated"] == m.chunks_speculated and sp["chunks_replayed"] == m.chunks_replayed
    if p_c == 0.9:
        assert sp["chunks_speculated"] >= 20 and sp["chunks_replayed"] == 0
    else:
        assert sp["chunks_replayed"] > 0


def make(ctx, kind, length, th, n_max, form="auto"):
    return engine.InterferenceMitigation(ctx, KIND_NAMES[kind], n_max, threshold=th, p_c_factor=0.9, length=length, n_segments_est=S.N_EST,
                                         n_segments_reset=S.N_RESET, n_segments_coeff=3, chain_form=form)


@pytest.mark.parametrize("kind,form", [(M.PULSE_BLANKING, "auto"), (M.NOTCH, "serial"), (M.NOTCH, "speculative"),
                                       (M.NOTCH_LITE, "serial"), (M.NOTCH_LITE, "speculative")])
def test_cut_invariance(ctx, kind, form):
    length = 32
    if kind == M.PULSE_BLANKING:
        x, th = S.pulsed(length), S.thres_pfa(0.04, length)
    else:
        x, th = S.cw_gated(length, S.NOTCH_SEEDS[(kind, length)]), S.notch_thres(length)
    f = make(ctx, kind, length, th, len(x), form)
    whole = f.run(x)
    st_whole = f.state()
    # cut everywhere the issue names, one sample at a time over three segments, then inside a filtered run
    cuts = [1, length - 1, length, length + 1, 7 * length + 3, 0] + [1] * (3 * length)
    cuts.append(int(S.RUN_CUT_SEG * length) - sum(cuts))
    f.reset()
    outs, pos = [], 0
    for n in cuts + [len(x)]:
        outs.append(f.run(x[pos:pos + n]))
        pos = min(pos + n, len(x))
    st_cut = f.state()
    assert np.array_equal(bits(np.concatenate(outs)), bits(whole))
    for k in st_whole:
        if k not in ("chunks_speculated", "chunks_replayed"):
            assert st_whole[k] == st_cut[k] or (k == "noise_power" and np.float32(st_whole[k]).tobytes() == np.float32(st_cut[k]).tobytes()), k
    # a reset in the filter state, then a fresh stream: as a new block
    f.reset()
    on = int(225 * length)
    f.run(x[:on + 5 * length])
    if kind != M.PULSE_BLANKING:
        assert f.state()["filter_state"] == 1
    f.reset()
    st0 = f.state()
    assert (st0["n_segments"], st0["filter_state"], st0["samples_in"], st0["samples_out"], st0["pending_samples"], st0["noise_power"]) == (0, 0, 0, 0, 0, 0.0)
    again = f.run(x)
    f.close()
    assert np.array_equal(bits(again), bits(whole))


@pytest.mark.parametrize("kind", [M.PULSE_BLANKING, M.NOTCH, M.NOTCH_LITE])
def test_rejected_calls_leave_output_and_state_untouched(ctx, kind):
    length = 32
    name = KIND_NAMES[kind]
    for bad in (dict(length=1), dict(length=1025), dict(n_segments_est=0), dict(pfa=0.0), dict(pfa=1.0), dict(max_in=0)):
        kw = dict(pfa=0.01, length=length, n_segments_est=S.N_EST, n_segments_reset=S.N_RESET)
        kw.update({k: v for k, v in bad.items() if k != "max_in"})
        with pytest.raises(abi.GnssHipError) as e:
            engine.InterferenceMitigation(ctx, name, bad.get("max_in", 1024), **kw)
        assert e.value.code == abi.E_INVAL and "gnsship_mit_create" in str(e.value)
    if kind == M.NOTCH_LITE:
        with pytest.raises(abi.GnssHipError):
            engine.InterferenceMitigation(ctx, name, 1024, pfa=0.01, length=length, n_segments_coeff=0)
    # an explicit threshold overrides a pfa that would be rejected
    engine.InterferenceMitigation(ctx, name, 1024, pfa=0.0, threshold=50.0, length=length).close()
    x = S.pulsed(length) if kind == M.PULSE_BLANKING else S.cw_gated(length, S.NOTCH_SEEDS[(kind, length)])
    n = 4096
    th = S.thres_pfa(0.04, length) if kind == M.PULSE_BLANKING else S.notch_thres(length)
    ref = make(ctx, kind, length, th, n)
    want = np.concatenate([ref.run(x[:n - 7]), ref.run(x[n - 7:2 * n - 7])])
    want_state = ref.state()
    ref.close()
    f = make(ctx, kind, length, th, n)
    first = f.run(x[:n - 7])
    dev, n_out = f.last_dev
    before = f.state()
    with pytest.raises(abi.GnssHipError) as e:
        f.run(x[:n + 1])  # n_in > max_in_samples
    assert e.value.code == abi.E_INVAL and "max_in_samples" in str(e.value)
    assert f.state() == before
    kept = np.zeros(n_out, np.complex64)
    ctx.lib.gnsship_dev_download(ctx.h, kept.ctypes.data, dev, kept.nbytes)
    assert np.array_equal(bits(kept), bits(first))
    got = np.concatenate([first, f.run(x[n - 7:2 * n - 7])])
    assert np.array_equal(bits(got), bits(want)) and f.state() == want_state
    f.close()
