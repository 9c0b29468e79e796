"""Interference mitigation on the GPU (mit_filter.hip) where tests/test_gpu_mit.py does not reach, against the model of
tests/mit_model.py; the streams are the coverage scenarios of tests/mit_scenarios.py, whose conditions
tests/test_mit_model.py asserts on the model alone.

Contract, the existing one: output and counters bit-equal to the model; pulse blanking's noise estimate bit-equal; the
notches' estimate within four times the model's own float32-against-float64 error, taken over the new streams.

* segment lengths 2, 13, 255, 257: mit_chain without a whole group of 8, with groups and a remainder; one below and
  one above the 256-lane strides of the DFT and the LDS loads; both chain forms at 13 and 257;
* runs of filtered segments on the edges of the scan's tiles of 1024, the stream whole and in runs of 1023, 1025, 2049
  segments and the rest;
* a reset and a new estimation window in a tile with base > 0 (the single-lane walk and the workgroup's estimation
  there), and the two sides of the scan's decision to take a tile at once;
* a device input 64 bytes inside a buffer and a caller's destination inside a larger one;
* a stream that starts with zeros: a noise estimate of 0, ratios 0/0 and x/0."""
import numpy as np
import pytest

import mit_model as M
import mit_scenarios as S
from gnss_sim_receiver_amd import engine
from test_gpu_mit import KIND_NAMES, bits, same_counters

pytestmark = pytest.mark.gpu

KINDS = [M.PULSE_BLANKING, M.NOTCH, M.NOTCH_LITE]


def estimate_tolerance():
    """Four times the largest relative error the model's float32 estimate shows against its float64 one over the new
    notch streams."""
    return 4.0 * max(m.est_err for m in S.cov_notch_models())


def check_estimate(st, m, kind, what):
    if kind == M.PULSE_BLANKING:
        assert np.float32(st["noise_power"]).tobytes() == m.noise.tobytes()
        return
    tol = estimate_tolerance()
    err = abs(st["noise_power"] - m.noise64) / m.noise64
    print(f"{what}: device noise estimate against the float64 model, relative error {err:.3e} (allowed {tol:.3e})")
    assert err <= tol


def run_in(f, x, lengths):
    """The stream in runs of the given sample counts and the rest; (output, emitted samples per run)."""
    outs, pos = [], 0
    for n in list(lengths) + [len(x)]:
        outs.append(f.run(x[pos:pos + n]))
        pos = min(pos + n, len(x))
    return np.concatenate(outs), [len(o) for o in outs]


@pytest.mark.parametrize("length", S.COV_LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_lengths_beside_the_strides(ctx, kind, length):
    M.require_glibc()
    x, th, m, y = S.cov_length_case(kind, length)
    c = np.array(m.codes)
    assert np.any(c == 0) and np.any(c != 0)
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=length, n_segments_est=S.N_EST,
                                      n_segments_reset=S.N_RESET, n_segments_coeff=S.COV_N_COEFF)
    out, _ = run_in(f, x, [S.run_cut_sample(length, len(x))])   # the cut falls inside a filtered run of the notches
    st = f.state()
    f.close()
    assert np.array_equal(bits(out), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    check_estimate(st, m, kind, f"kind {kind} length {length}")


@pytest.mark.parametrize("p_c", [0.9, 1.0])
@pytest.mark.parametrize("length", S.COV_CHAIN_LENGTHS)
def test_chain_forms_at_lengths_13_and_257(ctx, length, p_c):
    M.require_glibc()
    th = S.cov_notch_thres(length)
    xs = S.cw_continuous(S.CHAIN_N, S.CHAIN_SEED)
    outs, states = {}, {}
    for form in ("serial", "speculative"):
        f = engine.InterferenceMitigation(ctx, "notch", S.CHAIN_N, threshold=th, p_c_factor=p_c, length=length, n_segments_est=S.N_EST,
                                          n_segments_reset=5000000, chain_form=form)
        outs[form] = f.run(xs)
        states[form] = f.state()
        f.close()
    sp = states["speculative"]
    assert (sp["chunk_samples"], sp["warmup_samples"]) == S.chain_geometry(p_c, length)
    x, th, m, y = S.cov_chain_case(length, p_c, sp["chunk_samples"], sp["warmup_samples"])
    print(f"length {length} p_c {p_c}: chunk {sp['chunk_samples']} warm-up {sp['warmup_samples']} speculated {sp['chunks_speculated']} "
          f"replayed {sp['chunks_replayed']} (model {m.chunks_speculated}, {m.chunks_replayed})")
    assert np.array_equal(bits(outs["serial"]), bits(y))
    assert np.array_equal(bits(outs["speculative"]), bits(y))
    assert states["serial"]["chunks_speculated"] == 0 and states["serial"]["chunks_replayed"] == 0
    assert sp["chunks_speculated"] == m.chunks_speculated and sp["chunks_replayed"] == m.chunks_replayed
    assert sp["chunks_speculated"] > 0 and (sp["chunks_replayed"] == 0) == (p_c == 0.9)
    same_counters(sp, m)


@pytest.mark.parametrize("which", sorted(S.EDGE_RUNS))
@pytest.mark.parametrize("kind,n_coeff", [(M.PULSE_BLANKING, 1), (M.NOTCH, 1), (M.NOTCH_LITE, 3), (M.NOTCH_LITE, 5000)])
def test_runs_on_the_tile_edges(ctx, kind, n_coeff, which):
    M.require_glibc()
    x, th, m, y = S.edge_case(kind, n_coeff, which)
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=S.LONG_LENGTH, n_segments_est=S.N_EST,
                                      n_segments_reset=5000000, n_segments_coeff=n_coeff)
    whole = f.run(x)
    st = f.state()
    assert np.array_equal(bits(whole), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    check_estimate(st, m, kind, f"kind {kind} edges {which}")
    f.reset()
    out, emitted = run_in(f, x, S.segs_to_samples(kind, S.EDGE_CUT_SEGS))
    st = f.state()
    f.close()
    assert tuple(n // S.LONG_LENGTH for n in emitted[:3]) == S.EDGE_CUT_SEGS
    assert np.array_equal(bits(out), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)


@pytest.mark.parametrize("kind", KINDS)
def test_reset_among_the_tiles(ctx, kind):
    M.require_glibc()
    x, th, m, y = S.reset_case(kind)
    assert m.n_trace.count(1) >= 2
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=S.LONG_LENGTH, n_segments_est=S.N_EST,
                                      n_segments_reset=S.RESET_N_RESET, n_segments_coeff=S.COV_N_COEFF)
    whole = f.run(x)
    st = f.state()
    assert np.array_equal(bits(whole), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    check_estimate(st, m, kind, f"kind {kind} reset among tiles")
    # the two sides of the decision to take a tile at once: runs that start with n_segments = n_reset − nseg + 1 and
    # n_reset − nseg (tests/test_mit_model.py::test_reset_falls_among_the_tiles)
    f.reset()
    outs, pos, before = [], 0, []
    for n in S.segs_to_samples(kind, S.RESET_CUT_SEGS) + [len(x)]:
        before.append(f.state()["n_segments"])
        outs.append(f.run(x[pos:pos + n]))
        pos += n
    st = f.state()
    f.close()
    assert [len(o) // S.LONG_LENGTH for o in outs[:4]] == list(S.RESET_CUT_SEGS)
    assert before[1] == S.RESET_N_RESET - 1000 + 1 and before[3] == S.RESET_N_RESET - 1000
    assert np.array_equal(bits(np.concatenate(outs)), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    check_estimate(st, m, kind, f"kind {kind} reset among tiles, cut")


@pytest.mark.parametrize("kind", [M.NOTCH, M.PULSE_BLANKING])
def test_device_input_and_callers_destination(ctx, kind):
    """The input read from a pointer 64 bytes inside a device buffer, the output written inside a larger buffer of the
    caller's: equal to the host path, the words before and after the emitted samples untouched."""
    M.require_glibc()
    L = 32
    x, th, m, y = S.pulse_case(L) if kind == M.PULSE_BLANKING else S.notch_case(kind, L)
    n = len(x)
    cut = S.run_cut_sample(L, n)
    kw = dict(threshold=th, p_c_factor=0.9, length=L, n_segments_est=S.N_EST, n_segments_reset=S.N_RESET)
    host = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], n, **kw)
    want, emitted = run_in(host, x, [cut])
    want_state = host.state()
    host.close()
    assert np.array_equal(bits(want), bits(y)) and emitted[0] > 0 and emitted[1] > 0
    src = engine.DeviceBuffer(ctx, 64 + x.nbytes)
    src.upload(np.concatenate([np.full(64, 0xA5, np.uint8), x.view(np.uint8)]))
    lead, tail = 24, 40                                   # complex samples of pattern around the destination
    pattern = np.full(2 * (lead + n + tail), 0xDEADBEEF, np.uint32)
    dst = engine.DeviceBuffer(ctx, pattern.nbytes)
    dst.upload(pattern)
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], n, **kw)
    done = 0
    for a, b in ((0, cut), (cut, n)):
        where = dst.ptr + 8 * (lead + done)
        ptr, n_out = f.run(src.ptr + 64 + 8 * a, on_device=True, n_in=b - a, dev_dst=where)
        assert ptr == where and n_out == emitted[0 if a == 0 else 1]
        done += n_out
    ctx.sync()
    st = f.state()
    f.close()
    got = dst.download(np.empty_like(pattern))
    src.free()
    dst.free()
    assert done == len(want)
    assert np.all(got[: 2 * lead] == 0xDEADBEEF) and np.all(got[2 * (lead + done):] == 0xDEADBEEF)
    assert np.array_equal(got[2 * lead: 2 * (lead + done)], bits(want))
    assert st == want_state


@pytest.mark.parametrize("kind", KINDS)
def test_stream_that_starts_with_zeros(ctx, kind):
    M.require_glibc()
    x, th, m, y = S.leading_zeros_case(kind)
    f = engine.InterferenceMitigation(ctx, KIND_NAMES[kind], len(x), threshold=th, p_c_factor=0.9, length=S.ZERO_LENGTH, n_segments_est=S.N_EST,
                                      n_segments_reset=S.N_RESET, n_segments_coeff=S.COV_N_COEFF)
    out, _ = run_in(f, x, [S.N_EST * S.ZERO_LENGTH + 5])     # a cut inside the zeros, after the estimate is made
    st = f.state()
    f.close()
    assert np.array_equal(bits(out), bits(y))
    same_counters(st, m, lite=kind == M.NOTCH_LITE)
    check_estimate(st, m, kind, f"kind {kind} leading zeros")
