"""The acquisition resampler's coverage table (tests/acq_resampler_cases.py) on its own, no GPU: the tile and LDS
annotations recomputed from the formula of gnsship_acq_resampler_create, the classes the table must keep (a later
change to the list cannot drop one silently), the stream and call pattern of every shape, and the teeth of the
asymmetric taps: the oracle fed the reversed taps differs from the oracle fed the right ones on the test stream."""
import numpy as np
import pytest

import acq_resampler_cases as C
from gnss_sim_receiver_amd import abi, engine
from oracle import oracle as O


def test_table_annotations_match_the_formula():
    for t, d, opb, lds in C.SHAPE_TABLE:
        assert 1 <= t <= 4096 and d >= 1
        assert (C.opb_of(t, d), C.lds_bytes(t, d)) == (opb, lds), (t, d)
        span = (opb - 1) * d + t
        assert span <= 8192 and lds == 8 * ((t + 1) // 2 + span)


def test_table_keeps_every_class():
    opbs = {C.opb_of(t, d) for t, d in C.SHAPES}
    assert 1 in opbs and 2 in opbs and 256 in opbs and any(2 < o < 256 for o in opbs)
    lds = [C.lds_bytes(t, d) for t, d in C.SHAPES]
    assert min(lds) < 65536 < max(lds) and max(lds) == 81920  # 81 920: the largest an API-valid shape reaches
    assert sum(b > 65536 for b in lds) >= 5
    assert any((C.opb_of(t, d) - 1) * d + t == 8192 for t, d in C.SHAPES)       # a span of exactly 8192
    assert sum(t == 1 for t, d in C.SHAPES) >= 2                               # no history kernel
    assert any(t % 2 == 0 and t < 10 for t, d in C.SHAPES)                     # even taps, padded
    assert any(t == 4096 for t, d in C.SHAPES) and any(t == 4095 for t, d in C.SHAPES)
    # all three formats for opb = 1, n_taps = 1 and the two largest LDS figures; one device-pointer run
    for shape in C.SHAPES:
        if C.opb_of(*shape) == 1 or shape[0] == 1:
            assert shape in C.ALL_FORMATS, shape
    top = sorted(set(lds), reverse=True)[:2]
    assert {C.lds_bytes(*s) for s in C.ALL_FORMATS} >= set(top)
    assert C.DEVICE_INPUT[0] in C.SHAPES
    used = {fmt for _, _, _, fmt in C.cases()}
    assert used == set(C.FORMATS)


def test_automatic_designs_have_the_annotated_shapes(built):
    lib = abi.load()
    for key in C.DESIGNS:
        d, taps = engine.acq_resampler_design(lib, *key)
        t, d_want, opb, lds = C.DESIGN_SHAPES[key]
        assert (len(taps), d) == (t, d_want)
        assert (C.opb_of(t, d), C.lds_bytes(t, d)) == (opb, lds)
        assert opb < 256 and lds > 65536
        d_o, taps_o = O.acq_resampler_design(*key)
        assert d_o == d and np.array_equal(taps_o, taps)


@pytest.mark.parametrize("t,d", C.SHAPES + [v[:2] for v in C.DESIGN_SHAPES.values()])
def test_stream_and_calls_of_every_shape(t, d):
    opb, nk = C.opb_of(t, d), C.n_outputs(t, d)
    assert d * nk <= C.MAX_SAMPLES
    tiles = -(-nk // opb)
    assert tiles >= 3
    if opb > 1:
        assert nk % opb != 0                                 # the last tile is partial
    cuts = C.cuts(d, nk)
    lens = np.diff(cuts)
    assert list(lens[:3]) == [d, d, 7 * d] and lens[3] >= d and cuts[-1] == d * nk
    assert (lens // d == 1).sum() >= 1                       # a call with a single output
    if t - 1 > d:
        assert lens[0] < t - 1 and lens[1] < t - 1           # two successive calls shorter than the history
    assert nk >= 10                                          # the run after the reset has its 10·D samples


@pytest.mark.parametrize("name,t,d,fmt", [c for c in C.cases() if c[1] > 1], ids=[c[0] for c in C.cases() if c[1] > 1])
def test_reversed_taps_change_the_oracle_output(built, name, t, d, fmt):
    taps = C.asymmetric_taps(t)
    assert taps.dtype == np.float32 and len(taps) == t
    assert not np.array_equal(taps, taps[::-1])
    nk = C.n_outputs(t, d)
    _, x = C.stream(fmt, d * nk, seed=t + d)
    right = O.FirDecimator(taps, d)(x)
    wrong = O.FirDecimator(taps[::-1].copy(), d)(x)
    assert np.all(np.isfinite(right.view(np.float32)))
    # not in one sample only: most outputs differ, in every call of the pattern
    differ = right != wrong
    assert differ.mean() > 0.9
    for a, b in zip(C.cuts(d, nk)[:-1], C.cuts(d, nk)[1:]):
        assert differ[a // d: b // d].any()
