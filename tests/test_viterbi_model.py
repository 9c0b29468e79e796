"""tests/viterbi_model.py against the compiled reference (tests/golden/viterbi_ref.npz, made by
tests/golden/make_viterbi_golden.py from telemetry_decoder/libs/viterbi_decoder.cc): bits and the 64 carried
metrics of every call equal bit for bit, no traceback of a fixture frame visits an entry nothing stored (the one
case the model does not restate), and what the reference's metric costs: full mode decodes the sigma 0.6 frames
without error, the reference does not."""
import numpy as np
import pytest

import viterbi_model as V
from viterbi_cases import FRAMES, KINDS, LENGTHS, case, golden

CASES = [(LL, k) for LL in LENGTHS for k in KINDS]


def test_fixture_is_the_one_the_issue_describes():
    g = golden()
    assert tuple(g["lengths"]) == (114, 238, 486) and tuple(g["kinds"]) == (0, 1, 2, 3) and tuple(g["g"]) == V.G_GALILEO
    for LL, k in CASES:
        sym, bits, sec, _ = case(LL, k)
        assert sym.shape == (FRAMES, 2 * (LL + 6)) and sym.dtype == np.float32
        assert bits.shape == (FRAMES, LL) and sec.shape == (FRAMES, 64) and sec.dtype == np.float32
    sym = case(114, 2)[0]
    assert np.array_equal(sym, np.round(sym * 2) / 2)  # multiples of 0.5
    sym = case(114, 3)[0]
    assert not np.any(sym[0::2]) and np.all(np.any(sym[1::2] != 0, axis=1))


@pytest.mark.parametrize("LL,kind", CASES)
def test_model_equals_the_reference(LL, kind):
    sym, bits, sec, _ = case(LL, kind)
    d = V.ViterbiDecoder(LL)
    for f in range(FRAMES):
        got, unstored = d.decode(sym[f])
        assert not unstored, f"frame {f}: the traceback visited an entry nothing stored"
        assert np.array_equal(got, bits[f]), f"frame {f}: bits"
        assert np.array_equal(d.section.view(np.uint32), sec[f].view(np.uint32)), f"frame {f}: section words"


def test_the_batched_model_is_the_object_model():
    sym = case(114, 1)[0]
    d = V.ViterbiDecoder(114)
    one = d.decode(sym[0])[0]
    sec = V.new_section(3)
    many, _ = V.decode_batch(np.stack([sym[0], sym[1], sym[0]]), sec)
    assert np.array_equal(many[0], one) and np.array_equal(many[2], one)
    assert np.array_equal(sec[0].view(np.uint32), d.section.view(np.uint32))


@pytest.mark.parametrize("LL", LENGTHS)
def test_full_mode_decodes_what_the_reference_cannot(LL):
    sym, bits, _, truth = case(LL, 1)  # sigma 0.6
    full, _ = V.decode_batch(sym, V.new_section(FRAMES), V.FULL)
    assert np.array_equal(full, truth)
    assert np.count_nonzero(bits != truth) > 0
    # at sigma 0.3 neither has an error
    sym, bits, _, truth = case(LL, 0)
    full, _ = V.decode_batch(sym, V.new_section(FRAMES), V.FULL)
    assert np.array_equal(full, truth) and np.array_equal(bits, truth)


def test_full_mode_carries_nothing():
    sym = case(114, 1)[0]
    sec = V.new_section(1)
    sec[0, 5] = np.float32(3.0)
    before = sec.copy()
    a, _ = V.decode_batch(sym[:1], sec, V.FULL)
    assert np.array_equal(sec, before)
    d = V.ViterbiDecoder(114, mode=V.FULL)
    assert np.array_equal(d.decode(sym[1])[0], d.decode(sym[1])[0])
    assert np.array_equal(a[0], V.ViterbiDecoder(114, mode=V.FULL).decode(sym[0])[0])


def test_prepare_restates_the_block():
    rng = np.random.default_rng(3)
    for rows, cols, LL in (V.INAV, V.FNAV, V.CNAV):
        assert rows * cols == 2 * (LL + 6)
        x = rng.standard_normal(rows * cols).astype(np.float32)
        out = np.zeros_like(x)
        for r in range(rows):  # :344-350
            for c in range(cols):
                out[c * rows + r] = x[r * cols + c]
        assert np.array_equal(V.deinterleave(rows, cols, x), out)
        for i in range(out.size):  # :362-368
            if (i + 1) % 2 == 0:
                out[i] = -out[i]
        assert np.array_equal(V.prepare(x, rows, cols, True, False), out)
        assert np.array_equal(V.prepare(x, rows, cols, True, True), -out)


def test_encoder_and_trellis_agree():
    rng = np.random.default_rng(4)
    b = rng.integers(0, 2, 40).astype(np.uint8)
    s = V.encode(b)
    assert s.shape == (92,) and set(np.unique(s)) <= {-1.0, 1.0}
    got, unstored = V.ViterbiDecoder(40, mode=V.FULL).decode(s)
    assert np.array_equal(got, b)
