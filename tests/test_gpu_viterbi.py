"""The device Viterbi decoder (vit_decoder.hip) against the compiled reference's recorded results
(tests/golden/viterbi_ref.npz) and against the model of tests/viterbi_model.py.

Contract: bit equality, no tolerance.  Reference mode: bits and the 64 carried metrics (state_get, compared as
words) equal the fixture for every case, whatever else shares the launch and wherever in a batch a frame sits;
reset_channel gives a new object; raw pages (interleaved, G2 inverted, possibly negated) equal the model fed the
prepared symbols.  Full mode equals the model's full mode and leaves the carried metrics alone.  What the conf
comments of include/gnsship.h exclude is E_INVAL and runs nothing."""
import numpy as np
import pytest

import viterbi_model as V
from viterbi_cases import FRAMES, KINDS, LENGTHS, case
from gnss_sim_receiver_amd import abi, engine

pytestmark = pytest.mark.gpu

CHANNELS = 600


def words(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def plain(ctx):
    """One reference-mode decoder per fixture length, no interleaver, no G2 flip: Viterbi_Decoder alone."""
    d = {LL: engine.ViterbiDecoder(ctx, CHANNELS, LL) for LL in LENGTHS}
    yield d
    for v in d.values():
        v.close()


def fresh(dec, channels):
    for c in channels:
        dec.reset_channel(int(c))


def noise_frames(n, frame, seed):
    """Frames of the fixture's rounded kind: multiples of 0.5, frequent ties."""
    rng = np.random.default_rng(seed)
    return (np.round(rng.standard_normal((n, frame)) * 2.0) / 2.0).astype(np.float32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("LL", LENGTHS)
def test_reference_mode_equals_the_reference(plain, LL, kind):
    sym, bits, sec, _ = case(LL, kind)
    dec = plain[LL]
    fresh(dec, [3])
    for f in range(FRAMES):  # one object's four calls: four runs on one channel
        got = dec.run(sym[f:f + 1], [3])
        assert np.array_equal(got[0], bits[f]), f"frame {f}: bits"
        assert np.array_equal(words(dec.state(3)), words(sec[f])), f"frame {f}: carried metrics"


@pytest.mark.parametrize("LL", LENGTHS)
def test_a_channel_among_256_others(plain, LL):
    """The same four frames, each sent in a batch of 257 with 256 other channels' frames around it."""
    sym, bits, sec, _ = case(LL, 2)
    dec = plain[LL]
    target, where = 77, (0, 130, 256, 5)
    fresh(dec, range(257))
    others = np.array([c for c in range(257) if c != target], np.int32)
    for f in range(FRAMES):
        batch = noise_frames(257, sym.shape[1], 100 + f)
        channels = np.insert(others, where[f], target)
        batch[where[f]] = sym[f]
        got = dec.run(batch, channels)
        assert np.array_equal(got[where[f]], bits[f]), f"frame {f}: bits"
        assert np.array_equal(words(dec.state(target)), words(sec[f])), f"frame {f}: carried metrics"


@pytest.mark.parametrize("LL", LENGTHS)
def test_a_frame_alone_equals_the_frame_in_a_batch(plain, LL):
    """Batches of 5 and 257 frames: not multiples of the frames a workgroup holds."""
    sym, bits, sec, _ = case(LL, 1)
    dec = plain[LL]
    fresh(dec, range(300))
    alone = dec.run(sym[:1], [0])[0]
    assert np.array_equal(alone, bits[0])
    first = 1
    for n in (5, 257):
        for pos in (0, n - 1):
            channels = np.arange(first, first + n, dtype=np.int32)
            batch = noise_frames(n, sym.shape[1], n + pos)
            batch[pos] = sym[0]
            fresh(dec, channels)
            got = dec.run(batch, channels)
            assert np.array_equal(got[pos], alone), (n, pos)
            assert np.array_equal(words(dec.state(int(channels[pos]))), words(sec[0])), (n, pos)
        # every other frame of the batch against the model, new objects all
        want, _ = V.decode_batch(batch, V.new_section(n))
        assert np.array_equal(got, want), n


def test_reset_channel_is_a_new_object(plain):
    sym, bits, sec, _ = case(114, 1)
    dec = plain[114]
    fresh(dec, [9])
    assert np.array_equal(words(dec.state(9)), words(V.new_section()))
    dec.run(sym[0:1], [9])
    dec.run(sym[1:2], [9])
    assert np.array_equal(words(dec.state(9)), words(sec[1]))
    carried = dec.run(sym[0:1], [9])[0]  # the first frame again on the carried metrics: the third call of an object
    m = V.ViterbiDecoder(114)
    for f in (0, 1):
        m.decode(sym[f])
    assert np.array_equal(carried, m.decode(sym[0])[0]) and np.array_equal(words(dec.state(9)), words(m.section))
    dec.reset_channel(9)
    assert np.array_equal(words(dec.state(9)), words(V.new_section()))
    assert np.array_equal(dec.run(sym[0:1], [9])[0], bits[0])
    assert np.array_equal(words(dec.state(9)), words(sec[0]))


@pytest.mark.parametrize("page,factory", [(V.INAV, "galileo_inav_page_decoder"), (V.FNAV, "galileo_fnav_page_decoder"),
                                          (V.CNAV, "galileo_cnav_page_decoder")])
def test_raw_pages_equal_the_model_on_prepared_symbols(ctx, page, factory):
    rows, cols, LL = page
    rng = np.random.default_rng(rows * cols)
    n, calls = 6, 2
    dec = getattr(engine, factory)(ctx, n)
    assert (dec.data_length, dec.frame_symbols) == (LL, rows * cols)
    sec = V.new_section(n)
    channels = np.array([4, 0, 5, 2, 1, 3], np.int32)
    negate = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    for call in range(calls):
        truth = rng.integers(0, 2, (n, LL)).astype(np.uint8)
        sym = np.stack([V.encode(b) for b in truth]) + 0.25 * rng.standard_normal((n, rows * cols))
        sym = (np.round(sym * 4.0) / 4.0).astype(np.float32)
        # the transmitter's side: invert G2's symbols, interleave (the de-interleaver's inverse), a 180° lock on some
        raw = V.deinterleave(cols, rows, V.g2_flip(sym))
        raw[negate != 0] = -raw[negate != 0]
        prepared = np.stack([V.prepare(raw[i], rows, cols, True, bool(negate[i])) for i in range(n)])
        assert np.array_equal(prepared, sym)
        s = sec[channels]  # fancy index: a copy, written back below
        want, _ = V.decode_batch(prepared, s)
        sec[channels] = s
        got = dec.run(raw, channels, negate)
        assert np.array_equal(got, want), call
        if call == 0:
            assert np.array_equal(got, truth)  # new objects at this noise: the pages decode
        for i, c in enumerate(channels):
            assert np.array_equal(words(dec.state(int(c))), words(sec[c])), (call, c)
    dec.close()


def test_the_smallest_trellis(ctx):
    """LL = 1: 7 steps, 14 symbols."""
    dec = engine.ViterbiDecoder(ctx, 7, 1)
    sec = V.new_section(7)
    for call in range(3):
        sym = noise_frames(7, 14, 40 + call)
        want, _ = V.decode_batch(sym, sec)
        got = dec.run(sym, np.arange(7))
        assert got.shape == (7, 1) and np.array_equal(got, want), call
        for c in range(7):
            assert np.array_equal(words(dec.state(c)), words(sec[c])), (call, c)
    dec.close()


def test_device_resident_input_and_output(ctx, plain):
    sym = np.ascontiguousarray(case(238, 1)[0])
    dec = plain[238]
    n, LL = FRAMES, 238
    fresh(dec, range(2 * n))
    host = dec.run(sym, np.arange(n))
    src = ctx.upload(sym)
    dst = engine.DeviceBuffer(ctx, n * LL)
    assert dec.run(src.ptr, np.arange(n, 2 * n), on_device=True, bits_dev=dst.ptr, host=False) is None
    got = dst.download(np.zeros((n, LL), np.uint8))
    assert np.array_equal(got, host)
    for c in range(n):
        assert np.array_equal(words(dec.state(n + c)), words(dec.state(c)))
    # both at once: bits_dev and the host copy
    fresh(dec, range(n))
    both = dec.run(src.ptr, np.arange(n), on_device=True, bits_dev=dst.ptr, host=True)
    assert np.array_equal(both, host) and np.array_equal(dst.download(np.zeros((n, LL), np.uint8)), host)
    src.free()
    dst.free()


@pytest.mark.parametrize("LL", LENGTHS)
def test_full_mode_equals_the_model(ctx, LL):
    sym, bits, _, truth = case(LL, 1)
    dec = engine.ViterbiDecoder(ctx, 8, LL, mode="full")
    before = [dec.state(c) for c in (0, 5)]
    want, _ = V.decode_batch(sym, V.new_section(FRAMES), V.FULL)
    got = dec.run(sym, [5, 5, 0, 5])  # nothing is carried: a channel may appear again
    assert np.array_equal(got, want)
    assert np.array_equal(got, truth) and np.count_nonzero(bits != truth) > 0
    ties = np.concatenate([case(LL, 2)[0], case(LL, 3)[0]])
    want, _ = V.decode_batch(ties, V.new_section(len(ties)), V.FULL)
    assert np.array_equal(dec.run(ties, np.zeros(len(ties), np.int32)), want)
    for c, b in zip((0, 5), before):
        assert np.array_equal(words(dec.state(c)), words(b)) and np.array_equal(words(b), words(V.new_section()))
    dec.close()


def test_rejected_calls(ctx, plain):
    def refused(f):
        with pytest.raises(abi.GnssHipError) as e:
            f()
        assert e.value.code == abi.E_INVAL, e.value
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, 8, 31))            # rows·cols != 2·(LL + 6)
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, 8, 0))
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, constraint_length=9))
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, rate_n=3))
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 507))                   # 1026 symbols
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 0))
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, g=(128, 91)))
    refused(lambda: engine.ViterbiDecoder(ctx, 4, 114, mode=2))
    refused(lambda: engine.ViterbiDecoder(ctx, 0, 114))
    engine.ViterbiDecoder(ctx, 1, 506).close()                            # 1024 symbols: the limit itself
    dec = plain[114]
    sym = case(114, 0)[0]
    fresh(dec, [0, 1, 2])
    dec.run(sym[:1], [1])
    before = [dec.state(c) for c in (0, 1, 2)]
    refused(lambda: dec.run(sym[:3], [0, 1, 0]))                          # a channel twice in reference mode
    refused(lambda: dec.run(sym[:2], [0, CHANNELS]))                      # channel out of range
    refused(lambda: dec.run(sym[:2], [-1, 0]))
    refused(lambda: dec.reset_channel(CHANNELS))
    refused(lambda: dec.state(-1))
    for c, b in zip((0, 1, 2), before):                                   # nothing ran
        assert np.array_equal(words(dec.state(c)), words(b))
    assert np.array_equal(dec.run(sym[1:2], [1])[0], case(114, 0)[1][1])  # and the channel goes on as if never asked
