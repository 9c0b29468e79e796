"""The numpy restatement of the Galileo telemetry framing (tests/tlm_model.py): CRC-24Q against its published check
value, the frame-sync machine, page handling and the sticky I/NAV CRC flag on noiseless built streams (CPU only)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import tlm_model as M  # noqa: E402

FRAME_TYPES = [M.INAV, M.FNAV, M.CNAV]
LEAD = 37


def test_crc24q_check_value():
    assert M.crc24q_bytes(b"123456789") == 0xCDE703


@pytest.mark.parametrize("n", [196, 214, 462])
def test_crc24q_table_xor_equals_bitwise(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        bits = rng.integers(0, 2, n)
        assert M.crc24q_table_xor(bits) == M.crc24q_bits(bits)
    assert M.crc24q_table_xor(np.zeros(n, np.int64)) == 0 == M.crc24q_bits(np.zeros(n, np.int64))


def _stream(ft, n_parts, lead=LEAD, seed=5):
    """A stream on which n_parts parts are emitted, and the four parts it cycles."""
    g = M.GEOMETRY[ft]
    parts = M.four_parts(ft, seed)
    n = lead + g.required + 1 + (2 + n_parts - 1) * g.period + 5
    return M.build_stream(ft, parts, n, lead, seed + 1), parts


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("ft", FRAME_TYPES)
def test_model_on_built_stream(ft, sign):
    g = M.GEOMETRY[ft]
    x, parts = _stream(ft, 4)
    d = M.TlmDecoder(ft)
    pages, fault = d.run(np.float32(sign) * x)
    assert not fault and len(pages) == 4
    # the preamble is found at the oldest end of a full history, then confirmed one period later, then a part falls due
    assert [p["symbol_counter"] for p in pages] == [LEAD + g.required + 1 + (2 + k) * g.period for k in range(4)]
    # the first part emitted is the stream's third: the two before it went by while the history filled
    for k, p in enumerate(pages):
        assert np.array_equal(p["bits"], parts[(2 + k) % 4]), k
        assert bool(p["flags"] & M.F_PLL_180) == (sign < 0)
    ok = [bool(p["flags"] & M.F_CRC_OK) for p in pages]
    evaluated = [bool(p["flags"] & M.F_CRC_EVALUATED) for p in pages]
    if ft == M.INAV:
        assert ok == [False, True, True, True]  # even (nothing tested yet), odd, even (sticky), odd
        assert evaluated == [False, True, False, True]
        assert [bool(p["flags"] & M.F_ODD) for p in pages] == [False, True, False, True]
        assert [p["crc_error_counter"] for p in pages] == [1, 0, 0, 0]
    else:
        assert ok == [True] * 4 and evaluated == [True] * 4
    assert d.state()["stat"] == 2 and d.state()["frame_sync"] == 1


def test_state1_false_preamble_before_the_period_is_ignored():
    g = M.GEOMETRY[M.INAV]
    cap = g.required + 1
    # the window examined after symbol cap + k is symbols k .. k + P − 1
    d = M.TlmDecoder(M.INAV)
    body = np.ones(cap + 400, np.float32)
    body[0:g.P] = g.preamble       # oldest window after symbol cap → state 1 at counter cap
    body[100:100 + g.P] = g.preamble  # oldest window after symbol cap + 100: diff 100 < period
    d.run(body[:cap])
    assert d.stat == 1 and d.preamble_index == cap
    d.run(body[cap:cap + 100])
    assert d.stat == 1 and d.preamble_index == cap  # ignored
    d.run(body[cap + 100:cap + 400])
    assert d.stat == 1 and d.preamble_index == cap  # no hit at all: still state 1, however long


def test_state1_preamble_after_the_period_restarts():
    g = M.GEOMETRY[M.INAV]
    cap = g.required + 1
    d = M.TlmDecoder(M.INAV)
    body = np.ones(cap + 400, np.float32)
    body[0:g.P] = g.preamble
    body[g.period + 1:g.period + 1 + g.P] = g.preamble  # diff = period + 1
    d.run(body[:cap + g.period])
    assert d.stat == 1
    d.run(body[cap + g.period:cap + g.period + 1])
    assert d.stat == 0 and d.preamble_index == cap


def test_state1_preamble_at_the_period_locks_with_polarity():
    g = M.GEOMETRY[M.INAV]
    cap = g.required + 1
    for sign in (1.0, -1.0):
        d = M.TlmDecoder(M.INAV)
        body = np.ones(cap + g.period, np.float32)
        body[0:g.P] = g.preamble
        body[g.period:g.period + g.P] = g.preamble
        d.run(np.float32(sign) * body)
        assert d.stat == 2 and d.preamble_index == cap + g.period and d.pll_180 == (sign < 0)


def _corrupted(ft, n_bad, n_after=4):
    """A built F/NAV-style stream in which n_bad consecutive emitted parts fail their CRC (their CRC bits are wrong as
    built, the symbols themselves are clean), followed by good ones."""
    g = M.GEOMETRY[ft]
    rng = np.random.default_rng(9)
    good = [M.page_bits(ft, rng) for _ in range(2 + n_after)]
    bad = []
    for _ in range(n_bad):
        b = M.page_bits(ft, rng)
        b[g.crc_bits + 3] ^= 1
        bad.append(b)
    parts = good[:2] + bad + good[2:]
    body = np.concatenate([M.build_part(ft, b) for b in parts])
    tail = np.ones(g.required + 1 + 2 * g.period, np.float32)
    return np.concatenate([M.lead_in(ft, LEAD, 4), body, tail]), n_bad


@pytest.mark.parametrize("n_bad,lost", [(6, False), (7, True)])
def test_sync_loss_after_seven_failed_parts(n_bad, lost):
    x, _ = _corrupted(M.FNAV, n_bad)
    d = M.TlmDecoder(M.FNAV)
    pages, _ = d.run(x)
    # the first two stream parts pass before the history fills; emitted: n_bad failing parts, then the good ones
    flags = [p["flags"] for p in pages]
    fails = [not (f & M.F_CRC_OK) for f in flags[:n_bad]]
    assert all(fails)
    assert [p["crc_error_counter"] for p in pages[:n_bad]] == list(range(1, n_bad + 1))
    assert [bool(f & M.F_SYNC_LOST) for f in flags[:n_bad]] == [False] * 6 + ([True] if lost else [])
    if lost:
        assert not (flags[6] & M.F_FRAME_SYNC)
        assert len(pages) > 7 and pages[7]["symbol_counter"] - pages[6]["symbol_counter"] > M.GEOMETRY[M.FNAV].period  # re-sync takes longer
    else:
        assert len(pages) >= 7 and (flags[6] & M.F_CRC_OK) and pages[6]["crc_error_counter"] == 0
        assert pages[6]["symbol_counter"] - pages[5]["symbol_counter"] == M.GEOMETRY[M.FNAV].period


def test_tlm_separation_fires_once_and_after_reset():
    d = M.TlmDecoder(M.INAV)
    _, f = d.run(np.ones(15000, np.float32))
    assert not f
    _, f = d.run(np.ones(1, np.float32))
    assert f and d.sent_tlm_failed
    _, f = d.run(np.ones(20000, np.float32))
    assert not f
    d.reset()
    assert not d.sent_tlm_failed and d.last_valid_preamble == d.symbol_counter
    _, f = d.run(np.ones(15001, np.float32))
    assert f


def test_reset_keeps_history_and_sticky_flag():
    x, _ = _stream(M.INAV, 2)
    d = M.TlmDecoder(M.INAV)
    d.run(x)
    assert d.flag_crc_test and d.stat == 2
    h, even, cnt = d.history().copy(), d.page_even.copy(), d.symbol_counter
    d.reset()
    assert d.stat == 0 and not d.frame_sync and d.flag_crc_test and d.symbol_counter == cnt
    assert np.array_equal(d.history(), h) and np.array_equal(d.page_even, even)
