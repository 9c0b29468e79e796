"""The committed Viterbi fixture (tests/golden/viterbi_ref.npz), loaded once and shared by the tests that need it."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viterbi_ref.npz")
LENGTHS = (114, 238, 486)
KINDS = (0, 1, 2, 3)
FRAMES = 4


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(LL, kind):
    """(symbols float32[4, frame], reference bits uint8[4, LL], sections float32[4, 64], encoded bits or None) of one
    reference object's four calls.  Read-only."""
    g = golden()
    sym = g[f"sym_{LL}_{kind}"]
    bits = np.unpackbits(g[f"bits_{LL}_{kind}"], axis=1)[:, :LL]
    sec = g[f"sec_{LL}_{kind}"]
    truth = np.unpackbits(g[f"truth_{LL}_{kind}"], axis=1)[:, :LL] if f"truth_{LL}_{kind}" in g else None
    for a in (sym, bits, sec, truth):
        if a is not None:
            a.setflags(write=False)
    return sym, bits, sec, truth
