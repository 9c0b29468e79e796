"""Write gnss_sim_receiver_amd/csrc/galileo_e5_tables.h from tests/golden/galileo_e5_codes_ref.npz.

    python tests/golden/make_e5_tables.py

The header holds what the product's Galileo E5 generators need, in the product's own form:

  * per component (E5a-I, E5a-Q, E5b-I, E5b-Q) the feedback mask of the one 28-stage linear recurrence
    all of its 50 primary codes obey, found here with Berlekamp–Massey on the first 200 chips of every
    code and checked over all 10230, and per PRN the code's first 28 chips as the register's start
    (bit j = chip j, 1 ↔ chip −1);
  * the pilot secondary codes as bit rows (bit i of word i / 32 = character i == '1'), the form
    SymSync::secondary_bits uses; rows of PRN the fixture holds no string for stay zero, and
    kE5aQSecondaryCount says how many rows E5a-Q has.

tests/test_codes_e5.py derives the same numbers again from the fixture and compares them with what
the library generates.
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COMPONENTS = ("e5a_i", "e5a_q", "e5b_i", "e5b_q")
STAGES = 28


def berlekamp_massey(s):
    """(L, c): the shortest recurrence s[n] = XOR_{i=1..L} c[i]·s[n-i] of a bit sequence."""
    n = len(s)
    c, b = [0] * n, [0] * n
    c[0] = b[0] = 1
    L, m = 0, -1
    for N in range(n):
        d = s[N]
        for i in range(1, L + 1):
            d ^= c[i] & s[N - i]
        if d:
            t = c[:]
            for i in range(n - N + m):
                c[N - m + i] ^= b[i]
            if L <= N // 2:
                L, m, b = N + 1 - L, N, t
    return L, c[:L + 1]


def recurrence(bits):
    """Feedback mask (bit j set: chip n − 28 + j enters chip n) and the 50 start words of one component."""
    found = set()
    for row in bits:
        L, c = berlekamp_massey([int(x) for x in row[:200]])
        found.add((L, tuple(c)))
    assert len(found) == 1, "one recurrence per component"
    L, c = found.pop()
    assert L == STAGES
    mask = sum(1 << (L - i) for i in range(1, L + 1) if c[i])
    for row in bits:  # the recurrence over the whole code: no short-cycle reset
        s = row.astype(np.int64)
        acc = np.zeros(len(s) - L, np.int64)
        for i in range(1, L + 1):
            if c[i]:
                acc ^= s[L - i:len(s) - i]
        assert np.array_equal(acc, s[L:])
    seeds = [sum(int(row[j]) << j for j in range(L)) for row in bits]
    return mask, seeds


def secondary_rows(strings):
    rows = []
    for s in strings:
        w = [0] * 4
        for i, ch in enumerate(str(s)):
            if ch == "1":
                w[i >> 5] |= 1 << (i & 31)
        rows.append(w)
    return rows


def main():
    z = np.load(os.path.join(HERE, "galileo_e5_codes_ref.npz"))
    lines = ["// galileo_e5_tables.h — written by tests/golden/make_e5_tables.py from the golden fixture; see there.",
             "#pragma once", "#include <cstdint>", "", "namespace gnsship {", "namespace e5 {", "",
             "// component order: E5a-I, E5a-Q, E5b-I, E5b-Q", "constexpr int kStages = %d;" % STAGES]
    masks, seeds = [], []
    for name in COMPONENTS:
        m, s = recurrence(np.unpackbits(z[name + "_bits"], axis=1)[:, :10230])
        masks.append(m)
        seeds.append(s)
    assert masks[0] == masks[1]  # E5a-I and E5a-Q share their polynomial
    lines.append("constexpr uint32_t kFeedback[4] = {%s};" % ", ".join("0x%07X" % m for m in masks))
    lines.append("constexpr uint32_t kStart[4][50] = {")
    for s in seeds:
        lines.append("    {%s}," % ", ".join("0x%07X" % v for v in s))
    lines.append("};")
    n_a = sum(1 for s in z["e5a_q_secondary"] if len(str(s)) == 100)
    assert all(len(str(s)) == 100 for s in z["e5a_q_secondary"][:n_a]) and all(len(str(s)) == 0 for s in z["e5a_q_secondary"][n_a:])
    lines.append("constexpr int kE5aQSecondaryCount = %d;  // PRN 1..%d: the table this was taken from ends there" % (n_a, n_a))
    for name in ("e5a_q", "e5b_q"):
        lines.append("constexpr uint32_t k%sSecondary[50][4] = {" % {"e5a_q": "E5aQ", "e5b_q": "E5bQ"}[name])
        for w in secondary_rows(z[name + "_secondary"]):
            lines.append("    {%s}," % ", ".join("0x%08X" % x for x in w))
        lines.append("};")
    lines.append('constexpr char kE5aISecondary[] = "%s";' % str(z["e5a_i_secondary"]))
    lines.append('constexpr char kE5bISecondary[] = "%s";' % str(z["e5b_i_secondary"]))
    lines += ["", "}  // namespace e5", "}  // namespace gnsship", ""]
    path = os.path.join(HERE, "..", "..", "gnss_sim_receiver_amd", "csrc", "galileo_e5_tables.h")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    print(os.path.normpath(path))


if __name__ == "__main__":
    main()
