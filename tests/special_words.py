"""Special f32 words for static feature tables: the values a copy loop could alter without any
well-conditioned fixture noticing.  Shared by the fixture generator (tests/golden/make_golden.py
--numeric), the strata table (tests/strata.py) and the GPU tests that build such a table themselves.

No signalling NaN is among them: the reference quiets those when pandas widens its f32 feature
columns to f64 and narrows them back, so the expected output would not be the input.
"""
from __future__ import annotations

import numpy as np

SPECIAL_F32_WORDS = np.array([
    0x7FC00000, 0x7FC12345, 0xFFC00001,   # quiet NaNs of both signs, with and without payload
    0x7F800000, 0xFF800000,               # +inf, -inf
    0x80000000,                           # -0.0
    0x00000001, 0x80000001,               # the smallest subnormal of either sign
    0x007FFFFF, 0x807FFFFF,               # the largest subnormal of either sign
    0x7F7FFFFF,                           # FLT_MAX
    0x00800000,                           # FLT_MIN
], dtype=np.uint32)


def place_special_words(feat, seed, fraction=0.15):
    """A copy of f32 table `feat` with about `fraction` of its cells replaced by SPECIAL_F32_WORDS,
    every word at least once (the table must have that many cells)."""
    feat = np.array(feat, dtype=np.float32, order="C")
    words = feat.view(np.uint32).reshape(-1)
    rng = np.random.default_rng(seed)
    n = max(int(round(fraction * words.size)), len(SPECIAL_F32_WORDS))
    assert n <= words.size
    cells = rng.choice(words.size, n, replace=False)
    pick = np.concatenate([np.arange(len(SPECIAL_F32_WORDS)),
                           rng.integers(0, len(SPECIAL_F32_WORDS), n - len(SPECIAL_F32_WORDS))])
    words[cells] = SPECIAL_F32_WORDS[pick]
    return feat


def is_signalling_nan(feat):
    """Elementwise: an f32 NaN whose quiet bit (bit 22) is clear."""
    w = np.ascontiguousarray(feat, np.float32).view(np.uint32)
    return ((w & 0x7F800000) == 0x7F800000) & ((w & 0x007FFFFF) != 0) & ((w & 0x00400000) == 0)


def has_every_special_word(feat):
    """Whether every one of SPECIAL_F32_WORDS occurs in f32 table `feat`."""
    w = np.ascontiguousarray(feat, np.float32).view(np.uint32)
    return bool(np.isin(SPECIAL_F32_WORDS, w).all())
