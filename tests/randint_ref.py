"""Host restatement of e2eft_randint_fill (include/e2eft.h, "Integers of [0, high) from the generator's raw words"), written from that definition on
tests/noise_ref.py::words.  TEST INFRASTRUCTURE ONLY.

  from_word(word, high)                          -> (word * high) >> 32 in exact Python integers
  randint(seed, draw, slot, n, high, repeat=1)   -> int64 numpy [repeat * n]: element e takes word e & 3 of the counter of quad e >> 2, copy r at r * n + e
"""
import numpy as np

import noise_ref


def from_word(word, high):
    word, high = int(word), int(high)
    assert 0 <= word < 2 ** 32 and 1 <= high <= 2 ** 31 - 1
    return (word * high) >> 32


def randint(seed, draw, slot, n, high, repeat=1):
    out, e = noise_ref.words(seed, draw, slot, n)            # [n, 4] uint32: row e holds the four words of quad e >> 2
    word = out[np.arange(n), (e & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    t = (word * np.uint64(high)) >> np.uint64(32)            # word < 2^32, high < 2^31: the product fits 63 bits
    return np.tile(t.astype(np.int64), repeat)
