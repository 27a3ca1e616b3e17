"""TEST INFRASTRUCTURE: the mask rule of seeded lvl0 ciphertexts (include/rtfhe.h, "seeded lvl0 ciphertexts") restated in numpy,
written from the rule's text, not from the library's code.  Row R of a lvl0 object has a[16 c + i] = word i of the ChaCha20 block with key = seed,
the 64-bit counter c in state words 12-13 and R in state words 14-15, c = 0 .. ceil(n / 16) - 1; the words with 16 c + i >= n are discarded.  The
block function is the one of tests/seeded_oracle.py (RFC 8439 2.3)."""
import numpy as np

import seeded_oracle as so


def mask_rows(n, seed, first_row, rows):
    """u32[rows][n]: the masks of rows first_row .. first_row + rows - 1 (python ints: first_row + rows may reach 2^64)"""
    nb = -(-n // 16)
    return np.ascontiguousarray(so.mask_rows(16 * nb, seed, first_row, rows)[:, :n])


def expand(n, seed, first_row, b):
    """the full layout u32[rows][n + 1] of the seeded lvl0 object (seed, first_row, b u32[rows]): a[0 .. n) then b"""
    b = np.asarray(b, np.uint32).reshape(-1)
    return np.concatenate([mask_rows(n, seed, first_row, b.size), b[:, None]], axis=1)
