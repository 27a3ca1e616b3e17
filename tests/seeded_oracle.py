"""TEST INFRASTRUCTURE: the mask rule of seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts") restated in numpy, written
from RFC 8439 2.3 and the rule's text, not from the library's code.  A mask seed is a ChaCha20 key u32[8]; row R of length N has
a[16 c + i] = word i of the block with the 64-bit counter c in state words 12-13 and R in state words 14-15, c = 0 .. N/16 - 1."""
import numpy as np

SIGMA = np.array([0x61707865, 0x3320646e, 0x79622d32, 0x6b206574], np.uint32)
KAT_KEY = np.frombuffer(bytes(range(32)), "<u4")        # key bytes 00 .. 1f, the key of RFC 8439 2.3.2 and of the known answers


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)


def blocks(state):
    """The ChaCha20 block function on many states at once: u32[16][...] -> u32[16][...] (20 rounds, then the feed-forward)."""
    state = np.asarray(state, np.uint32)
    x = [state[i].copy() for i in range(16)]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
            _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
        return np.stack([x[i] + state[i] for i in range(16)])


def block(key, w12, w13, w14, w15):
    """one block: the 16 output words for the key u32[8] and the last four state words"""
    st = np.concatenate([SIGMA, np.asarray(key, np.uint32).reshape(8), np.array([w12, w13, w14, w15], np.uint32)])
    return blocks(st.reshape(16, 1))[:, 0]


def mask_rows(N, seed, first_row, rows):
    """u32[rows][N]: the masks of rows first_row .. first_row + rows - 1 (python ints: first_row + rows may reach 2^64)"""
    nb = N // 16
    R = np.array([(int(first_row) + r) % (1 << 64) for r in range(rows)], np.uint64)
    st = np.empty((16, rows, nb), np.uint32)
    st[0:4] = SIGMA[:, None, None]
    st[4:12] = np.asarray(seed, np.uint32).reshape(8)[:, None, None]
    st[12] = np.arange(nb, dtype=np.uint32)[None, :]
    st[13] = 0
    st[14] = (R & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    st[15] = (R >> np.uint64(32)).astype(np.uint32)[:, None]
    out = blocks(st)                                     # [16][rows][nb]
    return np.ascontiguousarray(out.transpose(1, 2, 0)).reshape(rows, N)


def expand(N, seed, first_row, b, group):
    """the full layout u32[rows / group][2][group][N] of the seeded object (seed, first_row, b u32[rows][N])"""
    b = np.asarray(b, np.uint32).reshape(-1, N)
    rows = b.shape[0]
    assert group >= 1 and rows % group == 0
    a = mask_rows(N, seed, first_row, rows)
    return np.stack([b.reshape(-1, group, N), a.reshape(-1, group, N)], axis=1)
