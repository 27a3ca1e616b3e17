"""TEST INFRASTRUCTURE: the oracle of the lvl0 dense layer (include/rtfhe.h: rtfhe_tlwe_dense_batch), numpy in int64:

    out[g][o][c] = (acc[g][o][c] if acc is given else 0) + [c == n] bias[o] + sum_i W[o][i] x[g][i][c]    mod 2^32

|W| <= 128, x < 2^32 and I <= 65,536 keep every int64 sum below 2^55: nothing wraps before the mask.  Also the rows with planted edge words the
GPU tests multiply, the correction words the library keeps per output, and a self-test against a Python-int loop (run on the CPU by
tests/test_dense_host.py)."""
import numpy as np

MASK = 0xFFFFFFFF
EDGE_WORDS = (0, 0x7F7F7F7F, 0x80808080, 0xFFFFFFFF, 0x0080FF7F)      # every byte at both ends of the signed limbs, and a mixed word


def dense(W, x, bias=None, acc=None):
    """W: int [O][I]; x: u32 [count][I][n+1]; bias: u32 [O] or None; acc: u32 [count][O][n+1] or None.  u32 [count][O][n+1]."""
    W = np.asarray(W).astype(np.int64)
    x = np.asarray(x, np.uint32)
    assert W.ndim == 2 and x.ndim == 3 and x.shape[1] == W.shape[1]
    out = np.stack([(W @ xg.astype(np.int64)) & MASK for xg in x]) if x.shape[0] else np.zeros((0, W.shape[0], x.shape[2]), np.int64)
    if bias is not None:
        out[:, :, -1] += np.asarray(bias, np.uint32).astype(np.int64)[None, :]
    if acc is not None:
        out = out + np.asarray(acc, np.uint32).astype(np.int64).reshape(out.shape)
    return (out & MASK).astype(np.uint32)


def correction(W):
    """what the kernel's signed byte limbs drop from every word of output o: 128 * 0x01010101 * sum_i W[o][i] mod 2^32; u32[O]"""
    return np.array([(128 * 0x01010101 * int(s)) & MASK for s in np.asarray(W).astype(np.int64).sum(axis=1)], np.uint32)


def rows_with_edges(seed, count, I, words):
    """u32[count][I][words] of random words with EDGE_WORDS planted: each edge word in the first and the last column of some row of every sample
    (as far as I reaches), the rest random"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (count, I, words), dtype=np.uint64).astype(np.uint32)
    for g in range(count):
        for k, e in enumerate(EDGE_WORDS):
            x[g, (g + k) % I, 0] = e
            x[g, (g + 2 * k + 1) % I, words - 1] = e
            x[g, (3 * k + g) % I, (7 * k + g) % words] = e
    return x


def weights(seed, O, I):
    """int32[O][I] uniform in [-128, 127] with both ends planted"""
    rng = np.random.default_rng(seed)
    W = rng.integers(-128, 128, (O, I)).astype(np.int32)
    W[0, 0], W[O - 1, I - 1] = -128, 127
    if I > 1:
        W[O // 2, 1] = 127 if W[0, 0] == -128 else -128
    return W


def self_test():
    """the numpy oracle against a loop over Python ints at a tiny shape, bias and accumulate included"""
    O, I, words, count = 3, 5, 4, 2
    W = weights(1, O, I)
    x = rows_with_edges(2, count, I, words)
    bias = np.array([7, MASK, 1 << 31], np.uint32)
    acc = np.random.default_rng(3).integers(0, 1 << 32, (count, O, words), dtype=np.uint64).astype(np.uint32)
    for b, a in ((None, None), (bias, None), (None, acc), (bias, acc)):
        got = dense(W, x, b, a)
        for g in range(count):
            for o in range(O):
                for c in range(words):
                    want = sum(int(W[o, i]) * int(x[g, i, c]) for i in range(I))
                    if b is not None and c == words - 1:
                        want += int(b[o])
                    if a is not None:
                        want += int(a[g, o, c])
                    assert int(got[g, o, c]) == want % (1 << 32), (g, o, c)
    assert np.array_equal(correction(W), np.array([(0x80808080 * (int(W[o].sum()) % (1 << 32))) % (1 << 32) for o in range(O)], np.uint32))
    return True
