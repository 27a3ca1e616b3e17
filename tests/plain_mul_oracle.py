"""The numpy oracle of the exact TRLWE x plain-polynomial product (include/rtfhe.h: rtfhe_trlwe_mul_plain_batch): np.convolve in int64, folded
negacyclically, masked to 32 bits.  Ciphertext words are read as signed (|x| <= 2^31) and the accepted weights have K * ||w||_1 <= 192 N, so
every sum stays below 2^31 * 192 * 2048 < 2^50: int64 is exact.  Shared by the CPU and GPU tests; inputs with the split's edge words too."""
import numpy as np

MASK = 0xFFFFFFFF
# the edges of the split into signed 16-bit halves (tests/test_gpu_xfft.py): lo = -2^15 with hi = 0 / +2^15 / -2^15, the extremes of both halves
EDGES = np.array([0, 0x00008000, 0x7FFF8000, 0x80008000, 0x8000FFFF, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
L1_PER_N = 192          # a call is accepted iff K * wmax <= 192 N
K_MAX = 8


def negacyclic(w, x):
    """w int[N] (any integers with ||w||_1 * 2^31 < 2^62), x u32[N] -> u32[N]: w * x in Z_2^32[X]/(X^N + 1)"""
    w = np.asarray(w).astype(np.int64)
    xs = np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)
    N = w.size
    assert xs.size == N and int(np.abs(w).sum()) < 1 << 31
    full = np.convolve(w, xs)
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return (out & MASK).astype(np.uint32)


def negacyclic_bigint(w, x, coefficients):
    """the same at a few coefficients, by the definition in Python integers"""
    N = len(w)
    w = [int(v) for v in w]
    x = [int(v) for v in np.asarray(x, dtype=np.uint32)]
    out = []
    for c in coefficients:
        s = 0
        for a in range(N):
            b = c - a
            s += w[a] * x[b] if b >= 0 else -w[a] * x[b + N]
        out.append(s & MASK)
    return np.array(out, np.uint32)


def mul_plain(w, x, K=1, w_idx=None, x_idx=None, acc=None, count=None):
    """out[g] = (acc[g] or 0) + sum_k w[w_idx[g][k]] * x[x_idx[g][k]] on both polynomials of every row; w int[n_w][N], x u32[n_x][2][N]"""
    w = np.asarray(w)
    x = np.asarray(x, dtype=np.uint32)
    N = w.shape[1]
    if count is None:
        count = (np.asarray(w_idx).size // K if w_idx is not None else np.asarray(x_idx).size // K if x_idx is not None
                 else np.asarray(acc).size // (2 * N) if acc is not None else x.shape[0] // K)
    wi = np.tile(np.arange(K), (count, 1)) if w_idx is None else np.asarray(w_idx).reshape(count, K)
    xi = np.arange(count * K).reshape(count, K) if x_idx is None else np.asarray(x_idx).reshape(count, K)
    out = np.zeros((count, 2, N), np.uint32) if acc is None else np.array(acc, dtype=np.uint32).reshape(count, 2, N)
    memo = {}
    for g in range(count):
        for k in range(K):
            key = (int(wi[g, k]), int(xi[g, k]))
            if key not in memo:
                memo[key] = np.stack([negacyclic(w[key[0]], x[key[1], c]) for c in range(2)])
            out[g] += memo[key]            # uint32: wraps mod 2^32
    return out


def rows_with_edges(seed, N, n_x):
    """u32[n_x][2][N] of random words with every edge word planted in both polynomials of every row, at positions that differ by row"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (n_x, 2, N), dtype=np.uint64).astype(np.uint32)
    for r in range(n_x):
        for c in range(2):
            at = rng.choice(N, EDGES.size, replace=False)
            x[r, c, at] = EDGES
            x[r, c, [0, N // 2, N - 1][(r + c) % 3]] = EDGES[(r + 2 * c) % EDGES.size]      # and on a coefficient the fold treats specially
    return x


def weights(seed, N, n_w, l1):
    """int32[n_w][N]: random signs, dense small entries, every polynomial's l1 norm exactly `l1` (l1 <= 192 N)"""
    rng = np.random.default_rng(seed)
    w = np.zeros((n_w, N), np.int64)
    for e in range(n_w):
        mag = np.full(N, l1 // N, np.int64)
        mag[rng.choice(N, l1 - int(mag.sum()), replace=False)] += 1
        w[e] = mag * rng.choice([-1, 1], N)
    assert (np.abs(w).sum(axis=1) == l1).all()
    return w.astype(np.int32)


def extreme_weights(N, l1_per_coef):
    """the four sign patterns of the largest sums, |w[c]| = l1_per_coef everywhere: all +, all -, alternating, half / half; int32[4][N]"""
    m = l1_per_coef
    alt = np.where(np.arange(N) % 2 == 0, m, -m)
    half = np.where(np.arange(N) < N // 2, m, -m)
    return np.stack([np.full(N, m), np.full(N, -m), alt, half]).astype(np.int32)


def aligned_rows(w, N, targets=None):
    """For each polynomial w[e] and each target coefficient c of (0, N/2, N-1), two rows u32[2][N] whose every word is 0x7FFF7FFF or 0x80008000
    (the largest hi and lo halves of one sign), signed so that EVERY term of output coefficient c has the same sign: polynomial 0 of the row
    drives the sum to its maximum, polynomial 1 to its minimum.  -> u32[n_w * 3][2][N], row e * 3 + t."""
    targets = (0, N // 2, N - 1) if targets is None else targets
    POS, NEG = 0x7FFF7FFF, 0x80008000
    rows = np.zeros((len(w) * len(targets), 2, N), np.uint32)
    for e, we in enumerate(np.asarray(w).astype(np.int64)):
        for t, c in enumerate(targets):
            b = np.arange(N)
            a = (c - b) % N
            sign = np.where(we[a] >= 0, 1, -1) * np.where(b <= c, 1, -1)          # the term's sign for a positive x[b]
            rows[e * len(targets) + t, 0] = np.where(sign > 0, POS, NEG)
            rows[e * len(targets) + t, 1] = np.where(sign > 0, NEG, POS)
    return rows
