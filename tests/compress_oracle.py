"""TEST INFRASTRUCTURE: a numpy restatement of compressed results (include/rtfhe.h, "compressed results"), written from the specification -- one
bit at a time, with no accumulator and no word arithmetic, so that it shares no idea with the C twins or the kernel -- plus the inputs with
planted edge words that the CPU and GPU tests share."""
import numpy as np


def words(L, k):
    """W(L, k) = ceil(L k / 32)"""
    return -(-L * k // 32)


def round_values(v, k):
    """r[i] = ((v[i] + 2^(31-k)) mod 2^32) >> (32 - k); k = 32: v itself.  v: u32[..., L] -> int64[..., L], each below 2^k"""
    v = np.asarray(v, np.uint32).astype(np.int64)
    return v if k == 32 else ((v + (1 << (31 - k))) % (1 << 32)) >> (32 - k)


def pack_rows(r, k):
    """rows of k-bit values int64[count][L] -> u32[count][W]: bit j of r[i] is stream bit i k + j, stream bit s is bit s mod 32 of word s / 32,
    the unused high bits of the last word are zero"""
    r = np.asarray(r, np.int64)
    count, L = r.shape
    W = words(L, k)
    bits = ((r[:, :, None] >> np.arange(k)) & 1).reshape(count, L * k)                 # the stream, one entry per bit
    stream = np.zeros((count, W * 32), np.int64)
    stream[:, :L * k] = bits
    return (stream.reshape(count, W, 32) << np.arange(32)).sum(axis=2).astype(np.uint32)


def unpack_rows(w, L, k):
    """u32[count][W] -> the k-bit values int64[count][L]"""
    w = np.asarray(w, np.uint32).astype(np.int64)
    stream = ((w[:, :, None] >> np.arange(32)) & 1).reshape(w.shape[0], -1)[:, :L * k]
    return (stream.reshape(w.shape[0], L, k) << np.arange(k)).sum(axis=2)


def coefficients(P, coef, stride):
    return np.arange(P, dtype=np.int64) * stride if coef is None else np.asarray(coef, np.int64)


def tlwe_compress(x, k):
    """[count][n+1] -> [count][W(n+1, k)]: the row is the whole sample"""
    x = np.asarray(x, np.uint32)
    return pack_rows(round_values(x, k), k)


def tlwe_expand(w, n, k):
    return (unpack_rows(w, n + 1, k) << (32 - k)).astype(np.uint32)


def trlwe_row(x, coefs):
    """[count][2][N] (b then a) -> the rows a[0 .. N), b[coef[0]], .., b[coef[P-1]]: [count][N + P]"""
    x = np.asarray(x, np.uint32)
    return np.concatenate([x[:, 1, :], x[:, 0, :][:, coefs]], axis=1)


def trlwe_compress(x, k, P, coef=None, stride=1):
    return pack_rows(round_values(trlwe_row(x, coefficients(P, coef, stride)), k), k)


def trlwe_expand(w, N, k, P, coef=None, stride=1):
    """full rows [count][2][N]: b zero at the coefficients that were not kept; with duplicates the later entry wins"""
    v = (unpack_rows(w, N + P, k) << (32 - k)).astype(np.uint32)
    out = np.zeros((v.shape[0], 2, N), np.uint32)
    out[:, 1, :] = v[:, :N]
    for p, j in enumerate(coefficients(P, coef, stride)):
        out[:, 0, j] = v[:, N + p]
    return out


def edge_words(k):
    """0, 2^(31-k) - 1 (the largest word that rounds down to 0), 2^(31-k) (the smallest that rounds up to 1), 0xFFFFFFFF and 2^32 - 2^(31-k) (the
    smallest word that rounds up to 2^k and wraps to 0); at k = 32 nothing rounds: the same positions hold 0, 1, 0x80000000 and 0xFFFFFFFF"""
    if k == 32:
        return np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32)
    h = 1 << (31 - k)
    return np.array([0, h - 1, h, 0xFFFFFFFF, (1 << 32) - h], np.uint32)


def plant_edges(rows, k):
    """rows u32[count][L] of random words, in place: the edge words at the first values of a row, at its last values, and at the values that
    straddle the first word boundaries of the stream (value i with i k < 32 m < (i + 1) k), rotated from row to row"""
    E = edge_words(k)
    count, L = rows.shape
    slots = list(range(min(L, len(E)))) + list(range(max(L - len(E), 0), L))
    slots += [i for i in range(L) if (i * k) // 32 != ((i + 1) * k - 1) // 32][:2 * len(E)]
    for g in range(count):
        for t, i in enumerate(slots):
            rows[g, i] = E[(g + t) % len(E)]
    return rows


def tlwe_inputs(seed, n, count, k):
    rng = np.random.default_rng(seed)
    return plant_edges(rng.integers(0, 1 << 32, (count, n + 1), dtype=np.uint64).astype(np.uint32), k)


def trlwe_inputs(seed, N, count, k, coefs):
    """random TRLWEs whose compressed row (a, then b at the kept coefficients) carries the planted edges; where a coefficient is listed twice the
    later plant stands, which both entries then read"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)
    row = plant_edges(trlwe_row(x, coefs), k)
    x[:, 1, :] = row[:, :N]
    for p, j in enumerate(coefs):
        x[:, 0, j] = row[:, N + p]
    return x
