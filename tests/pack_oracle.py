"""numpy restatement of the packing key switch (include/rtfhe.h: rtfhe_pack_batch): the digits of identity_key_switch, a gather of key
rows summed in uint32, rotation and replication by index arithmetic.  No device call, nothing from the package beyond the parameters."""
import numpy as np


def digits(a, ks_t=8, ks_basebit=2):
    """d[..., i, j] = ((a_i + ROUND) >> (32 - (j+1) basebit)) & (base - 1), ROUND = 2^(32 - t basebit - 1); a: u32[..., n]"""
    rnd = np.uint32(1 << (32 - ks_t * ks_basebit - 1))
    r = (np.asarray(a, np.uint32) + rnd).astype(np.uint32)          # wraps mod 2^32
    sh = np.array([32 - (j + 1) * ks_basebit for j in range(ks_t)], np.uint32)
    return ((r[..., None] >> sh) & np.uint32((1 << ks_basebit) - 1)).astype(np.int64)


def key_switch(params, pk, tlwe):
    """S(c) of every sample: tlwe u32[M][n+1], pk u32[n][t][base-1][2][N]  ->  u32[M][2][N]"""
    n, N, t, base1 = params.n, params.N, params.ks_t, (1 << params.ks_basebit) - 1
    tlwe = np.asarray(tlwe, np.uint32).reshape(-1, n + 1)
    rows = np.asarray(pk, np.uint32).reshape(n * t * base1, 2 * N)
    d = digits(tlwe[:, :n], t, params.ks_basebit)                   # [M][n][t]
    first = (np.arange(n)[:, None] * t + np.arange(t)[None, :]) * base1      # row of digit value 1 of (i, j)
    out = np.zeros((tlwe.shape[0], 2 * N), np.uint32)
    for m in range(tlwe.shape[0]):
        sel = (first + d[m] - 1)[d[m] != 0]
        out[m] = np.uint32(0) - rows[sel].sum(axis=0, dtype=np.uint32)
        out[m, :1] += tlwe[m, n:n + 1]
    return out.reshape(-1, 2, N)


def default_pos(P, rep):
    return np.arange(P, dtype=np.int64) * rep


def combine(S, P, pos, rep):
    """out[g][h][c] = sum_p sum_{k<rep} +- S[g P + p][h][u mod N], u = (c - pos[p] - k) mod 2N, + iff u < N; S u32[count * P][2][N]"""
    S = np.asarray(S, np.uint32)
    N = S.shape[-1]
    count = S.shape[0] // P
    pos = default_pos(P, rep) if pos is None else np.asarray(pos, np.int64)
    c = np.arange(N)
    out = np.zeros((count, 2, N), np.uint32)
    for p in range(P):
        sp = S[p::P][:count]                                        # sample p of every output: [count][2][N]
        for k in range(rep):
            u = (c - int(pos[p]) - k) % (2 * N)
            v = sp[:, :, u % N]
            out += np.where(u < N, v, np.uint32(0) - v).astype(np.uint32)
    return out


def pack(params, pk, tlwe, P, pos=None, rep=1):
    """rtfhe_pack_batch: tlwe u32[count][P][n+1]  ->  u32[count][2][N]"""
    return combine(key_switch(params, pk, tlwe), P, pos, rep)
