"""What the TRLWE sample extraction's tests share (tests/test_trlwe_extract_host.py on the CPU, tests/test_gpu_trlwe_extract.py on the GPU): a numpy
restatement of TRLWERep::sample_extract_index, inputs of random words with planted edge words, the oracle's words of a whole call, and the two
meaning cases with the seeds both tests use -- the CPU test checks on the oracle that those seeds decode every entry, the GPU test asserts the
oracle's words, so it cannot then fail on noise."""
import numpy as np

from kit import SMALL_N  # noqa: F401

EDGE_KS = np.array([0x00007FFF, 0x00008000, 0xFFFF7FFF, 0xFFFF8000, 0xFFFFFFFF, 0], np.uint32)      # EDGE_A of tests/test_gpu_pack.py: the key switch's rounding edges
EDGES = np.concatenate([np.array([0, 0x80000000, 0xFFFFFFFF], np.uint32), EDGE_KS[:4]])           # ... with the negation's (distinct values)


def extract_formula(x, N, j):
    """sample_extract_index(x, j) of a TRLWE u32[2][N] (b then a): e.a[c] = x.a[j - c] for c <= j, 0 - x.a[N + j - c] for c > j, e.b = x.b[j];
    u32[N + 1] (a', then b')"""
    x = np.ascontiguousarray(x, np.uint32).reshape(2, N)
    c = np.arange(N)
    a = x[1][(j - c) % N]
    e = np.empty(N + 1, np.uint32)
    e[:N] = np.where(c <= j, a, (0 - a.astype(np.int64)).astype(np.uint32))
    e[N] = x[0][j]
    return e


def coefficients(N, P, coef, stride):
    return np.arange(P, dtype=np.int64) * stride if coef is None else np.asarray(coef, np.int64)


def edge_slots(N, coefs):
    """(plain, negated): indices of the a-polynomial that land on the plain side (index <= j) for the largest coefficient j of the list and on
    the negated side (index > j) for the smallest, one per edge value where the list leaves room (j = 0 alone has one plain index, j = N - 1
    alone no negated one); the two sets are disjoint"""
    jmax, jmin = int(max(coefs)), int(min(coefs))
    plain = list(range(jmax, -1, -1))[:len(EDGES)]
    neg = [i for i in range(jmin + 1, N) if i not in plain][:len(EDGES)]
    return plain, neg


def trlwe_inputs(seed, N, count, coefs):
    """count TRLWEs of random words; in every a-polynomial each edge value once on the plain side and once on the negated side of the
    coefficients tested (edge_slots), the values rotated from row to row"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)
    plain, neg = edge_slots(N, coefs)
    for g in range(count):
        for k, i in enumerate(plain):
            x[g, 1, i] = EDGES[(g + k) % len(EDGES)]
        for k, i in enumerate(neg):
            x[g, 1, i] = EDGES[(g + k) % len(EDGES)]
    return x


def oracle_words(orc, P_orc, ksk, x, coefs):
    """(lvl1 [count][P][N+1], lvl0 [count][P][n+1]) from orc.sample_extract and orc.key_switch; read-only"""
    count, P = x.shape[0], len(coefs)
    lvl1 = np.empty((count, P, P_orc.N + 1), np.uint32)
    lvl0 = np.empty((count, P, P_orc.n + 1), np.uint32)
    for g in range(count):
        for p, j in enumerate(coefs):
            lvl1[g, p] = orc.sample_extract(P_orc, x[g].reshape(-1), int(j))
            lvl0[g, p] = orc.key_switch(P_orc, ksk, lvl1[g, p])
    lvl1.setflags(write=False)
    lvl0.setflags(write=False)
    return lvl1, lvl0


# ---- meaning with real keys (3-bit messages) ----
MEANING_BITS = 3
MEANING_KEY_SEED = {1024: 0xE871, 2048: 0xE872}
MEANING_PACK_P = 8


def meaning_keys(R, N):
    rp = R.Params(n=SMALL_N[N], N=N)
    key0, key1, _, ksk = R.keygen(rp, MEANING_KEY_SEED[N], want_bk=False)
    return rp, key0, key1, ksk


def meaning_case_a(R, N, rp, key1):
    """an encrypted polynomial of N random 3-bit messages; (messages, the TRLWE u32[1][2][N], the coefficients read)"""
    msgs = np.random.default_rng(N + 3).integers(0, 1 << MEANING_BITS, N)
    row = R.encrypt_lut(rp, key1, R.encode_msgs(msgs, MEANING_BITS), seed=0xA11 + N)
    return msgs, row, np.array([0, 1, N // 2, N - 1], np.int32)


def meaning_case_b(R, N, rp, key0, key1):
    """8 lvl0 ciphertexts of random 3-bit messages and a deterministic packing key; (messages, u32[1][8][n+1], pk)"""
    msgs = np.random.default_rng(N + 5).integers(0, 1 << MEANING_BITS, MEANING_PACK_P)
    ct = R.encrypt_torus(rp, key0, R.encode_msgs(msgs, MEANING_BITS), seed=0xB22 + N)
    return msgs, ct.reshape(1, MEANING_PACK_P, rp.n + 1), R.packing_keygen(rp, key0, key1, 0xBACC + N)
