"""TEST INFRASTRUCTURE: the TRLWE x TRGSW multiply-accumulate (include/rtfhe.h: rtfhe_trlwe_mul_trgsw_batch) restated from the oracle's own
blocks, in round_oracle.external_product's order with the running sums carried over the K terms:

    sum_c  = 0.0;  for k (term-major), for h = b, a, for j = 0 .. l-1:
                 sum_c = sum_c + orc_hadamard(S[s_idx[g][k]].row(c, h, j), orc_ifft_i32(digit_j(x[x_idx[g][k]].poly_h)))        c = 0, 1
    out[g].poly_c = (acc[g].poly_c if acc is given else 0) + orc_fft_u32(sum_c)                                  wrapping u32 add

K = 1 without acc is round_oracle.external_product word for word (tests/test_trgsw_mac_host.py); every word of the device is compared with this
(tests/test_gpu_trgsw_mac.py).  Beside it the inputs both of those files use: rows with the decomposition's edge words, the rows that drive
every digit to its largest magnitude, the noise bound of the meaning tests and their world."""
import ctypes as C

import numpy as np

import orc
import round_oracle as ro
from kit import torus_err  # noqa: F401
from round_oracle import REFERENCE, ROUNDED  # noqa: F401

_f64p, _u32p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
K_MAX = 8


def mac(p, plan, sel_f, s_idx, x_rows, x_idx, acc, mode, sums=None):
    """sel_f: float64[n_sel * 2 * 2l * N] spectra of the selector set (orc_trgsw_to_fft); x_rows: u32[n_x][2][N]; s_idx, x_idx: int [count][K]
    (None: g * K + k, with K taken from the other array, K = 1 when both are None); acc: u32[count][2][N] or None.  Returns u32[count][2][N].  sums: a list that
    receives every (g, c, sum_c) before its orc_fft_u32, for the tests of the conversion's range."""
    L = orc.lib()
    N, l, rows = p.N, p.l, 2 * p.l
    ma, mx = ro.constants(l, p.bgbit, mode)
    x_rows = np.ascontiguousarray(x_rows, np.uint32).reshape(-1, 2, N)
    given = s_idx if s_idx is not None else x_idx
    if given is not None:
        given = np.asarray(given, np.int64)
        count, K = given.shape
    else:
        count, K = (x_rows.shape[0] if acc is None else np.asarray(acc).size // (2 * N)), 1
    nat = np.arange(count * K, dtype=np.int64).reshape(count, K)
    s_idx = nat if s_idx is None else np.asarray(s_idx, np.int64).reshape(count, K)
    x_idx = nat if x_idx is None else np.asarray(x_idx, np.int64).reshape(count, K)
    trgsw = 2 * rows * N
    out = np.empty((count, 2, N), np.uint32)
    had, dec_f, word = np.empty(N, np.float64), np.empty(N, np.float64), np.empty(N, np.uint32)
    for g in range(count):
        s = [np.zeros(N, np.float64), np.zeros(N, np.float64)]
        for k in range(K):
            key = np.ascontiguousarray(sel_f[int(s_idx[g, k]) * trgsw:(int(s_idx[g, k]) + 1) * trgsw], np.float64).reshape(2, rows, N)
            row = x_rows[int(x_idx[g, k])]
            for h in range(2):
                dec = ro.digits(row[h], l, p.bgbit, ma, mx)
                for j in range(l):
                    L.orc_ifft_i32(plan.h, dec_f.ctypes.data_as(_f64p), dec[j].ctypes.data_as(_i32p))
                    for c in range(2):
                        L.orc_hadamard(N, had.ctypes.data_as(_f64p), key[c, h * l + j].ctypes.data_as(_f64p), dec_f.ctypes.data_as(_f64p))
                        s[c] = s[c] + had
        for c in range(2):
            if sums is not None:
                sums.append((g, c, s[c].copy()))
            L.orc_fft_u32(plan.h, word.ctypes.data_as(_u32p), s[c].ctypes.data_as(_f64p))
            out[g, c] = word if acc is None else word + np.asarray(acc, np.uint32).reshape(count, 2, N)[g, c]
    return out


def spectra(p, plan, trgsw_t):
    """orc_trgsw_to_fft of TRGSW words u32[n_sel][2][2l][N]: what rtfhe_trgsw_create builds on the device"""
    t = np.ascontiguousarray(trgsw_t, np.uint32).reshape(-1)
    f = np.empty(t.size, np.float64)
    orc.lib().orc_trgsw_to_fft(plan.h, t.ctypes.data_as(_u32p), f.ctypes.data_as(_f64p), t.size // p.N)
    return f


def edge_words(l=3, bits=6):
    """the decomposition's edge words: the four corners of u32, and one below / at / one above a digit boundary of each mode -- the reference
    mode's digits change where x + mask carries into a field (x = -mask's fields: multiples of the last digit's unit), the rounded mode's half
    a unit of the last digit away from those"""
    unit = 1 << (32 - l * bits)
    top = 1 << (32 - bits)
    e = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    for b in (unit, 5 * unit, top, top + unit, 0x80000000 + unit, (1 << 32) - unit):
        e += [b - 1, b, b + 1, b - unit // 2 - 1, b - unit // 2, b - unit // 2 + 1, b + unit // 2 - 1, b + unit // 2, b + unit // 2 + 1]
    return np.array([v & 0xFFFFFFFF for v in e], np.uint32)


def rows_with_edges(seed, N, n_rows):
    """u32[n_rows][2][N]: random words, the edge words planted at random places of both polynomials of every row"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, (n_rows, 2, N), dtype=np.uint64).astype(np.uint32)
    e = edge_words()
    for r in range(n_rows):
        for c in range(2):
            x[r, c, rng.choice(N, e.size, replace=False)] = e
    return x


def extreme_word(mode, l=3, bits=6):
    """a word whose every digit has the largest magnitude its mode admits, -Bg/2 (checked through round_oracle.digits by the callers)"""
    ma, mx = ro.constants(l, bits, mode)
    half = 1 << (bits - 1)
    u = sum(half << (32 - bits * (j + 1)) for j in range(l))        # every field = 100000b: the digit -Bg/2
    return ((u ^ mx) - ma) & 0xFFFFFFFF


def extreme_rows(N, n_rows, mode):
    """u32[n_rows][2][N] with every word extreme_word: with every selector word 0x80000000 (-2^31 as the transform reads it) coefficient N - 1
    of a product is 2l * N * (Bg/2) * 2^31 and a K-term sum K times that: 2^51.58 (N = 1024) and 2^52.58 (N = 2048) at K = 8"""
    return np.full((n_rows, 2, N), extreme_word(mode), np.uint32)


def noise_bound(N, mu_norms2, l=3):
    """6 sqrt(sum_k [2 l N 18.5^2 2^-50 + ||mu_k||_2^2 ((N/2 + 1) 2^-38 / 3 + N 2^-50)]): per term the selector rows' 2^-25 noise through 2 l N
    balanced 6-bit digits (rms 18.5; leveled_round_oracle.noise_bound's first term, which does not scale with mu), the rounding error (uniform
    in +-2^-19, times the binary key) through mu, and the input row's own phase noise through mu"""
    per = [2 * l * N * 18.5 ** 2 * 2.0 ** -50 + float(m2) * ((N / 2 + 1) * 2.0 ** -38 / 3 + N * 2.0 ** -50) for m2 in mu_norms2]
    return 6.0 * float(np.sqrt(sum(per)))


def negacyclic_i64(mu, m):
    """mu(X) * m(X) mod X^N + 1 in int64 (small operands), as u32 torus words"""
    mu, m = np.asarray(mu, np.int64), np.asarray(m, np.int64)
    N = mu.size
    full = np.convolve(mu, m)
    res = full[:N].copy()
    res[:N - 1] -= full[N:]
    return (res & 0xFFFFFFFF).astype(np.uint32)


def meaning_world(R):
    """The inputs of the meaning tests (tests/test_trgsw_mac_host.py through the restatement, tests/test_gpu_trgsw_mac.py on the device): n = 40,
    N = 1024, K = 4 ternary weight polynomials of 48 non-zero coefficients each, TRGSW-encrypted, times K fresh TRLWE rows of N random 3-bit
    messages, for 3 samples: 3 * 1024 = 3,072 checked coefficients of the phase."""
    import types
    m = types.SimpleNamespace(K=4, COUNT=3, MSG_BITS=3, NONZERO=48)
    m.rp = R.Params(n=40, N=1024)
    _, m.key1, _, _ = R.keygen(m.rp, 0x3AC1, want_bk=False, want_ksk=False)
    rng = np.random.default_rng(0x3AC2)
    N = m.rp.N
    m.mu = np.zeros((m.COUNT * m.K, N), np.int32)
    for e in range(m.mu.shape[0]):
        m.mu[e, rng.choice(N, m.NONZERO, replace=False)] = rng.choice([-1, 1], m.NONZERO)
    m.sel_t = R.encrypt_trgsw_polys(m.rp, m.key1, m.mu, seed=0x3AC3)
    m.msgs = rng.integers(0, 1 << m.MSG_BITS, (m.COUNT * m.K, N))
    m.plain = R.encode_msgs(m.msgs, m.MSG_BITS)
    m.rows = R.encrypt_lut(m.rp, m.key1, m.plain, seed=0x3AC4)
    m.want = np.stack([sum(negacyclic_i64(m.mu[g * m.K + k], m.plain[g * m.K + k].view(np.int32)).astype(np.uint64) for k in range(m.K)).astype(np.uint32)
                       for g in range(m.COUNT)])
    m.bound = [noise_bound(N, [float((m.mu[g * m.K + k].astype(np.int64) ** 2).sum()) for k in range(m.K)]) for g in range(m.COUNT)]
    return m
