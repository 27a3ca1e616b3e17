"""TEST INFRASTRUCTURE: the TRLWE key switch (include/rtfhe.h: rtfhe_trlwe_auto_batch) restated from the oracle's own blocks, in
round_oracle.external_product's order.  One step with entry e of the switching key K (u32[n_t][l][2][N]) and t = t[e] on a row x = (b, a):

    a' = automorphism(a, t),  b' = automorphism(b, t)          sigma_t(p)[j t mod 2N mod N] = +-p[j], negated when j t mod 2N >= N
    sum_c = 0.0;  for j = 0 .. l-1:  sum_c = sum_c + orc_hadamard(K[e].row(c, j), orc_ifft_i32(digit_j(a')))          c = 0 (b), 1 (a)
    y = (b' + orc_fft_u32(sum_0),  orc_fft_u32(sum_1))
    x <- y   (replace)      or      x <- x + y   (add; wrapping)

A step equals (sigma_t b, 0) + round_oracle.external_product on the TRGSW padded with zero rows, word for word
(tests/test_trlwe_auto_host.py); every word of the device is compared with this (tests/test_gpu_trlwe_auto.py).  Beside it what both of
those files use: the padded TRGSW, the noise bounds of the meaning tests and their world."""
import ctypes as C

import numpy as np

import orc
import round_oracle as ro
from round_oracle import REFERENCE, ROUNDED  # noqa: F401

_f64p, _u32p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
MAX_STEPS, MAX_EXPONENTS = 16, 64


def automorphism(x, t):
    """sigma_t on the last axis of a u32 array: x[.., j] goes to index j t mod 2N mod N, negated when j t mod 2N >= N"""
    x = np.ascontiguousarray(x, np.uint32)
    N = x.shape[-1]
    q = (np.arange(N, dtype=np.int64) * int(t)) % (2 * N)
    out = np.empty_like(x)
    out[..., q % N] = np.where(q < N, x, ~x + np.uint32(1))      # (~x + 1: the wrapping negation)
    return out


def inverse_exponent(N, t):
    """t^-1 mod 2N"""
    return pow(int(t), -1, 2 * int(N))


def spectra(p, plan, words):
    """orc_trgsw_to_fft of switching-key words u32[n_t][l][2][N], polynomial by polynomial: float64 of the same shape, what
    rtfhe_trlwe_ksk_create builds on the device"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    f = np.empty(w.size, np.float64)
    orc.lib().orc_trgsw_to_fft(plan.h, w.ctypes.data_as(_u32p), f.ctypes.data_as(_f64p), w.size // p.N)
    return f.reshape(-1, p.l, 2, p.N)


def step(p, plan, key_f, e, t, row, add, mode):
    """key_f: float64[n_t][l][2][N] (spectra); row: u32[2][N] (b then a).  Returns the row after the step."""
    L = orc.lib()
    N, l = p.N, p.l
    ma, mx = ro.constants(l, p.bgbit, mode)
    row = np.ascontiguousarray(row, np.uint32).reshape(2, N)
    b1, a1 = automorphism(row[0], t), automorphism(row[1], t)
    dec = ro.digits(a1, l, p.bgbit, ma, mx)
    dec_f, had, word = np.empty(N, np.float64), np.empty(N, np.float64), np.empty(N, np.uint32)
    s = [np.zeros(N, np.float64), np.zeros(N, np.float64)]
    for j in range(l):
        L.orc_ifft_i32(plan.h, dec_f.ctypes.data_as(_f64p), dec[j].ctypes.data_as(_i32p))
        for c in range(2):
            krow = np.ascontiguousarray(key_f[e, j, c], np.float64)
            L.orc_hadamard(N, had.ctypes.data_as(_f64p), krow.ctypes.data_as(_f64p), dec_f.ctypes.data_as(_f64p))
            s[c] = s[c] + had
    y = np.empty((2, N), np.uint32)
    for c in range(2):
        L.orc_fft_u32(plan.h, word.ctypes.data_as(_u32p), s[c].ctypes.data_as(_f64p))
        y[c] = word
    y[0] = y[0] + b1
    return row + y if add else y


def program(p, plan, key_f, t_list, rows, entry, add, mode):
    """rows: u32[count][2][N]; entry / add: the call's host lists (add None: all replace).  Returns u32[count][2][N]."""
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 2, p.N)
    out = np.empty_like(rows)
    for g in range(rows.shape[0]):
        x = rows[g]
        for k, e in enumerate(entry):
            x = step(p, plan, key_f, int(e), int(t_list[int(e)]), x, bool(add[k]) if add is not None else False, mode)
        out[g] = x
    return out


def padded_trgsw(p, key_words, e):
    """u32[2][2l][N]: the TRGSW sample whose rows (c, h = b, j) are entry e's rows (j, c) and whose rows (c, h = a, j) are zero"""
    k = np.ascontiguousarray(key_words, np.uint32).reshape(-1, p.l, 2, p.N)
    T = np.zeros((2, 2 * p.l, p.N), np.uint32)
    for c in range(2):
        T[c, :p.l] = k[e, :, c]
    return T


def trivial_key(p, t_list, key_from=None):
    """noiseless trivial rows (-sigma_t(s) g_j, 0): u32[n_t][l][2][N]; key_from None: s = 0, all-zero rows"""
    K = np.zeros((len(t_list), p.l, 2, p.N), np.uint32)
    if key_from is not None:
        for e, t in enumerate(t_list):
            s = automorphism(np.asarray(key_from, np.int32).astype(np.uint32), t).view(np.int32).astype(np.int64)      # 0, +1, -1
            for j in range(p.l):
                K[e, j, 0] = (-(s << (32 - (j + 1) * p.bgbit))) & 0xFFFFFFFF
    return K


def step_variance(N, hw_from, l=3):
    """l N 18.5^2 2^-50 + (hw(key_from) + 1) 2^-38 / 3 + N 2^-50: the key rows' 2^-25 noise through l N balanced 6-bit digits (rms 18.5), the
    rounding error of a' (uniform in +-2^-19) through sigma_t(key_from) and once on its own, and a fresh row's own phase noise -- in the
    rounded mode, torus units squared"""
    return l * N * 18.5 ** 2 * 2.0 ** -50 + (hw_from + 1) * 2.0 ** -38 / 3 + N * 2.0 ** -50


def step_bound(N, hw_from, m=1, l=3):
    """6 sigma of m replace steps in a chain: sqrt(m) times the one-step bound"""
    return 6.0 * float(np.sqrt(m * step_variance(N, hw_from, l)))


def trace_bound(N, hw_from, m, l=3):
    """6 sqrt(V_m) with V_m = 4 V_(m-1) + v, V_0 = 2^-50: every add step doubles what the row carried and adds one step's variance"""
    V, v = 2.0 ** -50, step_variance(N, hw_from, l)
    for _ in range(m):
        V = 4 * V + v
    return 6.0 * float(np.sqrt(V))


def meaning_world(R):
    """The inputs of the meaning tests (tests/test_trlwe_auto_host.py through the restatement, tests/test_gpu_trlwe_auto.py on the device): n = 40,
    N = 1024, two lvl1 keys A and B, a switching key A -> B for t = 1 and automorphism keys under B for {3, N + 1, 2N - 1} and the partial
    trace's {N + 1, N/2 + 1, N/4 + 1, N/8 + 1}; fresh rows of N random 3-bit messages under A and under B."""
    import types
    m = types.SimpleNamespace(MSG_BITS=3, ROWS=2)
    m.rp = R.Params(n=40, N=1024)
    N = m.rp.N
    _, m.keyA, _, _ = R.keygen(m.rp, 0x5A01, want_bk=False, want_ksk=False)
    _, m.keyB, _, _ = R.keygen(m.rp, 0x5A02, want_bk=False, want_ksk=False)
    m.t_rekey = [1]
    m.k_rekey = R.trlwe_ksk_keygen(m.rp, m.keyA, m.keyB, m.t_rekey, seed=0x5A03)
    m.t_auto = [3, N + 1, 2 * N - 1, N // 2 + 1, N // 4 + 1, N // 8 + 1]
    m.k_auto = R.trlwe_ksk_keygen(m.rp, m.keyB, m.keyB, m.t_auto, seed=0x5A04)
    rng = np.random.default_rng(0x5A05)
    m.msgs = rng.integers(0, 1 << m.MSG_BITS, (m.ROWS, N))
    m.plain = R.encode_msgs(m.msgs, m.MSG_BITS)
    m.rowsA = R.encrypt_lut(m.rp, m.keyA, m.plain, seed=0x5A06)
    m.rowsB = R.encrypt_lut(m.rp, m.keyB, m.plain, seed=0x5A07)
    m.hwA, m.hwB = int(np.sum(m.keyA)), int(np.sum(m.keyB))
    m.trace_entries = [1, 3, 4, 5]        # N + 1, N/2 + 1, N/4 + 1, N/8 + 1 in t_auto
    # the rows of the 4-step trace hold the same messages 16 times smaller (m 2^24), so that 16 x a surviving word is the ordinary 3-bit
    # encoding m 2^28 and not 0 mod 2^32: trace_want is non-zero exactly at the coefficients = 0 mod 16
    m.TRACE_STEPS = len(m.trace_entries)
    m.plain_small = R.encode_msgs(m.msgs, m.MSG_BITS + m.TRACE_STEPS)
    m.rows_trace = R.encrypt_lut(m.rp, m.keyB, m.plain_small, seed=0x5A08)
    m.trace_want = np.where(np.arange(N) % (1 << m.TRACE_STEPS) == 0, m.plain, 0).astype(np.uint32)
    assert np.array_equal(m.trace_want[:, ::16], m.plain_small[:, ::16] * np.uint32(16)) and np.count_nonzero(m.trace_want) > N // 32
    return m


def check_trace(R, m, traced, bound):
    """What both meaning tests assert of the traced rows (under key B): every coefficient within `bound` of trace_want; exactly the
    coefficients = 0 mod 16 carry 16 x the (small) message -- they decode to the messages, which are not all zero --, the others decode to 0.
    Returns max error / bound."""
    from kit import torus_err
    N = m.rp.N
    ph = R.trlwe_phase(m.rp, m.keyB, traced)
    ratio = float(np.abs(torus_err(ph, m.trace_want)).max()) / bound
    assert ratio <= 1.0, ratio
    dec = R.decode_msgs(ph, m.MSG_BITS)
    keep = np.arange(N) % (1 << m.TRACE_STEPS) == 0
    assert np.array_equal(dec[:, keep], m.msgs[:, keep]) and m.msgs[:, keep].any() and (dec[:, ~keep] == 0).all()
    assert (m.msgs[:, ~keep] != 0).any()      # ... and something was there to cancel
    return ratio
