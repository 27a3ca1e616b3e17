"""TEST INFRASTRUCTURE: programmable bootstrapping (include/rtfhe.h: rtfhe_pbs_batch, rtfhe_pbs_many_batch, rtfhe_lut_create_encrypted)
restated word for word with the oracle's own building blocks -- negacyclic rotation, CMUX, sample extract, key switch.  oracle_pbs,
oracle_pbs_many and oracle_pbs_enc are what the GPU suite compares the device's words with; the CPU suite holds them to the oracle's gate
bootstrap and to each other (tests/test_pbs_host.py, tests/test_pbs_many_host.py, tests/test_pbs_enc_host.py).  CPU only: numpy and the
`orc` module the callers pass in."""
import ctypes as C

import numpy as np

U32 = 0xFFFFFFFF


def switch_body(word, s, lt=0):
    """the mod switch of a body word at s = SH + lt (tfhe.rs:97): floor, scaled back by 2^lt"""
    return (int(word) >> s) << lt


def switch_mask(word, s, lt=0):
    """the mod switch of a mask word at s = SH + lt (tfhe.rs:107-108): round, the sum wrapping mod 2^32 as the reference's wrapping_add does,
    scaled back by 2^lt"""
    return (((int(word) + (1 << (s - 1))) & U32) >> s) << lt


def oracle_pbs(orc, p, plan, bk_f, ksk, tv, t):
    """rtfhe.h's PBS semantics, word for word with the reference's arithmetic: acc = X^{-bbar} (tv, 0); n CMUX steps; extract; key switch."""
    L = orc.lib()
    N, n = p.N, p.n
    sh = 32 - p.nbit - 1
    t = np.ascontiguousarray(t, np.uint32)
    bbar = switch_body(t[n], sh)
    acc = np.zeros(2 * N, np.uint32)
    acc[:N] = orc.rotate(np.ascontiguousarray(tv, np.uint32), -bbar)
    rot = np.empty(2 * N, np.uint32)
    trgsw = 2 * 2 * p.l * N
    for i in range(n):
        abar = switch_mask(t[i], sh)
        rot[:N] = orc.rotate(acc[:N], abar)
        rot[N:] = orc.rotate(acc[N:], abar)
        bki = np.ascontiguousarray(bk_f[i * trgsw:(i + 1) * trgsw])
        L.orc_cmux(C.byref(p), plan.h, bki.ctypes.data_as(C.POINTER(C.c_double)), None,
                   rot.ctypes.data_as(C.POINTER(C.c_uint32)), acc.ctypes.data_as(C.POINTER(C.c_uint32)),
                   acc.ctypes.data_as(C.POINTER(C.c_uint32)))
    return orc.key_switch(p, ksk, orc.sample_extract(p, acc))


def bk_fft(orc, p, plan, bk_t):
    bk_f = np.empty(bk_t.size, np.float64)
    orc.lib().orc_trgsw_to_fft(plan.h, np.ascontiguousarray(bk_t, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)),
                               bk_f.ctypes.data_as(C.POINTER(C.c_double)), bk_t.size // p.N)
    return bk_f


FUNCS = {
    "identity": lambda m, P: m,
    "square": lambda m, P: (m * m) % (1 << P),
    "succ": lambda m, P: (m + 1) % (1 << P),
    "msb": lambda m, P: int(m >= (1 << (P - 1))),
    "neg": lambda m, P: (-m) % (1 << P),
}


def coef0_after_rotation(tv, k):
    """coefficient 0 of X^{-k} * tv, k in [0, 2N): the negacyclic extension"""
    N = len(tv)
    k %= 2 * N
    return int(tv[k]) if k < N else (-int(tv[k - N])) & U32


def oracle_pbs_many(orc, p, plan, bk_f, ksk, tv, t, n_out):
    """rtfhe.h's many-LUT PBS semantics, word for word with the reference's arithmetic: the mod switch at SH + log2(n_out) scaled back by n_out,
    acc = X^{-bbar} (tv, 0); n CMUX steps; sample extract at 0 .. n_out - 1; key switch.  u32[n_out][n+1]."""
    L = orc.lib()
    N, n = p.N, p.n
    lt = int(n_out).bit_length() - 1
    assert n_out == 1 << lt, "n_out is a power of two"
    s = 32 - p.nbit - 1 + lt
    t = np.ascontiguousarray(t, np.uint32)
    bbar = switch_body(t[n], s, lt)
    acc = np.zeros(2 * N, np.uint32)
    acc[:N] = orc.rotate(np.ascontiguousarray(tv, np.uint32), -bbar)
    rot = np.empty(2 * N, np.uint32)
    trgsw = 2 * 2 * p.l * N
    for i in range(n):
        abar = switch_mask(t[i], s, lt)
        rot[:N] = orc.rotate(acc[:N], abar)
        rot[N:] = orc.rotate(acc[N:], abar)
        bki = np.ascontiguousarray(bk_f[i * trgsw:(i + 1) * trgsw])
        L.orc_cmux(C.byref(p), plan.h, bki.ctypes.data_as(C.POINTER(C.c_double)), None,
                   rot.ctypes.data_as(C.POINTER(C.c_uint32)), acc.ctypes.data_as(C.POINTER(C.c_uint32)),
                   acc.ctypes.data_as(C.POINTER(C.c_uint32)))
    return np.stack([orc.key_switch(p, ksk, orc.sample_extract(p, acc, j)) for j in range(n_out)])


def oracle_pbs_enc(orc, p, plan, bk_f, ksk, trlwe, t, n_out):
    """rtfhe.h's PBS from an encrypted table, word for word with the reference's arithmetic: oracle_pbs_many with the accumulator started
    from both halves of the table row, acc = X^{-bbar} (tb, ta).  trlwe: u32[2][N] (b then a).  u32[n_out][n+1]."""
    L = orc.lib()
    N, n = p.N, p.n
    lt = int(n_out).bit_length() - 1
    assert n_out == 1 << lt, "n_out is a power of two"
    s = 32 - p.nbit - 1 + lt
    t = np.ascontiguousarray(t, np.uint32)
    trlwe = np.ascontiguousarray(trlwe, np.uint32).reshape(2, N)
    bbar = switch_body(t[n], s, lt)
    acc = np.zeros(2 * N, np.uint32)
    acc[:N] = orc.rotate(np.ascontiguousarray(trlwe[0]), -bbar)
    acc[N:] = orc.rotate(np.ascontiguousarray(trlwe[1]), -bbar)
    rot = np.empty(2 * N, np.uint32)
    trgsw = 2 * 2 * p.l * N
    for i in range(n):
        abar = switch_mask(t[i], s, lt)
        rot[:N] = orc.rotate(acc[:N], abar)
        rot[N:] = orc.rotate(acc[N:], abar)
        bki = np.ascontiguousarray(bk_f[i * trgsw:(i + 1) * trgsw])
        L.orc_cmux(C.byref(p), plan.h, bki.ctypes.data_as(C.POINTER(C.c_double)), None,
                   rot.ctypes.data_as(C.POINTER(C.c_uint32)), acc.ctypes.data_as(C.POINTER(C.c_uint32)),
                   acc.ctypes.data_as(C.POINTER(C.c_uint32)))
    return np.stack([orc.key_switch(p, ksk, orc.sample_extract(p, acc, j)) for j in range(n_out)])
