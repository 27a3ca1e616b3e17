"""TEST INFRASTRUCTURE: the PBS family with a choice of gadget decomposition (include/rtfhe.h: rtfhe_set_decomposition), restated from the
oracle's own blocks.  The oracle's external product has the reference's mask built in, so the product is restated here, block by block in
orc_external_product's order:

    digits   orc_decomp_poly(N, (x + MA - MX) mod 2^32, bits, MX, l)    the oracle forms (p + mask) ^ mask, so this is ((x + MA) ^ MX)'s fields
    spectra  orc_ifft_i32 of every digit polynomial
    sum      from 0.0:  sum = sum + orc_hadamard(key row, digit spectrum),  rows in order, per output component
    words    orc_fft_u32(sum)

With MA = MX = make_decomp_mask this is orc_external_product word for word (tests/test_pbs_round_host.py); with the rounded constants it is
what the k_pbs_round_* kernels compute (tests/test_gpu_pbs_round.py)."""
import ctypes as C

import numpy as np

import orc

U32 = 0xFFFFFFFF
REFERENCE, ROUNDED = 0, 1

_f64p, _u32p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


def constants(l, bits, mode):
    """(MA, MX) of u = ((x + MA) mod 2^32) ^ MX."""
    if mode == REFERENCE:
        m = int(orc.lib().orc_make_decomp_mask(l, bits))
        return m, m
    mx = sum(1 << (32 - bits * j + bits - 1) for j in range(1, l + 1))
    return mx + (1 << (32 - l * bits - 1)), mx


def digits(x, l, bits, ma, mx):
    """int32[l][len(x)]: digit j of every word of x."""
    x = np.ascontiguousarray(x, np.uint32)
    shifted = ((x.astype(np.uint64) + ma - mx) & U32).astype(np.uint32)
    out = np.empty((l, x.size), np.int32)
    orc.lib().orc_decomp_poly(x.size, shifted.ctypes.data_as(_u32p), bits, mx, l, out.ctypes.data_as(_i32p))
    return out


def external_product(p, plan, trgsw_f, trlwe, ma, mx):
    """trgsw_f: float64[2][2l][N] spectra of one TRGSW (one bootstrapping-key entry); trlwe: u32[2N] (b then a)."""
    L = orc.lib()
    N, l, rows = p.N, p.l, 2 * p.l
    trlwe = np.ascontiguousarray(trlwe, np.uint32)
    dec = np.concatenate([digits(trlwe[:N], l, p.bgbit, ma, mx), digits(trlwe[N:], l, p.bgbit, ma, mx)])
    dec_f = np.empty((rows, N), np.float64)
    for j in range(rows):
        L.orc_ifft_i32(plan.h, dec_f[j].ctypes.data_as(_f64p), dec[j].ctypes.data_as(_i32p))
    key = np.ascontiguousarray(trgsw_f, np.float64).reshape(2, rows, N)
    out = np.empty(2 * N, np.uint32)
    had = np.empty(N, np.float64)
    for comp in range(2):
        s = np.zeros(N, np.float64)
        for j in range(rows):
            L.orc_hadamard(N, had.ctypes.data_as(_f64p), key[comp, j].ctypes.data_as(_f64p), dec_f[j].ctypes.data_as(_f64p))
            s = s + had
        L.orc_fft_u32(plan.h, out[comp * N:].ctypes.data_as(_u32p), s.ctypes.data_as(_f64p))
    return out


def cmux(p, plan, trgsw_f, rep1, rep0, ma, mx):
    rep1, rep0 = np.ascontiguousarray(rep1, np.uint32), np.ascontiguousarray(rep0, np.uint32)
    return external_product(p, plan, trgsw_f, rep1 - rep0, ma, mx) + rep0


def blind_rotate(p, plan, bk_f, tv, t, n_out=1, mode=ROUNDED):
    """The accumulator u32[2N] after the n CMUX steps of rtfhe_pbs_many_batch.  tv: u32[N] (plain table) or u32[2][N] (encrypted: b then a)."""
    N, n = p.N, p.n
    ma, mx = constants(p.l, p.bgbit, mode)
    lt = int(n_out).bit_length() - 1
    assert n_out == 1 << lt
    s = 32 - p.nbit - 1 + lt
    t = np.ascontiguousarray(t, np.uint32)
    tv = np.ascontiguousarray(tv, np.uint32).reshape(-1, N)
    bbar = (int(t[n]) >> s) << lt
    acc = np.zeros(2 * N, np.uint32)
    acc[:N] = orc.rotate(tv[0], -bbar)
    if tv.shape[0] == 2:
        acc[N:] = orc.rotate(tv[1], -bbar)
    trgsw = 2 * 2 * p.l * N
    rot = np.empty(2 * N, np.uint32)
    for i in range(n):
        abar = (((int(t[i]) + (1 << (s - 1))) & U32) >> s) << lt
        rot[:N] = orc.rotate(acc[:N], abar)
        rot[N:] = orc.rotate(acc[N:], abar)
        acc = cmux(p, plan, bk_f[i * trgsw:(i + 1) * trgsw], rot, acc, ma, mx)
    return acc


def pbs_many(p, plan, bk_f, ksk, tv, t, n_out=1, mode=ROUNDED):
    """u32[n_out][n+1]: rtfhe_pbs_many_batch's rows of one gate in the given decomposition mode (n_out = 1: rtfhe_pbs_batch's word)."""
    acc = blind_rotate(p, plan, bk_f, tv, t, n_out, mode)
    return np.stack([orc.key_switch(p, ksk, orc.sample_extract(p, acc, j)) for j in range(n_out)])


def pbs(p, plan, bk_f, ksk, tv, t, mode=ROUNDED):
    return pbs_many(p, plan, bk_f, ksk, tv, t, 1, mode)[0]
