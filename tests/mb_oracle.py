"""TEST INFRASTRUCTURE: the multi-bit blind rotation (include/rtfhe.h: rtfhe_pbs_mb_batch) restated in numpy from the oracle's own blocks, as
tests/round_oracle.py restates the single-bit step:

    digits   round_oracle.digits of the accumulator itself (the decomposition mode's constants)
    spectra  orc_ifft_i32 of every digit polynomial
    key      per digit row and component:  K = F_{e_1} B_1;  K = K + F_{e_j} B_j  for j = 2 .. J
    sum      from 0.0:  sum = sum + K * digit spectrum,  rows in order, per output component
    words    acc += orc_fft_u32(sum)

Every product and sum is one numpy operation on float64 arrays, so every one is rounded on its own; a complex product is (rr - ii, ir + ri).
F_e[k] = W[(e q_k) mod 2N] - 1 from the LIBRARY's roots table and point map (rustfhe_amd.mb_roots, mb_point_exponents), the map brought from the
device's point order p = m * 64 + lane to the oracle's spectrum order k = lane * R + m.  Spectra are the oracle's FrrSeries: Re[0 .. N/2) then
Im[0 .. N/2)."""
import ctypes as C

import numpy as np

import orc
import round_oracle as ro

U32 = 0xFFFFFFFF
_f64p, _u32p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


class Tables:
    """W and the point map in the oracle's spectrum order, for one N"""

    def __init__(self, R, N):
        self.N = N
        self.W = R.mb_roots(N)
        q_dev = R.mb_point_exponents(N).astype(np.int64)
        k = np.arange(N // 2)
        rr = N // 128
        self.q = q_dev[(k % rr) * 64 + k // rr]

    def F(self, e):
        """(re, im) of the spectrum of X^e - 1"""
        w = self.W[(int(e) * self.q) % (2 * self.N)]
        return w[:, 0] - 1.0, w[:, 1]


def trgsw_count(n, g):
    return (n // g) * ((1 << g) - 1) + (1 << (n % g)) - 1


def groups(n, g):
    """[(first key bit, bits, first TRGSW)] of every group"""
    out, first = [], 0
    for i0 in range(0, n, g):
        bits = min(g, n - i0)
        out.append((i0, bits, first))
        first += (1 << bits) - 1
    return out


def key_spectra(p, plan, words):
    """float64[n_trgsw][2][2l][N]: the oracle's spectra of a multi-bit key u32[n_trgsw][2][2l][N]"""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1)
    out = np.empty(words.size, np.float64)
    orc.lib().orc_trgsw_to_fft(plan.h, words.ctypes.data_as(_u32p), out.ctypes.data_as(_f64p), words.size // p.N)
    return out.reshape(-1, 2, 2 * p.l, p.N)


def exponents(rs, N):
    """e_j for j = 1 .. 2^len(rs) - 1"""
    return [sum(r for q, r in enumerate(rs) if (j >> q) & 1) % (2 * N) for j in range(1, 1 << len(rs))]


def step(p, plan, tab, key, acc, rs, ma, mx):
    """one group: key float64[J][2][2l][N], acc u32[2N] (b then a), rs the group's rotations"""
    L = orc.lib()
    N, P, l, rows = p.N, p.N // 2, p.l, 2 * p.l
    acc = np.ascontiguousarray(acc, np.uint32)
    dec = np.concatenate([ro.digits(acc[:N], l, p.bgbit, ma, mx), ro.digits(acc[N:], l, p.bgbit, ma, mx)])
    dec_f = np.empty((rows, N), np.float64)
    for r in range(rows):
        L.orc_ifft_i32(plan.h, dec_f[r].ctypes.data_as(_f64p), dec[r].ctypes.data_as(_i32p))
    Fs = [tab.F(e) for e in exponents(rs, N)]
    out = acc.copy()
    for comp in range(2):
        s_re, s_im = np.zeros(P), np.zeros(P)
        for r in range(rows):
            kx = ky = None
            for j, (fx, fy) in enumerate(Fs):
                bx, by = key[j, comp, r, :P], key[j, comp, r, P:]
                ii, rr_, ri, ir = fy * by, fx * bx, fx * by, fy * bx
                if j == 0:
                    kx, ky = rr_ - ii, ir + ri
                else:
                    kx, ky = kx + (rr_ - ii), ky + (ir + ri)
            re, im = dec_f[r, :P], dec_f[r, P:]
            ii, rr_, ri, ir = ky * im, kx * re, kx * im, ky * re
            s_re, s_im = s_re + (rr_ - ii), s_im + (ir + ri)
        s = np.ascontiguousarray(np.concatenate([s_re, s_im]))
        w = np.empty(N, np.uint32)
        L.orc_fft_u32(plan.h, w.ctypes.data_as(_u32p), s.ctypes.data_as(_f64p))
        out[comp * N:(comp + 1) * N] += w
    return out


def rotations(p, t):
    """(bbar, [abar_i]) of the single-bit PBS's mod switch"""
    s = 32 - p.nbit - 1
    t = np.ascontiguousarray(t, np.uint32)
    return int(t[p.n]) >> s, [((int(t[i]) + (1 << (s - 1))) & U32) >> s for i in range(p.n)]


def blind_rotate(p, plan, tab, key_f, tv, t, g, mode=ro.REFERENCE):
    """the accumulator u32[2N] after the ceil(n / g) steps"""
    N = p.N
    ma, mx = ro.constants(p.l, p.bgbit, mode)
    bbar, abar = rotations(p, t)
    acc = np.zeros(2 * N, np.uint32)
    acc[:N] = orc.rotate(np.ascontiguousarray(tv, np.uint32), -bbar)
    for i0, bits, first in groups(p.n, g):
        acc = step(p, plan, tab, key_f[first:first + (1 << bits) - 1], acc, abar[i0:i0 + bits], ma, mx)
    return acc


def pbs_mb(p, plan, tab, key_f, ksk, tv, t, g, mode=ro.REFERENCE):
    """u32[n+1]: rtfhe_pbs_mb_batch's row of one gate"""
    return orc.key_switch(p, ksk, orc.sample_extract(p, blind_rotate(p, plan, tab, key_f, tv, t, g, mode), 0))


def plant(p, t, rs):
    """a copy of the ciphertext t whose first len(rs) mask words mod-switch to the rotations rs"""
    s = 32 - p.nbit - 1
    t = np.array(t, np.uint32)
    for i, r in enumerate(rs):
        t[i] = (int(r) << s) & U32
    return t
