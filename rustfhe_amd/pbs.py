"""Encoding of small integers for programmable bootstrapping (Engine.pbs_batch, Engine.pbs_many_batch): messages, test polynomials, decoding.

One padding bit: a message m in [0, 2^p) is the torus word m * 2^(32-p-1), so every valid phase lies in the upper half-circle's
complement [0, 1/2) and the blind rotation never needs the negacyclic half of the test polynomial for it.

Why the table below computes f.  A PBS mod-switches the phase to k ~ m * B (+ rounding noise) in Z_2N, with the box width
B = N / 2^p, and coefficient 0 of X^{-k} * tv is

    tv[k]          for 0 <= k < N
    -tv[k - N]     for N <= k < 2N          (X^N = -1)

A message m > 0 lands in k in [m B - B/2, m B + B/2), inside [0, N - B/2): so tv[j] = enc_out(f(floor((j + B/2) / B))) for
j < N - B/2.  Message 0 also lands just below zero, k in [2N - B/2, 2N) = -[N - B/2, N) mod 2N: coefficient 0 is then
-tv[k - N] with k - N in [N - B/2, N), which must be enc_out(f(0)) -- hence tv[j] = -enc_out(f(0)) on the top half-box
j >= N - B/2.  enc_out(v) = v * 2^(32-q-1) with q = out_bits (default p), so that one PBS's output is the next one's input;
raw=True takes f's values as torus words as they are (e.g. +-1/8 = 0x20000000 / 0xE0000000, the gates' encoding).
"""
import numpy as np


def _shift(bits):
    if not 1 <= bits <= 30:
        raise ValueError("message width must be 1..30 bits")
    return 32 - bits - 1


def encode_msgs(msgs, msg_bits):
    """m in [0, 2^msg_bits) -> the torus word m * 2^(32 - msg_bits - 1) (one padding bit), u32."""
    m = np.asarray(msgs, dtype=np.int64)
    if m.size and (m.min() < 0 or m.max() >= (1 << msg_bits)):
        raise ValueError("messages must lie in [0, 2^msg_bits)")
    return (m.astype(np.uint64) << np.uint64(_shift(msg_bits))).astype(np.uint32)


def decode_msgs(phases, msg_bits):
    """Phases (u32 torus words, e.g. from phases()) -> the nearest message in [0, 2^msg_bits)."""
    sh = _shift(msg_bits)
    ph = np.asarray(phases, dtype=np.uint64)
    rounded = ((ph + np.uint64(1 << (sh - 1))) & np.uint64(0xFFFFFFFF)) >> np.uint64(sh)
    return (rounded & np.uint64((1 << msg_bits) - 1)).astype(np.int64)


def lut_polynomial(f, N, msg_bits, out_bits=None, raw=False):
    """The test polynomial (u32[N]) of the function f on messages of msg_bits bits (see the module docstring for the derivation).
    f: a callable on an int, or a sequence of 2^msg_bits values.  Outputs are encoded with out_bits (default msg_bits) or, with
    raw=True, taken as torus words."""
    p = msg_bits
    if (1 << p) > N // 2:
        raise ValueError("a box must hold at least two coefficients: msg_bits <= log2(N) - 1")
    vals = [f(m) for m in range(1 << p)] if callable(f) else list(f)
    if len(vals) != 1 << p:
        raise ValueError("f must give 2^msg_bits values")
    if raw:
        enc = np.array([int(v) & 0xFFFFFFFF for v in vals], dtype=np.uint64)
    else:
        q = p if out_bits is None else out_bits
        if min(vals) < 0 or max(vals) >= (1 << q):
            raise ValueError("f's values must lie in [0, 2^out_bits)")
        enc = np.array(vals, dtype=np.uint64) << np.uint64(_shift(q))
    B = N >> p
    j = np.arange(N)
    box = (j + B // 2) // B
    tv = enc[np.minimum(box, (1 << p) - 1)]
    top = j >= N - B // 2
    tv[top] = (np.uint64(1 << 32) - enc[0]) & np.uint64(0xFFFFFFFF)
    return tv.astype(np.uint32)


def lut_pack_layout(N, msg_bits):
    """(pos, rep) with which Engine.pack_batch turns the 2^msg_bits ciphertexts of enc_out(f(e)), e = 0 .. 2^msg_bits - 1, into an encryption
    of lut_polynomial(f, N, msg_bits): rep = B = N / 2^msg_bits and pos[e] = (e B - B/2) mod 2N, int32.  Box e of the module docstring is
    [e B - B/2, e B + B/2); entry 0's lower half-box starts at 2N - B/2 = X^N * X^(N - B/2), i.e. on the top half-box with the sign flipped."""
    p = msg_bits
    if p < 1 or (1 << p) > N // 2:
        raise ValueError("a box must hold at least two coefficients: 1 <= msg_bits <= log2(N) - 1")
    B = N >> p
    pos = (np.arange(1 << p, dtype=np.int64) * B - B // 2) % (2 * N)
    return pos.astype(np.int32), B


def many_lut_polynomial(fs, N, msg_bits, out_bits=None, raw=False):
    """The test polynomial (u32[N]) of a many-LUT PBS (Engine.pbs_many_batch with n_out = len(fs)): theta = len(fs) functions of the same
    message, interleaved.  Each f in fs is what lut_polynomial takes (a callable or 2^msg_bits values); out_bits and raw apply to all of them.

    Why this computes all of them.  The many-LUT PBS rounds the mod switch to multiples of theta = 2^t: the rotation is k ~ m * B with k a
    multiple of theta (B = N / 2^p as in the module docstring), and output j is coefficient j of X^{-k} * tv,

        tv[k + j]          for 0 <= k + j < N
        -tv[k + j - N]     for N <= k + j < 2N

    so the block of theta coefficients k .. k + theta - 1 carries one value of every function.  If theta divides B / 2 (theta <= N / 2^(p+1)),
    the box edges m B - B/2 are multiples of theta and no block straddles two boxes: a message m > 0 lands in a block inside
    [m B - B/2, m B + B/2), so tv[i] = enc_out(f_{i mod theta}(floor((i - i mod theta + B/2) / B))) for i - i mod theta < N - B/2.  Message 0
    also lands in a block k in [2N - B/2, 2N) (k + j < 2N, since k <= 2N - theta): coefficient j is -tv[k + j - N], k + j - N in
    [N - B/2, N), which must be enc_out(f_j(0)) -- hence tv[i] = -enc_out(f_{i mod theta}(0)) on the top half-box.  In short
    tv[i] = lut_polynomial(f_{i mod theta})[i - i mod theta]: with one function this is lut_polynomial's table exactly.  The coarser rounding
    multiplies the input's mod-switch error by theta (include/rtfhe.h)."""
    fs = list(fs)
    th = len(fs)
    if th not in (1, 2, 4, 8):
        raise ValueError("a many-LUT PBS takes 1, 2, 4 or 8 functions (got %d)" % th)
    if (1 << msg_bits) > N // 2:
        raise ValueError("a box must hold at least two coefficients: msg_bits <= log2(N) - 1")
    if th > N >> (msg_bits + 1):
        raise ValueError("%d functions need half a box of at least %d coefficients: msg_bits <= log2(N) - 1 - log2(len(fs))" % (th, th))
    tabs = [lut_polynomial(f, N, msg_bits, out_bits=out_bits, raw=raw) for f in fs]
    i = np.arange(N)
    base = i - i % th
    tv = np.empty(N, np.uint32)
    for j in range(th):
        tv[j::th] = tabs[j][base[j::th]]
    return tv
