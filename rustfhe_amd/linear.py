"""Encrypted linear layers on the exact TRLWE x plain-polynomial product (include/rtfhe.h: rtfhe_trlwe_mul_plain_batch): the
layout that turns one product into up to N/d dot products of length d, and the matching input encoder.  Host-side numpy only.

A client's row holds x_0 .. x_{d-1} in coefficients 0 .. d-1.  Row r of a weight polynomial is written BACKWARDS into coefficients
r d .. r d + d - 1, w[r d + d - 1 - i] = W[r][i], so that coefficient r d + d - 1 of w * x is exactly sum_i W[r][i] x_i: the only pairs
(a, b) with a + b = r d + d - 1 and b < d have a inside row r's block, and a wrapped pair a + b - N <= d - 2 never reaches a read coefficient.
"""
import numpy as np


def dense_layer_polys(W, d, N=1024):
    """W: integer matrix [m][d], d dividing N.  Returns (polys, coef): polys int32[ceil(m / (N/d))][N], polynomial q holding rows
    q N/d .. of W, and coef int32[min(m, N/d)], the coefficients r d + d - 1 to read with trlwe_extract_batch: sample p of the product with
    polynomial q is the dot product of row q N/d + p."""
    W = np.asarray(W)
    assert W.ndim == 2 and W.shape[1] == d, "W must be [m][d]"
    assert np.issubdtype(W.dtype, np.integer), "integer weights"
    assert d >= 1 and N % d == 0, "d must divide N"
    assert W.size == 0 or (np.abs(W.astype(np.int64)).max() < 1 << 31), "weights must fit int32"
    m, per = W.shape[0], N // d
    assert m >= 1, "at least one row"
    n_poly = (m + per - 1) // per
    polys = np.zeros((n_poly, N), np.int32)
    for j in range(m):
        q, r = divmod(j, per)
        polys[q, r * d:(r + 1) * d] = W[j, ::-1]
    coef = (np.arange(min(m, per), dtype=np.int32) * d + d - 1).astype(np.int32)
    return polys, coef


def dense_layer_trgsw(rp, key1, W, d, seed=None):
    """dense_layer_polys with the weights encrypted by the key holder: (trgsw, coef), trgsw u32[n_poly][2][2l][N] the TRGSW encryptions under
    key1 of the weight polynomials (encrypt_trgsw_polys; Engine.selectors uploads them, Engine.trlwe_mul_trgsw_batch multiplies), coef as
    dense_layer_polys gives it.  seed: encrypt_trgsw_polys's (None in production)."""
    from .client import encrypt_trgsw_polys
    polys, coef = dense_layer_polys(W, d, rp.N)
    return encrypt_trgsw_polys(rp, key1, polys, seed), coef


def dense_layer_input(x, d, N=1024, unit=1):
    """The plain polynomial a client encrypts (encrypt_lut): x_i * unit in coefficient i < d, zero elsewhere; u32[..][N] for x of shape [..][d]."""
    x = np.asarray(x).astype(np.int64)
    assert x.shape[-1] == d and d <= N
    out = np.zeros(x.shape[:-1] + (N,), np.int64)
    out[..., :d] = x * int(unit)
    return (out & 0xFFFFFFFF).astype(np.uint32)


def dense_layer_bias(bias, d, N=1024, unit=1):
    """The trivial TRLWE rows (bias in b, 0 in a) to initialise the product's output with under accumulate: bias[j] * unit in coefficient
    r d + d - 1 of polynomial q's row, (q, r) = divmod(j, N/d); u32[n_poly][2][N]."""
    bias = np.asarray(bias).astype(np.int64).reshape(-1)
    per = N // d
    rows = np.zeros(((bias.size + per - 1) // per, 2, N), np.int64)
    for j, b in enumerate(bias):
        q, r = divmod(j, per)
        rows[q, 0, r * d + d - 1] = int(b) * int(unit)
    return (rows & 0xFFFFFFFF).astype(np.uint32)


def dense_bias(b, unit):
    """The torus words of integer biases at a message unit, for Engine.tlwe_dense_batch[_dev] (include/rtfhe.h: rtfhe_tlwe_dense_batch; DESIGN.md
    5.20): b[o] * unit mod 2^32, u32[O].  `unit` is the torus word of message 1 (e.g. 1 << 27 for 1/32)."""
    b = np.asarray(b)
    assert b.size == 0 or np.issubdtype(b.dtype, np.integer), "integer biases"
    return np.array([(int(v) * int(unit)) & 0xFFFFFFFF for v in b.reshape(-1)], np.uint32)
