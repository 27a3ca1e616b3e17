#!/usr/bin/env python3
"""An encrypted dense layer with a threshold activation, computed by the SERVER on inputs it cannot read.  Each client sends ONE TRLWE (8 KB)
of D binary inputs; the server holds an integer weight matrix W [M][D] and a bias in the clear.  On one stream, without leaving the device:

    trlwe_mul_plain_batch_dev(accumulate)        row g = bias + W x_g: M dot products in one exact product (include/rtfhe.h)
    trlwe_extract_batch_dev(P = M)               M lvl0 ciphertexts of the sums per client
    pbs_batch_dev, table m -> [m >= t]           M lvl0 ciphertexts of the flags (1-bit outputs), rounded decomposition mode

and the key holder decrypts flags only -- never an input, never a sum.

Sized as examples/histogram_threshold.py: a sum is a 3-bit PBS message with its padding bit clear, unit encode_msgs(1, 3) = 2^-4.  The weights
are in {-1, 0, 1} with at most POS = 4 positive and NEG = 3 negative entries per row and the bias is NEG, so that bias + W x stays in [0, 7]
for every binary x.  The layout is rustfhe_amd.dense_layer_polys: D = 8 inputs in coefficients 0 .. 7, row r of W backwards in coefficients
8 r .. 8 r + 7, its dot product at coefficient 8 r + 7.

Noise budget at the default parameters (n = 635, N = 1024), from the figures the project already has.  What the PBS's mod switch sees is the
sum plus
    the product         ||w||_2 2^-25 <= sqrt(M (POS + NEG)) 2^-25 = 3.2e-7: the clients' fresh noise (sigma 2^-25) scaled by the weights -- the
                        product itself adds nothing --, with a mean of at most ||w||_1 2^-28.7 = 2.6e-7 (the sampler's documented mean),
    the key switch      rms 2.3e-3 with a mean of -1.8e-3 (measured),
    the mod switch      sqrt((n/2 + 1) / 12) / 2N = 2.5e-3,
3.4e-3 in quadrature.  Half a 3-bit box is 2^-5 = 3.1e-2: less the two means, 8.6 deviations -- above the 6 this project asks for.  The flag is
a 1-bit output (half a box 1/8) behind a rounded-mode PBS whose output noise is 3.0e-3: 40 deviations.

    python examples/encrypted_dense_layer.py [clients] [threshold]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

MSG_BITS = 3                        # a sum is a 3-bit message: bias + W x in [0, 7]
UNIT = 1 << (32 - MSG_BITS - 1)     # encode_msgs(1, 3) = 2^-4
D, M = 8, 16                        # inputs per client, neurons
POS, NEG = 4, 3                     # at most that many +1 / -1 weights per row; the bias NEG keeps every sum non-negative
FRESH_SIGMA, FRESH_MEAN = 2.0 ** -25, 2.0 ** -28.7        # a fresh TRLWE's noise (encrypt_lut) and the sampler's documented mean
KEY_SWITCH_RMS, KEY_SWITCH_MEAN = 2.3e-3, 1.8e-3          # DESIGN.md 5.12, measured at n = 635, N = 1024
DEVIATIONS = 6.0


def noise_budget(n, N, W):
    """(sigma of the phase the PBS mod-switches, the margin of half a MSG_BITS box in deviations) from the three figures of the docstring"""
    W = np.asarray(W, dtype=np.int64)
    product = float(np.sqrt((W ** 2).sum())) * FRESH_SIGMA
    product_mean = float(np.abs(W).sum()) * FRESH_MEAN
    mod_switch = np.sqrt((n / 2 + 1) / 12.0) / (2 * N)
    sigma = float(np.sqrt(product ** 2 + KEY_SWITCH_RMS ** 2 + mod_switch ** 2))
    return sigma, (2.0 ** -(MSG_BITS + 2) - KEY_SWITCH_MEAN - product_mean) / sigma


def draw_layer(rng):
    """(W int[M][D] in {-1, 0, 1} with at most POS positive and NEG negative entries per row, bias int[M] = NEG)"""
    W = np.zeros((M, D), np.int64)
    for r in range(M):
        at = rng.permutation(D)
        n_pos, n_neg = rng.integers(1, POS + 1), rng.integers(0, NEG + 1)
        W[r, at[:n_pos]] = 1
        W[r, at[n_pos:n_pos + n_neg]] = -1
    return W, np.full(M, NEG, np.int64)


def client_rows(p, key1, x, seed=None):
    """every client's one TRLWE of its D binary inputs: u32[clients][2][N]"""
    return R.encrypt_lut(p, key1, R.dense_layer_input(x, D, p.N, UNIT), seed=seed)


def server_layer(engine, W, bias, rows, threshold):
    """product (with the bias through accumulate) -> extraction -> PBS on device buffers and one stream; the decomposition mode of the PBS family
    is set to rounded around the bootstrap and restored.  Returns the flag ciphertexts u32[clients][M][n+1]."""
    import torch
    p = engine.p
    clients = rows.shape[0]
    polys, coef = R.dense_layer_polys(W, D, p.N)
    assert polys.shape[0] == 1 and coef.size == M
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32)).cuda()
    d_sums = torch.from_numpy(np.repeat(R.dense_layer_bias(bias, D, p.N, UNIT), clients, axis=0).view(np.int32)).cuda()      # the trivial TRLWE of the bias
    d_lvl0 = torch.zeros((clients * M, p.n + 1), dtype=torch.int32, device="cuda")
    d_flags = torch.zeros((clients * M, p.n + 1), dtype=torch.int32, device="cuda")
    d_w_idx = torch.zeros((clients, 1), dtype=torch.int32, device="cuda")              # the same weights for every client
    tv = R.lut_polynomial(lambda m: int(m >= threshold), p.N, MSG_BITS, out_bits=1)
    before = engine.decomposition()
    engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with engine.plain_polys(polys) as pp, engine.lut(tv) as lut:
            engine.trlwe_mul_plain_batch_dev(pp, d_x, clients, d_sums, clients, 1, d_w_idx, None, True, st)
            engine.trlwe_extract_batch_dev(d_sums, M, d_lvl0, clients, coef=coef, stream=st)
            engine.pbs_batch_dev(lut, d_lvl0, d_flags, clients * M, None, st)
            engine.sync(st)
    finally:
        engine.set_decomposition(before)
    return d_flags.cpu().numpy().view(np.uint32).reshape(clients, M, p.n + 1)


def run(engine, key0, key1, clients=4, threshold=4, seed=None):
    """`clients` inputs through the whole protocol on an engine that holds the bootstrapping and the key-switching key of (key0, key1).
    Returns (the clear flags [bias + W x >= threshold], the decrypted flags, the clear sums), each [clients][M]."""
    rng = np.random.default_rng(seed)
    p = engine.p
    W, bias = draw_layer(rng)
    _, margin = noise_budget(p.n, p.N, W)
    assert margin >= DEVIATIONS, "half a %d-bit box keeps only %.1f deviations at these parameters: lower MSG_BITS" % (MSG_BITS, margin)
    x = rng.integers(0, 2, (clients, D))
    sums = x @ W.T + bias
    assert sums.min() >= 0 and sums.max() < 1 << MSG_BITS
    flags_ct = server_layer(engine, W, bias, client_rows(p, key1, x, seed), threshold)
    got = R.decode_msgs(R.phases(p, key0, flags_ct.reshape(-1, p.n + 1)), 1).reshape(clients, M)
    return (sums >= threshold).astype(np.int64), got, sums


def main():
    clients = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    threshold = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    want, got, sums = run(eng, key0, key1, clients, threshold)
    print("%d clients, %d inputs, %d neurons, threshold %d: sums as %d-bit messages" % (clients, D, M, threshold, MSG_BITS))
    for g in range(clients):
        print("client %d  sums %s  flags %s  decrypted %s" % (g, sums[g].tolist(), want[g].tolist(), got[g].tolist()))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
