#!/usr/bin/env python3
"""examples/encrypted_dense_layer.py with the WEIGHTS encrypted too: the server computes a dense layer with a threshold activation on inputs it
cannot read with weights it cannot read.  Each client sends ONE TRLWE (8 KB) of D binary inputs; the model owner -- the key holder -- sends the
weight matrix W [M][D] once as ONE TRGSW sample (48 KB) of the weight polynomial and the bias in the clear.  On one stream, without leaving the
device:

    trlwe_mul_trgsw_batch_dev(accumulate)        row g = bias + W x_g: M dot products in one external product (include/rtfhe.h),
                                                 rounded leveled decomposition
    trlwe_extract_batch_dev(P = M)               M lvl0 ciphertexts of the sums per client
    pbs_batch_dev, table m -> [m >= t]           M lvl0 ciphertexts of the flags (1-bit outputs), rounded decomposition mode

and the key holder decrypts flags only.  Sizes, layout and message space are encrypted_dense_layer.py's: sums are 3-bit PBS messages with the
padding bit clear, weights in {-1, 0, 1} with at most POS = 4 positive and NEG = 3 negative entries per row, bias NEG.

Noise budget at the default parameters (n = 635, N = 1024).  The product is no longer exact: with ||mu||_2^2 <= M (POS + NEG) = 112 the weight
polynomial's TRGSW sample adds
    the product         sqrt(2 l N 18.5^2 2^-50 + ||mu||_2^2 ((N/2 + 1) 2^-38 / 3 + N 2^-50)) <= 2.7e-4: the selector rows' noise through the
                        balanced digits, which does not scale with mu, plus the decomposition's rounding and the client's fresh noise through mu,
    the key switch      rms 2.3e-3 with a mean of -1.8e-3 (measured),
    the mod switch      sqrt((n/2 + 1) / 12) / 2N = 2.5e-3,
3.4e-3 in quadrature.  Half a 3-bit box is 2^-5 = 3.1e-2: less the key switch's mean, 8.6 deviations -- above the 6 this project asks for.

    python examples/private_dense_layer.py [clients] [threshold]
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rustfhe_amd as R  # noqa: E402

_spec = importlib.util.spec_from_file_location("encrypted_dense_layer", os.path.join(HERE, "encrypted_dense_layer.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

MSG_BITS, UNIT, D, M, POS, NEG = base.MSG_BITS, base.UNIT, base.D, base.M, base.POS, base.NEG
KEY_SWITCH_RMS, KEY_SWITCH_MEAN, DEVIATIONS = base.KEY_SWITCH_RMS, base.KEY_SWITCH_MEAN, base.DEVIATIONS
draw_layer, client_rows = base.draw_layer, base.client_rows


def product_sigma(N, mu_norm2, l=3):
    """one term of DESIGN.md 5.17's bound: sqrt(2 l N 18.5^2 2^-50 + ||mu||_2^2 ((N/2 + 1) 2^-38 / 3 + N 2^-50))"""
    return float(np.sqrt(2 * l * N * 18.5 ** 2 * 2.0 ** -50 + mu_norm2 * ((N / 2 + 1) * 2.0 ** -38 / 3 + N * 2.0 ** -50)))


def noise_budget(n, N, W):
    """(sigma of the phase the PBS mod-switches, the margin of half a MSG_BITS box in deviations) from the three figures of the docstring"""
    W = np.asarray(W, dtype=np.int64)
    product = product_sigma(N, float((W ** 2).sum()))
    mod_switch = np.sqrt((n / 2 + 1) / 12.0) / (2 * N)
    sigma = float(np.sqrt(product ** 2 + KEY_SWITCH_RMS ** 2 + mod_switch ** 2))
    return sigma, (2.0 ** -(MSG_BITS + 2) - KEY_SWITCH_MEAN) / sigma


def owner_weights(p, key1, W, seed=None):
    """the model owner's one TRGSW sample of the weight polynomial, and the coefficients the sums arrive at"""
    trgsw, coef = R.dense_layer_trgsw(p, key1, W, D, seed=seed)
    assert trgsw.shape[0] == 1 and coef.size == M
    return trgsw, coef


def server_layer(engine, trgsw, coef, bias, rows, threshold):
    """product (with the bias through accumulate) -> extraction -> PBS on device buffers and one stream; the leveled decomposition and the PBS
    family's are set to rounded around the chain and restored.  Returns the flag ciphertexts u32[clients][M][n+1]."""
    import torch
    p = engine.p
    clients = rows.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    d_x = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32)).cuda()
    d_sums = torch.from_numpy(np.repeat(R.dense_layer_bias(bias, D, p.N, UNIT), clients, axis=0).view(np.int32)).cuda()      # the trivial TRLWE of the bias
    d_lvl0 = torch.zeros((clients * M, p.n + 1), dtype=torch.int32, device="cuda")
    d_flags = torch.zeros((clients * M, p.n + 1), dtype=torch.int32, device="cuda")
    d_s_idx = torch.zeros((clients, 1), dtype=torch.int32, device="cuda")              # the same weights for every client
    tv = R.lut_polynomial(lambda m: int(m >= threshold), p.N, MSG_BITS, out_bits=1)
    before, before_leveled = engine.decomposition(), engine.leveled_decomposition()
    engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
    engine.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with engine.selectors(trgsw) as sel, engine.lut(tv) as lut:
            engine.trlwe_mul_trgsw_batch_dev(sel, d_x, clients, d_sums, clients, 1, d_s_idx, None, True, st)
            engine.trlwe_extract_batch_dev(d_sums, M, d_lvl0, clients, coef=coef, stream=st)
            engine.pbs_batch_dev(lut, d_lvl0, d_flags, clients * M, None, st)
            engine.sync(st)
    finally:
        engine.set_decomposition(before)
        engine.set_leveled_decomposition(before_leveled)
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
    trgsw, coef = owner_weights(p, key1, W, None if seed is None else seed + 1)
    flags_ct = server_layer(engine, trgsw, coef, bias, client_rows(p, key1, x, seed), threshold)
    got = R.decode_msgs(R.phases(p, key0, flags_ct.reshape(-1, p.n + 1)), 1).reshape(clients, M)
    return (sums >= threshold).astype(np.int64), got, sums


def main():
    clients = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    threshold = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    p = R.Params()
    full = np.ones((M, POS + NEG), np.int64)
    sigma, margin = noise_budget(p.n, p.N, full)
    print("budget: product %.2e, key switch %.2e, mod switch %.2e -> sigma %.2e, %.1f deviations in half a %d-bit box"
          % (product_sigma(p.N, float(full.sum())), KEY_SWITCH_RMS, np.sqrt((p.n / 2 + 1) / 12.0) / (2 * p.N), sigma, margin, MSG_BITS))
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    want, got, sums = run(eng, key0, key1, clients, threshold)
    print("%d clients, %d inputs, %d neurons, threshold %d: sums as %d-bit messages, weights TRGSW-encrypted" % (clients, D, M, threshold, MSG_BITS))
    for g in range(clients):
        print("client %d  sums %s  flags %s  decrypted %s" % (g, sums[g].tolist(), want[g].tolist(), got[g].tolist()))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
