#!/usr/bin/env python3
"""A two-layer sign network on lvl0 ciphertexts, on the GPU end to end (include/rtfhe.h, "lvl0 dense layers"): a template
matcher over +-1 pixels followed by a code book.

  inputs    I1 = 784 values +-1 per sample at unit u1 = 2^-12, shipped seeded: 4 bytes per value (Engine.upload_tlwe_seeded)
  layer 1   O1 = 32 neurons, weights +-1 (a template each), bias -I1/2: neuron o fires when the sample agrees with template o in more than
            three quarters of its pixels                                                              (Engine.tlwe_dense_batch_dev)
  sign      one bootstrap per neuron in rounded mode, output +-u2 with u2 = 1/8                          (Engine.pbs_batch_dev)
  layer 2   O2 = 8 neurons on the bootstrap outputs as they lie, weights +-1 (bit o of template c's label), bias sum_c W2[o][c]: the
            pre-activation is 2 W2[o][c] for the one template c that fired
  sign      one bootstrap per output bit; optionally the 8 flags of a sample packed into one TRLWE row (Engine.pack_batch) for the way back

Samples are templates with a tenth of their pixels flipped.  The weights stay small on purpose: a layer multiplies its inputs' noise by the
weights' l2 norm, and what a bootstrap hands the second layer carries the key switch's noise -- the example measures both (tlwe_phase against
the clear pre-activations) and prints every margin in deviations; it asserts that each one is at least 6, excludes no sample, and compares the
decrypted labels with the clear network's.

    python examples/dense_sign_network.py [samples] [--pack]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

I1, O1, O2 = 784, 32, 8
U1, U2 = 1 << 20, 1 << 29           # 2^-12 and 1/8 as torus words
MIN_DEVIATIONS = 6.0


def network(seed):
    """(templates +-1 [O1][I1], labels [O1], W1, bias1, W2, bias2): the clear network, integer weights and integer biases"""
    rng = np.random.default_rng(seed)
    templates = rng.choice([-1, 1], (O1, I1))
    labels = rng.permutation(256)[:O1]
    W2 = np.where((labels[None, :] >> np.arange(O2)[:, None]) & 1, 1, -1)            # [O2][O1]
    return templates, labels, templates.astype(np.int32), np.full(O1, -I1 // 2), W2.astype(np.int32), W2.sum(axis=1)


def clear_forward(W1, b1, W2, b2, x):
    """pre-activations and +-1 outputs of both layers on clear +-1 inputs x [samples][I1]"""
    pre1 = x @ W1.T + b1
    h = np.where(pre1 >= 0, 1, -1)
    pre2 = h @ W2.T + b2
    return pre1, h, pre2, np.where(pre2 >= 0, 1, -1)


def signed(words):
    """u32 torus words as fractions in [-1/2, 1/2)"""
    return np.asarray(words, np.uint32).view(np.int32).astype(np.float64) / 2.0 ** 32


def margins(R_, p, key0, out, pre, unit, what):
    """phases of a layer's output against the clear pre-activations: (measured deviation of the noise, smallest margin in deviations).  A
    deviation is the measured one with the bootstrap's own rounding of the n + 1 words to Z_2N added in quadrature, sqrt((n/2 + 1) / 12) / 2N
    for a binary key."""
    ph = R_.phases(p, key0, out.reshape(-1, p.n + 1)).reshape(pre.shape)
    want = ((pre.astype(np.int64) * unit) & 0xFFFFFFFF).astype(np.uint32)
    noise = signed(ph - want)
    sigma = float(np.sqrt((noise ** 2).mean()))
    switch = float(np.sqrt((p.n / 2 + 1) / 12.0) / (2 * p.N))
    dev = float(np.hypot(sigma, switch))
    # distance of the CLEAR pre-activation from the two boundaries of the sign, 0 and 1/2
    frac = signed(want)
    dist = np.minimum(np.abs(frac), 0.5 - np.abs(frac))
    worst = float(dist.min() / dev)
    print("%s: noise %.3e measured over %d phases (largest %.3e), with the bootstrap's rounding %.3e; smallest margin %.4f = %.1f deviations"
          % (what, sigma, noise.size, np.abs(noise).max(), dev, dist.min(), worst))
    return sigma, worst


def run(engine, p, key0, samples, seed=None, key1=None, pk=None):
    """`samples` noisy templates through the encrypted network on `engine` (keys loaded).  Returns (decrypted labels, the clear network's labels,
    the templates' labels, smallest margin of layer 1, of layer 2, packed flags or None)."""
    import torch
    templates, labels, W1, b1, W2, b2 = network(0xD5E if seed is None else seed)
    rng = np.random.default_rng(seed)
    which = rng.integers(0, O1, samples)
    x = templates[which] * np.where(rng.random((samples, I1)) < 0.1, -1, 1)
    pre1, h, pre2, flags = clear_forward(W1, b1, W2, b2, x)
    mu = ((x.reshape(-1).astype(np.int64) * U1) & 0xFFFFFFFF).astype(np.uint32)
    if seed is None:
        mask, b = R.encrypt_torus_seeded(p, key0, mu)
    else:
        mask, b = R.encrypt_torus_seeded(p, key0, mu, noise_seed=seed, seed=np.random.default_rng(seed + 1).integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32))
    n1 = p.n + 1
    st = torch.cuda.current_stream().cuda_stream
    before = engine.decomposition() if hasattr(engine, "decomposition") else None
    engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with engine.dense(W1) as layer1, engine.dense(W2) as layer2, engine.lut(np.full(p.N, U2, np.uint32)) as sign:
            d_x = engine.upload_tlwe_seeded(mask, b)                                     # [samples * I1][n+1]
            d_pre1 = torch.empty((samples, O1, n1), dtype=torch.int32, device="cuda")
            d_h = torch.empty((samples, O1, n1), dtype=torch.int32, device="cuda")
            d_pre2 = torch.empty((samples, O2, n1), dtype=torch.int32, device="cuda")
            d_out = torch.empty((samples, O2, n1), dtype=torch.int32, device="cuda")
            engine.tlwe_dense_batch_dev(layer1, d_x, d_pre1, samples, R.dense_bias(b1, U1), False, st)
            engine.pbs_batch_dev(sign, d_pre1, d_h, samples * O1, None, st)
            engine.tlwe_dense_batch_dev(layer2, d_h, d_pre2, samples, R.dense_bias(b2, U2), False, st)
            engine.pbs_batch_dev(sign, d_pre2, d_out, samples * O2, None, st)
            engine.sync(st)
            words = [t.cpu().numpy().view(np.uint32) for t in (d_pre1, d_pre2, d_out)]
            packed = None
            if pk is not None:                                                           # the 8 flags of a sample on coefficients 0 .. 7 of one row
                d_row = torch.empty((samples, 2, p.N), dtype=torch.int32, device="cuda")
                engine.pack_batch_dev(pk, d_out, O2, d_row, samples, 1, None, st)
                engine.sync(st)
                packed = d_row.cpu().numpy().view(np.uint32)
    finally:
        if before is not None:
            engine.set_decomposition(before)
    _, m1 = margins(R, p, key0, words[0], pre1, U1, "layer 1")
    _, m2 = margins(R, p, key0, words[1], pre2, U2, "layer 2")
    got = signed(R.phases(p, key0, words[2].reshape(-1, n1))).reshape(samples, O2) >= 0
    decrypted = (got.astype(np.int64) << np.arange(O2)).sum(axis=1)
    clear = ((flags > 0).astype(np.int64) << np.arange(O2)).sum(axis=1)
    if packed is not None and key1 is not None:
        ph = signed(R.trlwe_phase(p, key1, packed)[:, :O2]) >= 0
        packed = (ph.astype(np.int64) << np.arange(O2)).sum(axis=1)
    return decrypted, clear, labels[which], m1, m2, packed


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    samples = int(args[0]) if args else 16
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    engine = R.Engine(p, 0)
    pk = None
    try:
        engine.load_bk_torus(bk)
        engine.load_ksk(ksk)
        if "--pack" in sys.argv:
            pk = engine.packing_key(R.packing_keygen(p, key0, key1))
        got, clear, labels, m1, m2, packed = run(engine, p, key0, samples, key1=key1, pk=pk)
    finally:
        if pk is not None:
            pk.close()
        engine.close()
    print("%d / %d labels equal the clear network's, %d / %d the templates'" % (int((got == clear).sum()), samples, int((clear == labels).sum()), samples))
    if packed is not None:
        print("%d / %d packed rows decrypt to the same labels" % (int((packed == clear).sum()), samples))
    ok = np.array_equal(got, clear) and min(m1, m2) >= MIN_DEVIATIONS and (packed is None or np.array_equal(packed, clear))
    assert min(m1, m2) >= MIN_DEVIATIONS, "a pre-activation lies within %.0f deviations of a decision boundary: %.1f, %.1f" % (MIN_DEVIATIONS, m1, m2)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
