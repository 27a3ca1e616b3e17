#!/usr/bin/env python3
"""examples/nander_adder.py's 8-bit ripple-carry adder on seeded lvl0 ciphertexts (include/rtfhe.h, "seeded lvl0 ciphertexts"): the client ships
its two bytes per replica as a 32-byte public seed and ONE word per encrypted bit, and the whole evaluation key in seeded form -- the
bootstrapping key's b polynomials and one word per key-switching row.  The server loads both keys seeded (rtfhe_load_bk_seeded,
rtfhe_load_ksk_seeded), regenerates every input mask on the GPU straight into the adder's wire table (rtfhe_tlwe_seeded_expand_dev;
k_tlwe_seeded_expand) and runs the NAND-only adder as one graph; the client decrypts.

    python examples/seeded_gates.py [replicas]      # random bytes, checked against their sums
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402
from rustfhe_amd.circuit import CircuitRunner, ripple_carry_adder  # noqa: E402

BITS = 8


def client_inputs(p, key0, a, b, seed=None):
    """bytes a[replicas], b[replicas] -> (seed, b words u32[replicas * 16]): per replica a's bits, least significant first, then b's.  One call,
    one fresh seed, rows numbered from 0.  An integer seed: TEST ONLY, the deterministic form."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    bits = np.concatenate([(a[:, None] >> np.arange(BITS)) & 1, (b[:, None] >> np.arange(BITS)) & 1], axis=1).astype(np.uint8)
    if seed is None:
        return R.encrypt_bits_seeded(p, key0, bits)
    mask = np.random.default_rng(seed).integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
    return R.encrypt_bits_seeded(p, key0, bits, noise_seed=seed, seed=mask)


def server_add(engine, bk, ksk, inputs, replicas):
    """Loads both seeded keys, expands each replica's 16 input rows in place in the wire table (rows 2 .. 17 of the replica's wires; rows
    16 r .. 16 r + 15 of the seed) and runs the adder.  Returns the sum bits' ciphertexts u32[replicas][9][n+1]."""
    import torch
    seed, b = inputs
    engine.load_bk_seeded(*bk)
    engine.load_ksk_seeded(*ksk)
    net = ripple_carry_adder(BITS, True)
    with CircuitRunner(engine, net, replicas) as run:
        st = torch.cuda.current_stream().cuda_stream
        d_b = torch.from_numpy(np.ascontiguousarray(b, np.uint32).view(np.int32)).cuda()
        wires = run.wires.view(replicas, net.num_wires, engine.p.n + 1)
        for r in range(replicas):
            engine.tlwe_seeded_expand_dev(seed, d_b[2 * BITS * r:], wires[r, 2:], 2 * BITS, first_row=2 * BITS * r, stream=st)
        run.run()
        return run.outputs()


def shipped_bytes(p, replicas):
    """(full, seeded) bytes of the inputs and of the evaluation key"""
    rows = 2 * BITS * replicas
    ksk_rows = p.N * p.ks_t * ((1 << p.ks_basebit) - 1)
    full = (rows + ksk_rows) * (p.n + 1) * 4 + p.bk_words * 4
    return full, (rows + ksk_rows) * 4 + p.bk_words * 2 + 3 * 32


def run(p, replicas, seed=None, device=0):
    """`replicas` random pairs of bytes.  Returns (decrypted sums, expected)."""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, replicas), rng.integers(0, 256, replicas)
    key0, _, bk, ksk = R.keygen_seeded(p, seed)
    engine = R.Engine(p, device)
    try:
        out = server_add(engine, bk, ksk, client_inputs(p, key0, a, b, seed), replicas)
    finally:
        engine.close()
    bits = R.decrypt_bits(p, key0, out.reshape(-1, p.n + 1)).reshape(replicas, BITS + 1).astype(np.int64)
    return (bits << np.arange(BITS + 1)).sum(axis=1), a + b


def main():
    replicas = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    p = R.Params()
    got, want = run(p, replicas)
    full, seeded = shipped_bytes(p, replicas)
    print("%d / %d sums right" % (int((got == want).sum()), replicas))
    print("shipped: %d bytes seeded, %d bytes in full (%.3f x)" % (seeded, full, seeded / full))
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
