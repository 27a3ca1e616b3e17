#!/usr/bin/env python3
"""A 4-bit S-box on encrypted nibbles in ONE programmable bootstrap each (include/rtfhe.h: rtfhe_set_decomposition).  With the reference's gadget
decomposition a bootstrapped ciphertext at n = 635, N = 1024 carries sigma = 0.011 of the torus and a 4-bit box (half width 1/64) fails about one
time in five; the rounded decomposition brings sigma to 0.0028, more than five sigma inside the box.  The S-box is PRESENT's.

    python examples/pbs_4bit.py [nibbles]      # random nibbles through the S-box in rounded mode, checked against the plaintext
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

MSG_BITS = 4
SBOX = [0xC, 0x5, 0x6, 0xB, 0x9, 0x0, 0xA, 0xD, 0x3, 0xE, 0xF, 0x8, 0x4, 0x7, 0x1, 0x2]


def encrypt_nibbles(p, key0, x, seed=None):
    return R.encrypt_torus(p, key0, R.encode_msgs(np.asarray(x, np.int64), MSG_BITS), seed=seed)


def sbox_batch(engine, cts, rounded=True):
    """One PBS per ciphertext through the S-box table, in rounded mode (or, for comparison, the reference's); the engine's mode is restored."""
    before = engine.decomposition()
    with engine.lut(R.lut_polynomial(SBOX, engine.p.N, MSG_BITS)) as lut:
        engine.set_decomposition(R._ffi.DECOMP_ROUNDED if rounded else R._ffi.DECOMP_REFERENCE)
        try:
            return engine.pbs_batch(lut, cts)
        finally:
            engine.set_decomposition(before)


def decode(p, key0, out):
    return R.decode_msgs(R.phases(p, key0, out), MSG_BITS)


def run(engine, key0, count, seed=None, rounded=True):
    """`count` random nibbles through the S-box.  Returns (x, result, expected)."""
    x = np.random.default_rng(seed).integers(0, 1 << MSG_BITS, count)
    out = sbox_batch(engine, encrypt_nibbles(engine.p, key0, x, seed=seed), rounded)
    return x, decode(engine.p, key0, out), np.array(SBOX)[x]


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    x = np.random.default_rng().integers(0, 1 << MSG_BITS, count)
    cts = encrypt_nibbles(p, key0, x)
    want = np.array(SBOX)[x]
    got = decode(p, key0, sbox_batch(eng, cts))
    ref = decode(p, key0, sbox_batch(eng, cts, rounded=False))      # the same ciphertexts
    print("rounded decomposition:   %d / %d nibbles right" % (int((got == want).sum()), count))
    print("reference decomposition: %d / %d nibbles right" % (int((ref == want).sum()), count))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
