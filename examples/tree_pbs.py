#!/usr/bin/env python3
"""A 4-bit function in five bootstraps by tree PBS (include/rtfhe.h: rtfhe_pack_batch_dev, rtfhe_lut_update_dev).  The input is two 2-bit
digits (hi, lo), each a TLWE.  Stage 1 bootstraps lo once per sub-table f(h, .), h = 0 .. 3; stage 2 packs the four outputs into one TRLWE
row -- the test polynomial of h -> f(h, lo), which the server now holds encrypted without having learnt lo --; stage 3 writes the row into
an encrypted table in place; stage 4 bootstraps hi with its own row.  One PBS with a plain table stops at 2-3 bits at N = 1024.  Every stage
works on device buffers; nothing passes through the host in between.

    python examples/tree_pbs.py [inputs]      # a random function, random inputs, checked against the plaintext function, with the time per evaluation
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

DIGIT_BITS = 2


def run(engine, pack_key, key0, f, hi, lo, seed=None):
    """f: int[4][4] with values in [0, 4); hi, lo: the digits of every input.  Returns (decrypted f(hi, lo), seconds per evaluation)."""
    import torch
    p, G, D = engine.p, len(hi), 1 << DIGIT_BITS
    st = torch.cuda.current_stream().cuda_stream
    dev = lambda a, dt=np.uint32: torch.from_numpy(np.ascontiguousarray(a, dt).view(np.int32)).cuda()      # noqa: E731
    c_hi = R.encrypt_torus(p, key0, R.encode_msgs(hi, DIGIT_BITS), seed=seed)
    c_lo = R.encrypt_torus(p, key0, R.encode_msgs(lo, DIGIT_BITS), seed=None if seed is None else seed + 1)
    pos, rep = R.lut_pack_layout(p.N, DIGIT_BITS)
    sub_tables = np.stack([R.lut_polynomial([int(v) for v in f[h]], p.N, DIGIT_BITS) for h in range(D)])
    with engine.lut(sub_tables) as sub, engine.lut_encrypted(np.zeros((G, 2, p.N), np.uint32)) as rows:
        d_lo = dev(np.repeat(c_lo, D, axis=0))                      # input g once per sub-table
        d_sub_idx = dev(np.tile(np.arange(D, dtype=np.int32), G), np.int32)
        d_hi, d_own = dev(c_hi), dev(np.arange(G, dtype=np.int32), np.int32)
        d_s1 = torch.zeros((G * D, p.n + 1), dtype=torch.int32, device="cuda")
        d_rows = torch.zeros((G, 2, p.N), dtype=torch.int32, device="cuda")
        d_out = torch.zeros((G, p.n + 1), dtype=torch.int32, device="cuda")

        def evaluate():
            engine.pbs_batch_dev(sub, d_lo, d_s1, G * D, d_sub_idx, st)          # enc(f(h, lo)) for every h
            engine.pack_batch_dev(pack_key, d_s1, D, d_rows, G, rep, pos, st)   # one row per input: the table of h -> f(h, lo)
            rows.update_dev(d_rows, 0, G, st)
            engine.pbs_batch_dev(rows, d_hi, d_out, G, d_own, st)               # f(hi, lo)
            engine.sync(st)
        evaluate()                                                  # first call: buffers are allocated
        t0 = time.perf_counter()
        evaluate()
        dt = time.perf_counter() - t0
        out = d_out.cpu().numpy().view(np.uint32)
    return R.decode_msgs(R.phases(p, key0, out), DIGIT_BITS), dt / G


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    pk = R.packing_keygen(p, key0, key1)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    rng = np.random.default_rng()
    f = rng.integers(0, 4, (4, 4))
    hi, lo = rng.integers(0, 4, count), rng.integers(0, 4, count)
    with eng.packing_key(pk) as key:
        got, per = run(eng, key, key0, f, hi, lo)
    want = f[hi, lo]
    print("%d / %d evaluations of a 4-bit function right; %.1f us per evaluation (5 bootstraps and one packing key switch each)"
          % (int((got == want).sum()), count, per * 1e6))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
