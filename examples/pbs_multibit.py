#!/usr/bin/env python3
"""One 4-bit S-box lookup through the multi-bit blind rotation (include/rtfhe.h: rtfhe_pbs_mb_batch) beside the single-bit PBS: the same
encrypted nibbles through PRESENT's S-box both ways, one gate and 64 gates, with the time of each call.  The multi-bit PBS makes
ceil(n / g) dependent steps where the single-bit one makes n -- 318 instead of 635 at g = 2 -- for a key 1.5 x the size; a single lookup is
bound by that chain, a full batch by the arithmetic, which grows.  Rounded decomposition, as examples/pbs_4bit.py.

    python examples/pbs_multibit.py [g]      # g = 2 (default) or 3
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

MSG_BITS = 4
SBOX = [0xC, 0x5, 0x6, 0xB, 0x9, 0x0, 0xA, 0xD, 0x3, 0xE, 0xF, 0x8, 0x4, 0x7, 0x1, 0x2]


def lookups(engine, mbk, lut, cts, repeat=5):
    """The S-box of every ciphertext both ways: (single-bit words, its best wall time in ms, multi-bit words, its best time)."""
    out = []
    for call in (lambda: engine.pbs_batch(lut, cts), lambda: engine.pbs_mb_batch(mbk, lut, cts)):
        call()                                  # the first call of a size grows the staging buffers
        best, words = None, None
        for _ in range(repeat):
            t0 = time.perf_counter()
            words = call()
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        out += [words, best]
    return tuple(out)


def run(engine, key0, mbk, counts=(1, 64), seed=None):
    """[(count, nibbles, single-bit result, ms, multi-bit result, ms, expected)] in rounded mode; the engine's mode is restored."""
    p, rows = engine.p, []
    before = engine.decomposition()
    with engine.lut(R.lut_polynomial(SBOX, p.N, MSG_BITS)) as lut:
        engine.set_decomposition(R._ffi.DECOMP_ROUNDED)
        try:
            for count in counts:
                x = np.random.default_rng(seed).integers(0, 1 << MSG_BITS, count)
                cts = R.encrypt_torus(p, key0, R.encode_msgs(x, MSG_BITS), seed=seed)
                single, t1, multi, t2 = lookups(engine, mbk, lut, cts)
                rows.append((count, x, R.decode_msgs(R.phases(p, key0, single), MSG_BITS), t1,
                             R.decode_msgs(R.phases(p, key0, multi), MSG_BITS), t2, np.array(SBOX)[x]))
        finally:
            engine.set_decomposition(before)
    return rows


def main():
    g = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    ok = True
    with eng.multibit_key(R.mbk_keygen(p, key0, key1, g), g) as mbk:
        for count, x, single, t1, multi, t2, want in run(eng, key0, mbk):
            print("count %3d: single-bit PBS %7.3f ms (%d right), multi-bit g = %d %7.3f ms (%d right)" %
                  (count, t1, int((single == want).sum()), g, t2, int((multi == want).sum())))
            ok = ok and np.array_equal(multi, want)
    eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
