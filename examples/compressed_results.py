#!/usr/bin/env python3
"""1,024 programmable-bootstrap results leave the GPU three ways (include/rtfhe.h, "compressed results"):

  full        as 1,024 lvl0 rows, u32[n+1] each -- the only way before;
  lvl0 k=10   the same rows rounded to 10 bits per word and bit-packed on the GPU (rtfhe_tlwe_compress_batch_dev);
  packed k=12 packed into ONE TRLWE by the packing key switch (rtfhe_pack_batch_dev), then that row's a polynomial and its 1,024 b coefficients
              rounded to 12 bits and bit-packed (rtfhe_trlwe_compress_batch_dev).

Everything runs on one stream and only the small buffers are copied to the host.  The key holder expands on the CPU (rustfhe_amd.tlwe_expand /
trlwe_expand) and decrypts.  Printed per route: bytes per result, how many of the 1,024 messages decode, the measured noise of the results, and
the phase error the compression itself added beside its worst-case bound (h + 1) 2^-(k+1).

    python examples/compressed_results.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

RESULTS, MSG_BITS, K_LVL0, K_PACKED = 1024, 2, 10, 12


def f(m):
    return (3 * m + 1) % 4


def _centered(d):
    return (((np.asarray(d, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31) / 2.0 ** 32


def run(engine, key0, key1, pk=None, seed=None):
    """The three routes on `engine` (both keys loaded).  pk: a packing key u32[n][t][base-1][2][N] (None: generated here).  Returns one dict per
    route: bytes_per_result, decoded (of RESULTS), noise (std of the results' phase error, of the torus), added_max / added_std (what the
    compression added to the phase) and bound."""
    import torch
    p, N, n1 = engine.p, engine.p.N, engine.p.n + 1
    assert RESULTS <= N
    rng = np.random.default_rng(seed)
    msgs = rng.integers(0, 1 << MSG_BITS, RESULTS)
    want = f(msgs)
    ideal = R.encode_msgs(want, MSG_BITS).astype(np.int64)
    ct = R.encrypt_torus(p, key0, R.encode_msgs(msgs, MSG_BITS), seed)
    if pk is None:
        pk = R.packing_keygen(p, key0, key1, seed)
    st = torch.cuda.current_stream().cuda_stream
    W0, W1 = R.compressed_words(n1, K_LVL0), R.compressed_words(N + RESULTS, K_PACKED)
    with torch.cuda.device(engine.device), engine.lut(R.lut_polynomial(f, N, MSG_BITS)) as lut, engine.packing_key(pk) as key:
        d_ct = torch.from_numpy(ct.view(np.int32)).cuda()
        d_res = torch.empty((RESULTS, n1), dtype=torch.int32, device="cuda")
        d_lvl0 = torch.empty((RESULTS, W0), dtype=torch.int32, device="cuda")
        d_row = torch.empty((1, 2, N), dtype=torch.int32, device="cuda")
        d_packed = torch.empty((1, W1), dtype=torch.int32, device="cuda")
        engine.pbs_batch_dev(lut, d_ct, d_res, RESULTS, None, st)
        engine.tlwe_compress_dev(d_res, K_LVL0, d_lvl0, RESULTS, st)
        engine.pack_batch_dev(key, d_res, RESULTS, d_row, 1, 1, None, st)
        engine.trlwe_compress_dev(d_row, K_PACKED, RESULTS, d_packed, 1, None, 1, st)
        engine.sync(st)
        full, lvl0, packed = (t.cpu().numpy().view(np.uint32) for t in (d_res, d_lvl0, d_packed))
        row = d_row.cpu().numpy().view(np.uint32)      # (the uncompressed packed row: read back here only to measure what the compression added)
    # the key holder's side
    h0, h1 = int(np.sum(key0)), int(np.sum(key1))
    ph_full = R.phases(p, key0, full)
    ph_lvl0 = R.phases(p, key0, R.tlwe_expand(p.n, K_LVL0, lvl0))
    ph_row = R.trlwe_phase(p, key1, row)[0, :RESULTS]
    ph_packed = R.trlwe_phase(p, key1, R.trlwe_expand(N, K_PACKED, packed, RESULTS))[0, :RESULTS]

    def route(ph, nbytes, base=None, h=0, k=32):
        added = None if base is None else _centered(ph.astype(np.int64) - base.astype(np.int64))
        return {"bytes_per_result": nbytes / RESULTS, "decoded": int((R.decode_msgs(ph, MSG_BITS) == want).sum()),
                "noise": float(_centered(ph.astype(np.int64) - ideal).std()),
                "added_max": None if added is None else float(np.abs(added).max()), "added_std": None if added is None else float(added.std()),
                "bound": None if base is None else (h + 1) * 2.0 ** -(k + 1)}
    return {"full": route(ph_full, full.nbytes),
            "lvl0 k=%d" % K_LVL0: route(ph_lvl0, lvl0.nbytes, ph_full, h0, K_LVL0),
            "packed k=%d" % K_PACKED: route(ph_packed, packed.nbytes, ph_row, h1, K_PACKED)}


def main():
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    engine = R.Engine(p, 0)
    try:
        engine.load_bk_torus(bk)
        engine.load_ksk(ksk)
        res = run(engine, key0, key1)
    finally:
        engine.close()
    ok = True
    for name, r in res.items():
        line = "%-12s %8.1f bytes per result, %4d / %d decode, noise %.5f" % (name, r["bytes_per_result"], r["decoded"], RESULTS, r["noise"])
        if r["bound"] is not None:
            line += "; compression added max %.5f, spread %.5f (bound %.5f)" % (r["added_max"], r["added_std"], r["bound"])
            ok = ok and r["added_max"] <= r["bound"]
        print(line)
        ok = ok and r["decoded"] == RESULTS
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
