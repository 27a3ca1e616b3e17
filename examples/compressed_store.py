#!/usr/bin/env python3
"""Results kept at rest in compressed form and taken up again by another engine (include/rtfhe.h, "compressed results"):

  1. 1,024 2-bit messages go through one programmable bootstrap on the computing engine;
  2. the results leave it twice: as lvl0 rows rounded to 10 bits per word (rtfhe_tlwe_compress_batch_dev), and packed into ONE TRLWE by the
     packing key switch and rounded to 12 bits (rtfhe_trlwe_compress_batch_dev) -- both written to "RTFHECZ1" files (write_compressed);
  3. a fresh engine reads the files (read_compressed), copies the PACKED words up and expands them on the GPU
     (Engine.upload_tlwe_compressed / upload_trlwe_compressed: rtfhe_tlwe_expand_batch_dev / rtfhe_trlwe_expand_batch_dev); the TRLWE goes back
     to 1,024 lvl0 rows through trlwe_extract_batch_dev;
  4. a second bootstrap runs on both forms, and on the rows that never left the device, and the key holder decodes all 1,024 results of each.

Printed per route: the bytes that were stored and crossed the bus per result, how many of the 1,024 decode after the second bootstrap, the noise
of the rows that went INTO the second bootstrap and the noise of its results.  The widths are examples/compressed_results.py's: k = 10 for lvl0
rows and k = 12 for the packed row leave the first bootstrap's sigma of about 0.0098 at 0.0111 and 0.0100, inside the 0.0116 at which a chained
2-bit bootstrap is exact, and every result decodes at them; choosing k stays the caller's job.

    python examples/compressed_store.py
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

RESULTS, MSG_BITS, K_LVL0, K_PACKED = 1024, 2, 10, 12


def f(m):
    return (3 * m + 1) % 4


def _centered(d):
    return (((np.asarray(d, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31) / 2.0 ** 32


def run(engine, reader, key0, key1, pk=None, seed=None, k_lvl0=K_LVL0, k_packed=K_PACKED):
    """The chain on `engine` (computes and stores) and `reader` (loads, expands and computes on), both with both keys loaded; they may be the same
    engine.  pk: a packing key u32[n][t][base-1][2][N] (None: generated here).  Returns one dict per route -- "uncompressed", "lvl0 k=..",
    "packed k=.." --: bytes_per_result, decoded (of RESULTS), noise_in and noise (std of the phase error before and after the second bootstrap,
    of the torus)."""
    import torch
    p, N, n1 = engine.p, engine.p.N, engine.p.n + 1
    assert RESULTS <= N
    rng = np.random.default_rng(seed)
    msgs = rng.integers(0, 1 << MSG_BITS, RESULTS)
    first, second = f(msgs), f(f(msgs))
    ct = R.encrypt_torus(p, key0, R.encode_msgs(msgs, MSG_BITS), seed)
    if pk is None:
        pk = R.packing_keygen(p, key0, key1, seed)
    table = R.lut_polynomial(f, N, MSG_BITS)
    st = torch.cuda.current_stream().cuda_stream
    W0, W1 = R.compressed_words(n1, k_lvl0), R.compressed_words(N + RESULTS, k_packed)
    with tempfile.TemporaryDirectory() as tmp:
        lvl0_file, packed_file = os.path.join(tmp, "results_lvl0.rtfhe"), os.path.join(tmp, "results_packed.rtfhe")
        # the computing side: one bootstrap, both compressed forms to disk; the uncompressed chain goes on in place
        with torch.cuda.device(engine.device), engine.lut(table) as lut, engine.packing_key(pk) as key:
            d_res = torch.empty((RESULTS, n1), dtype=torch.int32, device="cuda")
            d_lvl0 = torch.empty((RESULTS, W0), dtype=torch.int32, device="cuda")
            d_row = torch.empty((1, 2, N), dtype=torch.int32, device="cuda")
            d_packed = torch.empty((1, W1), dtype=torch.int32, device="cuda")
            d_again = torch.empty((RESULTS, n1), dtype=torch.int32, device="cuda")
            engine.pbs_batch_dev(lut, torch.from_numpy(ct.view(np.int32)).cuda(), d_res, RESULTS, None, st)
            engine.tlwe_compress_dev(d_res, k_lvl0, d_lvl0, RESULTS, st)
            engine.pack_batch_dev(key, d_res, RESULTS, d_row, 1, 1, None, st)
            engine.trlwe_compress_dev(d_row, k_packed, RESULTS, d_packed, 1, None, 1, st)
            engine.pbs_batch_dev(lut, d_res, d_again, RESULTS, None, st)
            engine.sync(st)
            R.write_compressed(lvl0_file, d_lvl0.cpu().numpy().view(np.uint32), k_lvl0, n=p.n)
            R.write_compressed(packed_file, d_packed.cpu().numpy().view(np.uint32), k_packed, N=N, coef=np.arange(RESULTS))
            routes = {"uncompressed": (d_res.cpu().numpy().view(np.uint32), d_again.cpu().numpy().view(np.uint32), 4 * n1 * RESULTS)}
        stored = {"lvl0 k=%d" % k_lvl0: os.path.getsize(lvl0_file), "packed k=%d" % k_packed: os.path.getsize(packed_file)}
        # the reading side: nothing but the files; the packed words go up and are expanded on the GPU
        with torch.cuda.device(reader.device), reader.lut(table) as lut:
            st = torch.cuda.current_stream().cuda_stream
            words, k, n, _, _ = R.read_compressed(lvl0_file)
            assert n == reader.p.n
            d_in0 = reader.upload_tlwe_compressed(words, k)
            words, k, _, N_file, coef = R.read_compressed(packed_file)
            assert N_file == N
            d_rows = reader.upload_trlwe_compressed(words, k, len(coef), coef)
            d_in1 = torch.empty((RESULTS, n1), dtype=torch.int32, device="cuda")
            reader.trlwe_extract_batch_dev(d_rows, len(coef), d_in1, 1, coef, 1, st)
            for name, d_in in (("lvl0 k=%d" % k_lvl0, d_in0), ("packed k=%d" % k_packed, d_in1)):
                d_out = torch.empty((RESULTS, n1), dtype=torch.int32, device="cuda")
                reader.pbs_batch_dev(lut, d_in, d_out, RESULTS, None, st)
                reader.sync(st)
                routes[name] = (d_in.cpu().numpy().view(np.uint32), d_out.cpu().numpy().view(np.uint32), stored[name])
    # the key holder's side
    ideal_in, ideal_out = R.encode_msgs(first, MSG_BITS).astype(np.int64), R.encode_msgs(second, MSG_BITS).astype(np.int64)
    res = {}
    for name, (rows_in, rows_out, nbytes) in routes.items():
        ph_in, ph_out = R.phases(p, key0, rows_in), R.phases(p, key0, rows_out)
        res[name] = {"bytes_per_result": nbytes / RESULTS, "decoded": int((R.decode_msgs(ph_out, MSG_BITS) == second).sum()),
                     "noise_in": float(_centered(ph_in.astype(np.int64) - ideal_in).std()),
                     "noise": float(_centered(ph_out.astype(np.int64) - ideal_out).std())}
    return res


def main():
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    engines = []
    try:
        for _ in range(2):                                                           # the one that computes and stores, and a fresh one that reads
            engines.append(R.Engine(p, 0))
            engines[-1].load_bk_torus(bk)
            engines[-1].load_ksk(ksk)
        res = run(engines[0], engines[1], key0, key1)
    finally:
        for e in engines:
            e.close()
    print("widths: k = %d for lvl0 rows, k = %d for the packed row" % (K_LVL0, K_PACKED))
    ok = True
    for name, r in res.items():
        print("%-12s %8.1f bytes per result, %4d / %d decode after the second bootstrap, noise before it %.5f, after it %.5f"
              % (name, r["bytes_per_result"], r["decoded"], RESULTS, r["noise_in"], r["noise"]))
        ok = ok and r["decoded"] == RESULTS
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
