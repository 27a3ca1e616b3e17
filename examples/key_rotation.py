#!/usr/bin/env python3
"""Key rotation on the GPU, and a partial trace (include/rtfhe.h, "TRLWE key switching"):

  1. a key holder with key set A has data at rest on a server: an encrypted table of 2-bit functions (rustfhe_amd.encrypt_lut, the rows of
     Engine.lut_encrypted) and a TRLWE row of packed 2-bit results -- both TRLWE rows under A's lvl1 key, tied to it for life;
  2. the holder rotates to key set B.  Instead of downloading, decrypting, re-encrypting and uploading everything, it sends ONE switching key
     from A to B (rustfhe_amd.trlwe_ksk_keygen with t = [1]: l TRLWE rows) and the server re-keys every row on the GPU
     (Engine.trlwe_auto_batch_dev, one launch);
  3. the server runs a programmable bootstrap with B's bootstrapping key over the re-keyed table (Engine.pbs_batch_dev) on inputs encrypted
     under B;
  4. everything decodes under B -- the bootstrap's results, the re-keyed packed row -- and nothing decodes under A any more;
  5. then, with automorphism keys under B (key_from = key_to = B's lvl1 key), a 3-step partial trace of the packed row: x <- x + sigma_t(x) for
     t = N + 1, N/2 + 1, N/4 + 1 keeps every 8th coefficient, times 8, and cancels the others.  Printed: which coefficients survive.

The switch runs in the rounded leveled decomposition (one step adds phase noise of about 4e-5 of the torus), which this script
selects for the call and puts back.

    python examples/key_rotation.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

MSG_BITS, TABLES, TRACE_STEPS = 2, 4, 3
PACKED_BITS = MSG_BITS + TRACE_STEPS      # the packed row holds its 2-bit messages 2^TRACE_STEPS times smaller: the trace multiplies by that


def draw_functions(rng):
    """TABLES secret functions of a 2-bit message"""
    return rng.integers(0, 1 << MSG_BITS, (TABLES, 1 << MSG_BITS))


def run(engine, key1_a, key0_b, key1_b, rows=1024, seed=None):
    """engine: a context with key set B loaded (bootstrapping and key-switching key).  key1_a: A's lvl1 key -- A needs nothing else here, the
    data at rest are TRLWE rows.  rows: the inputs of the bootstrap; the packed row always holds N messages.  Returns a dict: what the
    bootstrap gave and should give under B, the packed row's messages decoded under B and under A, the share of the table's coefficients that
    still decode under A, the phase of the traced row and what it should be."""
    import torch
    p, N, n1 = engine.p, engine.p.N, engine.p.n + 1
    rng = np.random.default_rng(seed)
    sub = (lambda k: None if seed is None else seed + k)
    funcs = draw_functions(rng)
    # 1. data at rest under A
    table_plain = np.stack([R.lut_polynomial([int(v) for v in f], N, MSG_BITS) for f in funcs])
    table_a = R.encrypt_lut(p, key1_a, table_plain, seed=sub(1))
    packed_msgs = rng.integers(0, 1 << MSG_BITS, N)                        # a full row, whatever `rows` is
    packed_a = R.encrypt_lut(p, key1_a, R.encode_msgs(packed_msgs, PACKED_BITS), seed=sub(2))
    # 2. the keys the holder sends: A -> B for t = 1, and automorphism keys under B for the trace
    rekey_words = R.trlwe_ksk_keygen(p, key1_a, key1_b, [1], seed=sub(3))
    trace_t = R.trace_exponents(N, TRACE_STEPS)
    trace_words = R.trlwe_ksk_keygen(p, key1_b, key1_b, trace_t, seed=sub(4))
    # inputs of the bootstrap, under B
    x = rng.integers(0, 1 << MSG_BITS, rows)
    which = rng.integers(0, TABLES, rows).astype(np.int32)
    cts = R.encrypt_torus(p, key0_b, R.encode_msgs(x, MSG_BITS), sub(5))

    st = torch.cuda.current_stream().cuda_stream
    before = engine.leveled_decomposition()
    engine.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED)
    try:
        with torch.cuda.device(engine.device), engine.trlwe_switch_key(rekey_words, [1]) as rekey, engine.trlwe_switch_key(trace_words, trace_t) as trace:
            d_rows = torch.from_numpy(np.concatenate([table_a, packed_a]).view(np.int32)).cuda()      # everything at rest, one batch
            engine.trlwe_auto_batch_dev(rekey, d_rows, d_rows, TABLES + 1, [0], None, st)              # in place: one launch
            engine.sync(st)
            rows_b = d_rows.cpu().numpy().view(np.uint32)
            # 3. a bootstrap with B's keys over the re-keyed table
            with engine.lut_encrypted(rows_b[:TABLES]) as lut:
                d_out = torch.empty((rows, n1), dtype=torch.int32, device="cuda")
                engine.pbs_batch_dev(lut, torch.from_numpy(cts.view(np.int32)).cuda(), d_out, rows, torch.from_numpy(which).cuda(), st)
                engine.sync(st)
                out = d_out.cpu().numpy().view(np.uint32)
            # 5. the partial trace of the re-keyed packed row
            d_tr = torch.empty((1, 2, N), dtype=torch.int32, device="cuda")
            engine.trlwe_auto_batch_dev(trace, d_rows[TABLES:], d_tr, 1, list(range(TRACE_STEPS)), [1] * TRACE_STEPS, st)
            engine.sync(st)
            traced = d_tr.cpu().numpy().view(np.uint32)
    finally:
        engine.set_leveled_decomposition(before)

    # 4. the key holder's side
    res = {"want": funcs[which, x], "got": R.decode_msgs(R.phases(p, key0_b, out), MSG_BITS)}
    res["packed_want"] = packed_msgs
    res["packed_under_b"] = R.decode_msgs(R.trlwe_phase(p, key1_b, rows_b[TABLES:])[0], PACKED_BITS)
    res["packed_under_a"] = R.decode_msgs(R.trlwe_phase(p, key1_a, rows_b[TABLES:])[0], PACKED_BITS)
    ph_a = R.trlwe_phase(p, key1_a, rows_b[:TABLES])
    res["table_words_under_a"] = float(np.mean(R.decode_msgs(ph_a, MSG_BITS) == R.decode_msgs(table_plain, MSG_BITS)))
    # a surviving coefficient carries 2^steps x its word: the packed row's small encoding becomes the ordinary 2-bit one
    scale = 1 << TRACE_STEPS
    res["trace_phase"] = R.trlwe_phase(p, key1_b, traced)[0]
    res["trace_want"] = np.where(np.arange(N) % scale == 0, R.encode_msgs(packed_msgs, MSG_BITS), 0).astype(np.uint32)
    return res


def main():
    p = R.Params()
    _, key1_a, _, _ = R.keygen(p, want_bk=False, want_ksk=False)          # key set A: only its lvl1 key matters here
    key0_b, key1_b, bk_b, ksk_b = R.keygen(p)                             # key set B
    engine = R.Engine(p, 0)
    try:
        engine.load_bk_torus(bk_b)
        engine.load_ksk(ksk_b)
        res = run(engine, key1_a, key0_b, key1_b)
    finally:
        engine.close()
    N = p.N
    ok_pbs = int((res["got"] == res["want"]).sum())
    ok_b = int((res["packed_under_b"] == res["packed_want"]).sum())
    ok_a = int((res["packed_under_a"] == res["packed_want"]).sum())
    print("bootstrap over the re-keyed table, B's keys: %d / %d results decode under B" % (ok_pbs, res["want"].size))
    print("re-keyed packed row: %d / %d messages decode under B, %d / %d under A (chance: %d)" % (ok_b, N, ok_a, N, N >> PACKED_BITS))
    print("re-keyed table under A: %.3f of its words decode (chance: %.3f)" % (res["table_words_under_a"], 1.0 / (1 << MSG_BITS)))
    err = np.abs(((res["trace_phase"].astype(np.int64) - res["trace_want"].astype(np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)) / 2.0 ** 32
    print("%d-step partial trace: coefficients 0, %d, %d, ... (%d of %d) carry %d x their message, the others are zero: largest distance from that %.2e"
          % (TRACE_STEPS, 1 << TRACE_STEPS, 2 << TRACE_STEPS, N >> TRACE_STEPS, N, 1 << TRACE_STEPS, err.max()))
    sys.exit(0 if ok_pbs == res["want"].size and ok_b == N and ok_a < N // 2 and err.max() < 2.0 ** -(MSG_BITS + 2) else 1)


if __name__ == "__main__":
    main()
