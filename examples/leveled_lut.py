#!/usr/bin/env python3
"""A 12-bit table lookup in TFHE's leveled mode, no bootstrapping key anywhere (include/rtfhe.h: rtfhe_cmux_tree_batch,
rtfhe_trgsw_rotate_extract_batch).  The server holds a secret table of 4,096 2-bit values as four encrypted rows of N = 1,024 coefficients:
entry a lives at coefficient a mod N of row a div N.  The client sends the twelve bits of the address a as TRGSW ciphertexts
(rustfhe_amd.encrypt_selectors).  The server selects the row of every query with a depth-2 CMUX tree (3 CMUXes, vertical packing) into a
device buffer, rotates it there in place by the ten low bits (10 CMUXes, horizontal packing: X^-addr brings the entry to coefficient 0), then
extracts coefficient 0 and key-switches it: 13 CMUXes per query, and the server learns nothing about the address.

    python examples/leveled_lut.py [queries]      # random table, random addresses, checked against the plaintext table
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

ROW_BITS = 2        # address bits selected by the CMUX tree: 4 rows
MSG_BITS = 2


def encrypted_rows(p, key1, table, seed=None):
    """The table as the server holds it: u32[4][2][N], row h = TRLWE of the polynomial whose coefficient c encodes table[h N + c]."""
    return R.encrypt_lut(p, key1, R.encode_msgs(np.asarray(table).reshape(1 << ROW_BITS, p.N), MSG_BITS), seed=seed)


def client_query(p, key1, addr, seed=None):
    """addresses in [0, 4 N) -> TRGSW selectors u32[len * (log2 N + 2)][2][2l][N]: per query the log2 N coefficient bits, least significant
    first, then the two row bits"""
    addr = np.asarray(addr, np.int64)
    bits = ((addr[:, None] >> np.arange(p.nbit + ROW_BITS)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors(p, key1, bits, seed=seed)


def server_lookup(engine, rows, selectors, count):
    """What the server runs, on device buffers and one stream: the tree into d_row, then the rotation of d_row in place (query g uses
    selectors g * 12 + k: k < 10 for the rotation, 10 and 11 for the tree).  Coefficient 0 of the rotated rows is then extracted
    (trlwe.rs:110-121) and key-switched; Engine.trgsw_rotate_extract_batch_dev fuses the rotation with these last two steps."""
    import torch
    p = engine.p
    per = p.nbit + ROW_BITS
    st = torch.cuda.current_stream().cuda_stream
    idx = np.arange(count * per, dtype=np.int32).reshape(count, per)
    d_low = torch.from_numpy(np.ascontiguousarray(idx[:, :p.nbit])).cuda()
    d_high = torch.from_numpy(np.ascontiguousarray(idx[:, p.nbit:])).cuda()
    d_row = torch.zeros((count, 2, p.N), dtype=torch.int32, device="cuda")
    with engine.selectors(selectors) as sel, engine.lut_encrypted(rows) as table:
        engine.cmux_tree_batch_dev(sel, table, ROW_BITS, d_row, count, d_high, None, st)
        engine.trgsw_rotate_batch_dev(sel, d_row, p.nbit, d_row, count, d_low, None, st)      # in place: X^-addr * row
        engine.sync(st)
    acc = d_row.cpu().numpy().view(np.uint32)
    b, a = acc[:, 0], acc[:, 1]
    tlwe1 = np.concatenate([a[:, :1], (0 - a[:, :0:-1].astype(np.int64)).astype(np.uint32), b[:, :1]], axis=1)      # a'_0 = a_0, a'_c = -a_{N-c}; b' = b_0
    return engine.key_switch_batch(tlwe1)


def run(engine, key0, key1, count, seed=None):
    """`count` random addresses into a random table.  Returns (addresses, decrypted results, expected)."""
    rng = np.random.default_rng(seed)
    p = engine.p
    table = rng.integers(0, 1 << MSG_BITS, p.N << ROW_BITS)
    addr = rng.integers(0, table.size, count)
    rows = encrypted_rows(p, key1, table, seed=seed)
    out = server_lookup(engine, rows, client_query(p, key1, addr, seed=seed), count)
    return addr, R.decode_msgs(R.phases(p, key0, out), MSG_BITS), table[addr]


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    p = R.Params()
    key0, key1, _, ksk = R.keygen(p, want_bk=False)
    eng = R.Engine(p, 0)
    eng.load_ksk(ksk)                                   # no bootstrapping key is ever loaded
    addr, got, want = run(eng, key0, key1, count)
    print("%d / %d lookups right (%d CMUXes, no bootstrap)" % (int((got == want).sum()), count, count * ((1 << ROW_BITS) - 1 + p.nbit)))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
