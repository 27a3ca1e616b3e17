#!/usr/bin/env python3
"""examples/leveled_lut.py's 12-bit table lookup with seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts"): the client ships the twelve
TRGSW selectors of every address as a 32-byte public seed and their b polynomials only, the table's owner does the same with the four encrypted
rows, and the server regenerates every mask on the GPU (rtfhe_trgsw_create_seeded, rtfhe_lut_create_encrypted_seeded; k_seeded_expand) --
half the bytes on the wire and over PCIe, the same 13 CMUXes per query, the same answers.

    python examples/seeded_leveled_lut.py [queries]      # random table, random addresses, checked against the plaintext table
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

ROW_BITS = 2        # address bits selected by the CMUX tree: 4 rows
MSG_BITS = 2


def _test_seed(seed, salt):
    """TEST ONLY: the deterministic forms' arguments from one integer (None: the production forms, which draw their own seed from the OS)"""
    if seed is None:
        return {}
    return {"noise_seed": seed + salt, "seed": np.random.default_rng(seed + salt).integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)}


def encrypted_rows(p, key1, table, seed=None):
    """The table as its owner ships it: (seed, b) with b u32[4][N], row h = the b half of a TRLWE of the polynomial whose coefficient c
    encodes table[h N + c]."""
    return R.encrypt_lut_seeded(p, key1, R.encode_msgs(np.asarray(table).reshape(1 << ROW_BITS, p.N), MSG_BITS), **_test_seed(seed, 1))


def client_query(p, key1, addr, seed=None):
    """addresses in [0, 4 N) -> (seed, b) with b u32[len * (log2 N + 2)][2l][N]: per query the log2 N coefficient bits, least significant
    first, then the two row bits.  One call, one fresh seed, rows numbered from 0: no (seed, row) pair masks two ciphertexts."""
    addr = np.asarray(addr, np.int64)
    bits = ((addr[:, None] >> np.arange(p.nbit + ROW_BITS)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors_seeded(p, key1, bits, **_test_seed(seed, 2))


def server_lookup(engine, rows, selectors, count):
    """examples/leveled_lut.py's server on the seeded uploads: the tree into d_row, the rotation of d_row in place, then sample extraction and
    the key switch."""
    import torch
    p = engine.p
    per = p.nbit + ROW_BITS
    st = torch.cuda.current_stream().cuda_stream
    idx = np.arange(count * per, dtype=np.int32).reshape(count, per)
    d_low = torch.from_numpy(np.ascontiguousarray(idx[:, :p.nbit])).cuda()
    d_high = torch.from_numpy(np.ascontiguousarray(idx[:, p.nbit:])).cuda()
    d_row = torch.zeros((count, 2, p.N), dtype=torch.int32, device="cuda")
    with engine.selectors_seeded(*selectors) as sel, engine.lut_encrypted_seeded(*rows) as table:
        engine.cmux_tree_batch_dev(sel, table, ROW_BITS, d_row, count, d_high, None, st)
        engine.trgsw_rotate_batch_dev(sel, d_row, p.nbit, d_row, count, d_low, None, st)      # in place: X^-addr * row
        engine.sync(st)
    acc = d_row.cpu().numpy().view(np.uint32)
    b, a = acc[:, 0], acc[:, 1]
    tlwe1 = np.concatenate([a[:, :1], (0 - a[:, :0:-1].astype(np.int64)).astype(np.uint32), b[:, :1]], axis=1)      # a'_0 = a_0, a'_c = -a_{N-c}; b' = b_0
    return engine.key_switch_batch(tlwe1)


def shipped_bytes(p, count):
    """(full, seeded) bytes of `count` queries and the table: every row is 2 N words in full, N words and a share of a 32-byte seed when seeded"""
    rows = count * (p.nbit + ROW_BITS) * 2 * p.l + (1 << ROW_BITS)
    return rows * 2 * p.N * 4, rows * p.N * 4 + 2 * 32


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
    full, seeded = shipped_bytes(p, count)
    print("%d / %d lookups right (%d CMUXes, no bootstrap)" % (int((got == want).sum()), count, count * ((1 << ROW_BITS) - 1 + p.nbit)))
    print("shipped: %d bytes seeded, %d bytes in full (%.3f x)" % (seeded, full, seeded / full))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
