#!/usr/bin/env python3
"""A 6-bit table lookup by vertical packing (include/rtfhe.h: rtfhe_cmux_tree_batch, rtfhe_lut_create_encrypted).  The server holds a secret
64-entry table of 2-bit values as 16 encrypted rows: row h is the TRLWE of the test polynomial of m -> T[4 h + m].  The client sends the
address a = 4 h + m in two parts: the four bits of h as TRGSW ciphertexts (rustfhe_amd.encrypt_selectors), the 2-bit digit m as a TLWE.
The server selects row h of every query with 15 CMUXes (a depth-4 tree) without learning h, then runs one PBS on the digit with the selected
row as its encrypted table.  The selected rows pass through the host on their way into Engine.lut_encrypted.

    python examples/wide_lut.py [queries]      # random table, random addresses, checked against the plaintext table
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

HIGH_BITS = 4       # address bits selected by the CMUX tree: 16 rows
MSG_BITS = 2        # address bits selected by the PBS: 4 values per row


def encrypted_rows(p, key1, table, seed=None):
    """The table as the server holds it: u32[16][2][N], row h = TRLWE of the test polynomial of m -> table[4 h + m]."""
    tv = np.stack([R.lut_polynomial([int(v) for v in row], p.N, MSG_BITS) for row in np.asarray(table).reshape(1 << HIGH_BITS, 1 << MSG_BITS)])
    return R.encrypt_lut(p, key1, tv, seed=seed)


def client_query(p, key0, key1, addr, seed=None):
    """addresses in [0, 64) -> (TRGSW selectors u32[len * 4][2][2l][N], bit k of query g at g * 4 + k; TLWE digits u32[len][n+1])"""
    addr = np.asarray(addr, np.int64)
    high, low = addr >> MSG_BITS, addr & ((1 << MSG_BITS) - 1)
    bits = ((high[:, None] >> np.arange(HIGH_BITS)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors(p, key1, bits, seed=seed), R.encrypt_torus(p, key0, R.encode_msgs(low, MSG_BITS), seed=seed)


def server_lookup(engine, rows, selectors, digits):
    """What the server runs: one depth-4 tree per query (query g uses selectors g * 4 + k), then one PBS per query on its own selected row."""
    count = digits.shape[0]
    with engine.selectors(selectors) as sel, engine.lut_encrypted(rows) as table:
        picked = engine.cmux_tree_batch(sel, table, HIGH_BITS, count)
    with engine.lut_encrypted(picked) as lut:
        return engine.pbs_batch(lut, digits, np.arange(count, dtype=np.int32))


def run(engine, key0, key1, count, seed=None):
    """`count` random addresses into a random table.  Returns (addresses, decrypted results, expected)."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, 1 << MSG_BITS, 1 << (HIGH_BITS + MSG_BITS))
    addr = rng.integers(0, table.size, count)
    rows = encrypted_rows(engine.p, key1, table, seed=seed)
    selectors, digits = client_query(engine.p, key0, key1, addr, seed=seed)
    out = server_lookup(engine, rows, selectors, digits)
    return addr, R.decode_msgs(R.phases(engine.p, key0, out), MSG_BITS), table[addr]


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    addr, got, want = run(eng, key0, key1, count)
    print("%d / %d lookups right (%d CMUXes and %d bootstraps)" % (int((got == want).sum()), count, count * 15, count))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
