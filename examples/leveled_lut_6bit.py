#!/usr/bin/env python3
"""An 18-bit lookup into a table of 6-bit entries in TFHE's leveled mode with the rounded gadget decomposition (include/rtfhe.h:
rtfhe_set_leveled_decomposition).  The server holds 2^8 * N = 262,144 six-bit values as 256 encrypted rows of N = 1,024
coefficients: entry a lives at coefficient a mod N of row a div N.  The client sends the eighteen bits of the address as TRGSW ciphertexts.
The server selects the row with a depth-8 CMUX tree (255 CMUXes) and rotates it in place by the ten low bits (10 CMUXes), both in the
rounded leveled mode; coefficient 0 of the result is the entry.  It is read here as the lvl1 sample it is, under the lvl1 key: a 6-bit
message has 1/128 of margin, which the leveled path keeps (about 5e-4 of noise) and a key switch to lvl0 would spend.

With the reference's decomposition every level whose address bit is 1 adds about 1e-3 of systematic error: the all-ones address comes out
wrong about half of the time.  Both modes run on the same ciphertexts.

    python examples/leveled_lut_6bit.py [queries]      # random table; the all-ones address, address 0 and random ones
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

ROW_BITS = 8        # address bits selected by the CMUX tree: 256 rows
MSG_BITS = 6


def encrypted_rows(p, key1, table, row_bits=ROW_BITS, seed=None):
    """The table as the server holds it: u32[2^row_bits][2][N], row h = TRLWE of the polynomial whose coefficient c encodes table[h N + c]."""
    return R.encrypt_lut(p, key1, R.encode_msgs(np.asarray(table).reshape(1 << row_bits, p.N), MSG_BITS), seed=seed)


def client_query(p, key1, addr, row_bits=ROW_BITS, seed=None):
    """addresses in [0, 2^row_bits N) -> TRGSW selectors u32[len * (log2 N + row_bits)][2][2l][N]: per query the log2 N coefficient bits,
    least significant first, then the row bits"""
    addr = np.asarray(addr, np.int64)
    bits = ((addr[:, None] >> np.arange(p.nbit + row_bits)) & 1).astype(np.uint8).reshape(-1)
    return R.encrypt_selectors(p, key1, bits, seed=seed)


def server_lookup(engine, rows, selectors, count, row_bits=ROW_BITS, rounded=True):
    """What the server runs, on device buffers and one stream, in the given leveled decomposition mode (restored afterwards): the tree into
    d_row, then the rotation of d_row in place.  Returns the rotated rows u32[count][2][N]; coefficient 0 holds the entry."""
    import torch
    p = engine.p
    per = p.nbit + row_bits
    st = torch.cuda.current_stream().cuda_stream
    idx = np.arange(count * per, dtype=np.int32).reshape(count, per)
    d_low = torch.from_numpy(np.ascontiguousarray(idx[:, :p.nbit])).cuda()
    d_high = torch.from_numpy(np.ascontiguousarray(idx[:, p.nbit:])).cuda()
    d_row = torch.zeros((count, 2, p.N), dtype=torch.int32, device="cuda")
    before = engine.leveled_decomposition()
    engine.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED if rounded else R._ffi.DECOMP_REFERENCE)
    try:
        with engine.selectors(selectors) as sel, engine.lut_encrypted(rows) as table:
            engine.cmux_tree_batch_dev(sel, table, row_bits, d_row, count, d_high, None, st)
            engine.trgsw_rotate_batch_dev(sel, d_row, p.nbit, d_row, count, d_low, None, st)      # in place: X^-addr * row
            engine.sync(st)
    finally:
        engine.set_leveled_decomposition(before)
    return d_row.cpu().numpy().view(np.uint32)


def run(engine, key1, count, row_bits=ROW_BITS, seed=None):
    """`count` addresses into a random table: the all-ones address, address 0, then random ones.  Returns (addresses, expected entries,
    decrypted results in rounded mode, ... in reference mode on the same ciphertexts)."""
    rng = np.random.default_rng(seed)
    p = engine.p
    table = rng.integers(0, 1 << MSG_BITS, p.N << row_bits)
    addr = np.concatenate([[table.size - 1, 0], rng.integers(0, table.size, max(count - 2, 0))])[:count]
    rows = encrypted_rows(p, key1, table, row_bits, seed=seed)
    selectors = client_query(p, key1, addr, row_bits, seed=seed)
    got = {}
    for rounded in (True, False):
        acc = server_lookup(engine, rows, selectors, count, row_bits, rounded)
        got[rounded] = R.decode_msgs(R.trlwe_phase(p, key1, acc)[:, 0], MSG_BITS)
    return addr, table[addr], got[True], got[False]


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    p = R.Params()
    _, key1, _, _ = R.keygen(p, want_bk=False, want_ksk=False)
    eng = R.Engine(p, 0)                                # no key is ever loaded: the leveled path needs none
    addr, want, got, ref = run(eng, key1, count)
    cmuxes = count * ((1 << ROW_BITS) - 1 + p.nbit)
    print("rounded leveled decomposition:   %d / %d lookups right (%d CMUXes, no bootstrap)" % (int((got == want).sum()), count, cmuxes))
    print("reference leveled decomposition: %d / %d lookups right on the same ciphertexts" % (int((ref == want).sum()), count))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
