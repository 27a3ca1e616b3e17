#!/usr/bin/env python3
"""A private function through encrypted tables (include/rtfhe.h: rtfhe_lut_create_encrypted).  The client picks a secret 2-bit -> 2-bit
function for each of the four 2-bit digits of a byte, encrypts the four tables under its lvl1 key (rustfhe_amd.encrypt_lut) and hands the
server only those ciphertexts.  The server applies digit d's table to digit d of every encrypted byte -- one PBS per digit, table index d in
the clear -- without learning the functions.  The client decrypts and checks against the plaintext functions.

    python examples/private_lut.py [bytes]      # random bytes, random secret functions, checked digit by digit
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rustfhe_amd as R  # noqa: E402

DIGITS = 4          # 2-bit digits per byte
MSG_BITS = 2


def secret_functions(rng):
    """[DIGITS][4]: the value table of each digit's function (any map of {0..3} to itself)."""
    return rng.integers(0, 1 << MSG_BITS, (DIGITS, 1 << MSG_BITS))


def client_tables(p, key1, funcs, seed=None):
    """The encrypted table the server gets: u32[DIGITS][2][N], row d = TRLWE of digit d's test polynomial under key1."""
    tv = np.stack([R.lut_polynomial([int(v) for v in f], p.N, MSG_BITS) for f in funcs])
    return R.encrypt_lut(p, key1, tv, seed=seed)


def encrypt_bytes(p, key0, x, seed=None):
    """bytes x -> u32[len(x) * DIGITS][n+1]: the digits of each byte, least significant first, each a 2-bit message."""
    digits = (np.asarray(x, np.int64)[:, None] >> (MSG_BITS * np.arange(DIGITS))) & ((1 << MSG_BITS) - 1)
    return R.encrypt_torus(p, key0, R.encode_msgs(digits.reshape(-1), MSG_BITS), seed=seed)


def server_apply(engine, table, cts):
    """What the server runs: digit d of every byte through row d of the encrypted table (one PBS per digit)."""
    idx = np.tile(np.arange(DIGITS, dtype=np.int32), cts.shape[0] // DIGITS)
    with engine.lut_encrypted(table) as lut:
        return engine.pbs_batch(lut, cts, idx)


def decode_bytes(p, key0, out):
    digits = R.decode_msgs(R.phases(p, key0, out), MSG_BITS).reshape(-1, DIGITS)
    return (digits << (MSG_BITS * np.arange(DIGITS))).sum(axis=1)


def plain(funcs, x):
    """The plaintext reference: digit d of each byte replaced by funcs[d][digit]."""
    x = np.asarray(x, np.int64)
    return sum(funcs[d][(x >> (MSG_BITS * d)) & 3] << (MSG_BITS * d) for d in range(DIGITS))


def run(engine, key0, key1, count, seed=None):
    """Applies random secret functions to `count` random encrypted bytes.  Returns (x, result, expected)."""
    rng = np.random.default_rng(seed)
    funcs = secret_functions(rng)
    x = rng.integers(0, 256, count)
    table = client_tables(engine.p, key1, funcs, seed=seed)
    out = server_apply(engine, table, encrypt_bytes(engine.p, key0, x, seed=seed))
    return x, decode_bytes(engine.p, key0, out), plain(funcs, x)


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = R.Params()
    key0, key1, bk, ksk = R.keygen(p)
    eng = R.Engine(p, 0)
    eng.load_bk_torus(bk)
    eng.load_ksk(ksk)
    x, got, want = run(eng, key0, key1, count)
    print("%d / %d bytes right (%d bootstraps from an encrypted table)" % (int((got == want).sum()), count, count * DIGITS))
    eng.close()
    sys.exit(0 if np.array_equal(got, want) else 1)


if __name__ == "__main__":
    main()
