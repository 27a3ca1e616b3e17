"""CPU: TRGSW blind rotation (include/rtfhe.h, rtfhe_trgsw_rotate_batch) without a GPU -- the rotation restated with the oracle's own building
blocks (tests/leveled_oracle.py: oracle_trgsw_rotate, which tests/test_gpu_trgsw_rotate.py compares the device's words with), what it means with keys and selectors
the product generated, and the entry points' refusal of a null context."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from kit import torus_dist
from leveled_oracle import as_trlwe, oracle_trgsw_rotate, rotate_clear
from pbs_oracle import bk_fft

@pytest.mark.parametrize("N", [1024, 2048])
def test_oracle_rotation_brings_the_addressed_coefficient_to_the_front(orc, N, capsys):
    """Keys from the product's keygen, selectors from encrypt_selectors, the default rot at depth log2 N: for addresses 0, 1, N - 1 and three
    random ones, over a row of N random 2-bit messages -- plain (trivial) and a real TRLWE encryption -- the oracle result's phase decodes to
    X^{-addr} * row at every coefficient (coefficient 0 to msgs[addr]), and stays within depth * 2e-3 * N / 1024 of it: the reference's own
    per-product bound (hom_nand/src/trgsw.rs:365-393) summed over the steps as tests/test_cmux_tree_host.py sums it over the levels.
    Measured on the CPU: worst distance 0.0069 of 0.020 at N = 1024, 0.0149 of 0.044 at N = 2048."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0xD9 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    rng = np.random.default_rng(N + 9)
    depth = N.bit_length() - 1
    msgs = rng.integers(0, 4, N)
    plain = R.encode_msgs(msgs, 2).reshape(N)
    rows = {"plain": as_trlwe(plain, N)[0], "encrypted": R.encrypt_lut(rp, key1, plain[None], seed=0xE7 + N)[0]}
    worst = {}
    for addr in [0, 1, N - 1] + [int(a) for a in rng.integers(2, N - 1, 3)]:
        bits = [(addr >> k) & 1 for k in range(depth)]
        sel = R.encrypt_selectors(rp, key1, bits, seed=0x5E2 + addr)
        sel_f = bk_fft(orc, p, plan, sel.reshape(-1))
        want = rotate_clear(plain, addr)
        for kind, row in rows.items():
            got = oracle_trgsw_rotate(orc, p, plan, sel_f, range(depth), None, row)
            ph = R.trlwe_phase(rp, key1, got[None])[0]
            dec = R.decode_msgs(ph, 2)
            assert np.array_equal(dec, R.decode_msgs(want, 2)), (kind, addr)
            assert dec[0] == msgs[addr], (kind, addr)
            worst[kind] = max(worst.get(kind, 0.0), float(torus_dist(ph, want).max()))
    with capsys.disabled():
        print("\noracle TRGSW rotation, N = %d, depth %d: largest torus distance from X^-addr * row %s" % (N, depth, {k: round(v, 5) for k, v in worst.items()}))
    for kind, w in worst.items():
        assert w < depth * 2e-3 * N / 1024, (kind, w)


def test_entries_reject_a_null_context():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = R._ffi.ERR_INVALID
    row = np.zeros((1, 2, p.N), np.uint32)
    res = np.zeros((1, 2, p.N), np.uint32)
    assert L.rtfhe_trgsw_rotate_batch(None, None, None, 1, None, ptr(row), ptr(res), 1) == INV
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trgsw_rotate_batch_dev(None, None, None, 1, None, None, None, 1, None) == INV
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trgsw_rotate_extract_batch(None, None, None, 1, None, ptr(row), ptr(res), 1) == INV
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trgsw_rotate_extract_batch_dev(None, None, None, 1, None, None, None, 1, None) == INV
    assert b"null context" in L.rtfhe_last_error(None)
