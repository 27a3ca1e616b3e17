"""CPU: CMUX-tree table lookup (include/rtfhe.h, rtfhe_cmux_tree_batch) without a GPU -- the tree restated with the oracle's own building
blocks (tests/leveled_oracle.py: oracle_cmux_tree, which tests/test_gpu_cmux_tree.py compares the device's words with), what it means with keys and selectors the
product generated, the host TRGSW encryption of selector bits, and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from kit import torus_dist
from leveled_oracle import as_trlwe, oracle_cmux_tree
from pbs_oracle import bk_fft

@pytest.mark.parametrize("N", [1024, 2048])
def test_oracle_tree_selects_the_addressed_row(orc, N, capsys):
    """Keys from the product's keygen, selectors from encrypt_selectors: for every address of a depth-3 and of a depth-4 tree over random rows
    of N 2-bit messages -- plain rows and TRLWE encryptions of them -- the oracle tree's phase decodes to the addressed row at every coefficient,
    and stays within depth * 2e-3 * N / 1024 of it: the reference's own per-product bound (hom_nand/src/trgsw.rs:365-393) as
    tests/test_gpu_trgsw_semantics.py scales it with N, summed over the levels."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    key0, key1, _, _ = R.keygen(rp, 0xC7 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    rng = np.random.default_rng(N + 3)
    worst = {}
    for depth in (3, 4):
        msgs = rng.integers(0, 4, (1 << depth, N))
        plain = R.encode_msgs(msgs, 2)
        for kind, rows in (("plain", as_trlwe(plain, N)), ("encrypted", R.encrypt_lut(rp, key1, plain, seed=0xE0 + depth))):
            for addr in range(1 << depth):
                bits = [(addr >> k) & 1 for k in range(depth)]
                sel = R.encrypt_selectors(rp, key1, bits, seed=0x5E1 + 16 * depth + addr)
                got = oracle_cmux_tree(orc, p, plan, bk_fft(orc, p, plan, sel.reshape(-1)), range(depth), rows)
                ph = R.trlwe_phase(rp, key1, got[None])[0]
                assert np.array_equal(R.decode_msgs(ph, 2), msgs[addr]), (depth, kind, addr)
                worst[depth, kind] = max(worst.get((depth, kind), 0.0), float(torus_dist(ph, plain[addr]).max()))
    with capsys.disabled():
        print("\noracle CMUX tree, N = %d: largest torus distance from the addressed row %s" % (N, {k: round(v, 5) for k, v in worst.items()}))
    for (depth, kind), w in worst.items():
        assert w < depth * 2e-3 * N / 1024, (depth, kind, w)


def test_encrypt_selectors_deterministic_per_seed_fresh_without():
    import rustfhe_amd as R
    p = R.Params(n=8)
    key1 = np.random.default_rng(5).integers(0, 2, p.N).astype(np.int32)
    bits = [1, 0, 1]
    a = R.encrypt_selectors(p, key1, bits, seed=11)
    assert a.shape == (3, 2, 2 * p.l, p.N) and a.dtype == np.uint32
    assert np.array_equal(a, R.encrypt_selectors(p, key1, bits, seed=11))
    assert not np.array_equal(a, R.encrypt_selectors(p, key1, bits, seed=12))
    assert not np.array_equal(R.encrypt_selectors(p, key1, bits), R.encrypt_selectors(p, key1, bits))
    assert not np.array_equal(a[0], a[2])                       # one generator runs through the whole call: no mask is reused


@pytest.mark.parametrize("N", [1024, 2048])
def test_encrypted_selectors_behave_as_bk_entries_do(orc, N):
    """The reference's trgsw_cmux property (hom_nand/src/trgsw.rs:395-426) on TRGSW(bit) from encrypt_selectors, OS CSPRNG and seeded:
    TRGSW(i).cmux(rep_1, rep_0) decrypts to pol_i for the all-One / all-Zero polynomials (One = +1/8, Zero = -1/8), within 2e-3 * N / 1024.
    And each sample is a valid TRGSW: its rows' phases are bit * (the gadget) as test_abi's check of the product's bootstrapping key reads them."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0xB1 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    pols = np.stack([np.full(N, 0xE0000000, np.uint32), np.full(N, 0x20000000, np.uint32)])      # pol_0 = all Zero, pol_1 = all One
    reps = R.encrypt_lut(rp, key1, pols, seed=0x77)
    for seed in (None, 0x5EED):
        sel = R.encrypt_selectors(rp, key1, [0, 1], seed=seed)
        sel_f = bk_fft(orc, p, plan, sel.reshape(-1))
        for bit in (0, 1):
            got = oracle_cmux_tree(orc, p, plan, sel_f, [bit], reps)
            ph = R.trlwe_phase(rp, key1, got[None])[0]
            assert torus_dist(ph, pols[bit]).max() < 2e-3 * N / 1024, (seed, bit)
            rows = sel[bit].reshape(2, 2 * p.l, N)
            for j in range(2 * p.l):
                ph = R.trlwe_phase(rp, key1, np.stack([rows[0, j], rows[1, j]])[None])[0].astype(np.int64)
                g = bit << (32 - p.bgbit * ((j % p.l) + 1))
                want = np.zeros(N, np.int64)
                if j < p.l:
                    want[0] = g                                       # cipher[j] += mu / Bg^(j+1)
                else:
                    want = (-g * key1.astype(np.int64)) % 2 ** 32     # p_key[j] += g  <=>  the phase gains -g * s(X)
                err = ((ph - want + 2 ** 31) % 2 ** 32) - 2 ** 31
                assert np.abs(err).max() < 2 ** 12, (seed, bit, j)


def test_entries_reject_null_handles_and_bad_arguments():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = R._ffi.ERR_INVALID
    key1 = np.zeros(p.N, np.int32)
    bits = np.array([1, 0], np.uint8)
    out = np.zeros((2, 2, 2 * p.l, p.N), np.uint32)
    assert L.rtfhe_trgsw_encrypt_bits(C.byref(p), ptr(key1), ptr(bits), ptr(out), 2) == 0
    assert L.rtfhe_trgsw_encrypt_bits(None, ptr(key1), ptr(bits), ptr(out), 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits(C.byref(p), None, ptr(bits), ptr(out), 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits(C.byref(p), ptr(key1), None, ptr(out), 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits(C.byref(p), ptr(key1), ptr(bits), None, 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits_deterministic(C.byref(p), None, 1, ptr(bits), ptr(out), 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits_deterministic(C.byref(p), ptr(key1), 1, ptr(bits), None, 2) == INV
    bad = R.Params(n=8)
    bad.N = 1000                                                   # not a power of two
    assert L.rtfhe_trgsw_encrypt_bits(C.byref(bad), ptr(key1), ptr(bits), ptr(out), 2) == INV
    key1[3] = 2                                                    # not a binary key
    assert L.rtfhe_trgsw_encrypt_bits_deterministic(C.byref(p), ptr(key1), 1, ptr(bits), ptr(out), 2) == INV
    # the device entry points: a null context (there is none without a GPU) is refused before anything else is looked at
    h = C.c_void_p()
    res = np.zeros((1, 2, p.N), np.uint32)
    assert L.rtfhe_trgsw_create(None, ptr(out), 2, C.byref(h)) == INV and not h.value
    L.rtfhe_trgsw_destroy(None)
    assert L.rtfhe_cmux_tree_batch(None, None, None, 1, None, None, ptr(res), 1) == INV
    assert L.rtfhe_cmux_tree_batch_dev(None, None, None, 1, None, None, None, 1, None) == INV
    assert L.rtfhe_cmux_tree_extract_batch(None, None, None, 1, None, None, None, ptr(res), 1) == INV
    assert L.rtfhe_cmux_tree_extract_batch_dev(None, None, None, 1, None, None, None, None, 1, None) == INV
    assert b"null context" in L.rtfhe_last_error(None)
