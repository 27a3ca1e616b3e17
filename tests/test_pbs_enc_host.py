"""CPU: encrypted tables for programmable bootstrapping (include/rtfhe.h, rtfhe_lut_create_encrypted) without a GPU -- the host TRLWE
encryption of test polynomials (rtfhe_trlwe_encrypt_torus[_deterministic], rtfhe_trlwe_phase), the PBS from an encrypted table restated
with the oracle's own building blocks (tests/pbs_oracle.py: oracle_pbs_enc, which tests/test_gpu_pbs_enc.py compares the device's words with) and the entry
points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from kit import torus_dist_lsb
from pbs_oracle import bk_fft, oracle_pbs_enc, oracle_pbs_many


@pytest.mark.parametrize("N", [1024, 2048])
def test_encrypt_then_phase(N):
    """|phase - mu| < 2^-20 of the torus on 64 random polynomials (alpha = 2^-25: about 2^-20 is 30 standard deviations), with the OS CSPRNG
    and with a seed."""
    import rustfhe_amd as R
    p = R.Params(n=16, N=N)
    key1 = np.random.default_rng(N).integers(0, 2, N).astype(np.int32)
    mu = np.random.default_rng(N + 1).integers(0, 1 << 32, (64, N), dtype=np.uint64).astype(np.uint32)
    for seed in (None, 0xE17C):
        ct = R.encrypt_lut(p, key1, mu, seed=seed)
        assert ct.shape == (64, 2, N) and ct.dtype == np.uint32
        ph = R.trlwe_phase(p, key1, ct)
        assert ph.shape == (64, N)
        assert torus_dist_lsb(ph, mu).max() < 1 << 12, seed          # 2^-20 of the torus = 2^12 of 2^32
        assert np.any(ph != mu)                                  # there is noise
        assert not np.array_equal(ct[:, 1], np.zeros_like(ct[:, 1]))   # and a random mask
    # the mask is uniform: its words are not small
    assert np.mean(torus_dist_lsb(ct[:, 1], 0) > 1 << 28) > 0.8


def test_trivial_encryption_has_the_table_as_phase():
    import rustfhe_amd as R
    p = R.Params(n=16)
    key1 = np.random.default_rng(3).integers(0, 2, p.N).astype(np.int32)
    tv = R.lut_polynomial(lambda m: (m + 1) % 4, p.N, 2)
    triv = np.stack([tv, np.zeros_like(tv)])[None]
    assert np.array_equal(R.trlwe_phase(p, key1, triv)[0], tv)


def test_deterministic_twin_reproducible_and_seed_sensitive_production_fresh():
    import rustfhe_amd as R
    p = R.Params(n=16)
    key1 = np.random.default_rng(5).integers(0, 2, p.N).astype(np.int32)
    mu = np.random.default_rng(6).integers(0, 1 << 32, (3, p.N), dtype=np.uint64).astype(np.uint32)
    a = R.encrypt_lut(p, key1, mu, seed=11)
    assert np.array_equal(a, R.encrypt_lut(p, key1, mu, seed=11))
    assert not np.array_equal(a, R.encrypt_lut(p, key1, mu, seed=12))
    assert not np.array_equal(R.encrypt_lut(p, key1, mu), R.encrypt_lut(p, key1, mu))
    # one polynomial, as u32[N], gives one row
    assert R.encrypt_lut(p, key1, mu[0], seed=11).shape == (1, 2, p.N)
    assert np.array_equal(R.encrypt_lut(p, key1, mu[0], seed=11)[0], a[0])


def test_oracle_enc_of_a_trivial_encryption_is_oracle_pbs_many(orc):
    """(tv, 0) through oracle_pbs_enc is oracle_pbs_many of tv word for word (small n, N = 1024), for every n_out."""
    p = orc.Params(n=24)
    plan = orc.Plan(p.N)
    keys = orc.Keys(p, 0x3A12, plan=plan)
    rng = np.random.default_rng(22)
    for n_out in (1, 2, 4, 8):
        tv = rng.integers(0, 1 << 32, p.N, dtype=np.uint64).astype(np.uint32)
        t = rng.integers(0, 1 << 32, p.n + 1, dtype=np.uint64).astype(np.uint32)
        triv = np.stack([tv, np.zeros_like(tv)])
        enc = oracle_pbs_enc(orc, p, plan, keys.bk_f, keys.ksk, triv, t, n_out)
        assert enc.shape == (n_out, p.n + 1)
        assert np.array_equal(enc, oracle_pbs_many(orc, p, plan, keys.bk_f, keys.ksk, tv, t, n_out)), n_out


def test_oracle_enc_of_a_real_encryption_decrypts_to_every_function(orc):
    """Keys from the product's keygen: 2-bit messages through encrypted tables of two and four interleaved functions, every output decrypts."""
    import rustfhe_amd as R
    rp = R.Params(n=64)
    key0, key1, bk, ksk = R.keygen(rp, 0xB02)
    p = orc.Params(n=64)
    plan = orc.Plan(p.N)
    bk_f = bk_fft(orc, p, plan, bk)
    msgs = np.array([0, 1, 2, 3, 3, 0, 2, 1])
    cts = R.encrypt_torus(rp, key0, R.encode_msgs(msgs, 2), seed=0xC9)
    for fs in ([lambda s: s & 1, lambda s: s >> 1], [lambda s: s, lambda s: (s * s) % 4, lambda s: (s + 1) % 4, lambda s: 3 - s]):
        row = R.encrypt_lut(rp, key1, R.many_lut_polynomial(fs, p.N, 2), seed=0xD0 + len(fs))[0]
        outs = np.stack([oracle_pbs_enc(orc, p, plan, bk_f, ksk, row, t, len(fs)) for t in cts])
        for j, f in enumerate(fs):
            assert list(R.decode_msgs(R.phases(rp, key0, outs[:, j]), 2)) == [f(m) for m in msgs], j


def test_entries_reject_null_pointers_and_bad_params():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=16)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    key1 = np.zeros(p.N, np.int32)
    mu = np.zeros((1, p.N), np.uint32)
    ct = np.zeros((1, 2, p.N), np.uint32)
    ph = np.zeros((1, p.N), np.uint32)
    INV = R._ffi.ERR_INVALID
    assert L.rtfhe_trlwe_encrypt_torus(C.byref(p), ptr(key1), ptr(mu), ptr(ct), 1) == 0
    assert L.rtfhe_trlwe_encrypt_torus(None, ptr(key1), ptr(mu), ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_encrypt_torus(C.byref(p), None, ptr(mu), ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_encrypt_torus(C.byref(p), ptr(key1), None, ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_encrypt_torus(C.byref(p), ptr(key1), ptr(mu), None, 1) == INV
    assert L.rtfhe_trlwe_encrypt_torus_deterministic(C.byref(p), None, 1, ptr(mu), ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_encrypt_torus_deterministic(C.byref(p), ptr(key1), 1, ptr(mu), None, 1) == INV
    assert L.rtfhe_trlwe_phase(C.byref(p), ptr(key1), None, ptr(ph), 1) == INV
    assert L.rtfhe_trlwe_phase(C.byref(p), ptr(key1), ptr(ct), None, 1) == INV
    bad = R.Params(n=16)
    bad.N = 1000                                                   # not a power of two
    assert L.rtfhe_trlwe_encrypt_torus(C.byref(bad), ptr(key1), ptr(mu), ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_phase(C.byref(bad), ptr(key1), ptr(ct), ptr(ph), 1) == INV
    key1[3] = 2                                                    # not a binary key
    assert L.rtfhe_trlwe_encrypt_torus_deterministic(C.byref(p), ptr(key1), 1, ptr(mu), ptr(ct), 1) == INV
    assert L.rtfhe_trlwe_phase(C.byref(p), ptr(key1), ptr(ct), ptr(ph), 1) == INV
    # the table entry point: null context / table rows / handle
    h = C.c_void_p()
    assert L.rtfhe_lut_create_encrypted(None, ptr(ct), 1, C.byref(h)) == INV
