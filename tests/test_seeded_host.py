"""CPU: seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts") without a GPU -- the mask rule against RFC 8439 and known answers, the host
expansion against its numpy restatement (tests/seeded_oracle.py, which tests/test_gpu_seeded.py compares the device's words with), what the
seeded encryptors' output means once expanded, and the argument checks of every seeded entry point."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
import seeded_oracle as so
from kit import random_words, torus_dist, torus_dist_lsb
from leveled_oracle import oracle_cmux_tree
from pbs_oracle import bk_fft

M64 = 1 << 64


def hexwords(s):
    return np.array([int(w, 16) for w in s.split()], np.uint32)


def test_oracle_block_function_reproduces_rfc8439_2_3_2():
    got = so.block(so.KAT_KEY, 1, 0x09000000, 0x4a000000, 0)
    want = hexwords("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")
    assert np.array_equal(got, want)


KNOWN = [(1024, 0, 0, "7d2bfd39 6a19c5d9 7703bd8d 494adcb8"), (1024, 0, 15, "0c415b48"),
         (1024, 5, 1008, "33d19c69 e3c08b23 287ab359 1410541d"), (1024, 5, 1023, "d526d505"),
         (2048, M64 - 1, 2032, "21be8713 a122d73c 38f1888c 73a08aa9"), (2048, M64 - 1, 2047, "99fc8aa5")]


@pytest.mark.parametrize("N,row,at,words", KNOWN)
def test_mask_expand_known_answers(N, row, at, words):
    import rustfhe_amd as R
    want = hexwords(words)
    a = R.mask_expand(N, so.KAT_KEY, 1, first_row=row)[0]
    assert np.array_equal(a[at:at + want.size], want)
    assert np.array_equal(so.mask_rows(N, so.KAT_KEY, row, 1)[0][at:at + want.size], want), "the oracle gives the same known answer"


@pytest.mark.skipif(not shutil.which("openssl"), reason="openssl not on the path")
def test_mask_row_is_the_openssl_chacha20_keystream():
    """A whole row against openssl enc -chacha20: key = the seed's bytes, IV = 32-bit counter 0 LE | 0 | row LE."""
    import rustfhe_amd as R
    N, row = 1024, 0x0123456789ABCDEF
    iv = (0).to_bytes(4, "little") + (0).to_bytes(4, "little") + row.to_bytes(8, "little")
    r = subprocess.run(["openssl", "enc", "-chacha20", "-K", so.KAT_KEY.tobytes().hex(), "-iv", iv.hex()], input=bytes(4 * N), capture_output=True, timeout=60)
    if r.returncode != 0 or len(r.stdout) != 4 * N:
        pytest.skip("this openssl has no chacha20 cipher")
    assert np.array_equal(R.mask_expand(N, so.KAT_KEY, 1, first_row=row)[0], np.frombuffer(r.stdout, "<u4"))


@pytest.mark.parametrize("N", [16, 1024, 2048])
@pytest.mark.parametrize("group", [1, 6])
def test_host_expansion_equals_the_oracle_word_for_word(N, group):
    import rustfhe_amd as R
    rng = np.random.default_rng(N + group)
    seed = random_words(rng, 8)
    rows = 12
    p = R.Params(n=8, N=N)
    b = random_words(rng, (rows, N))
    for first_row in (0, (1 << 32) - 2, M64 - rows):
        assert np.array_equal(R.mask_expand(N, seed, rows, first_row=first_row), so.mask_rows(N, seed, first_row, rows)), first_row
        got = R.seeded_expand(p, seed, b, group, first_row=first_row)
        assert got.shape == (rows // group, 2, group, N)
        assert np.array_equal(got, so.expand(N, seed, first_row, b, group)), first_row


@pytest.mark.parametrize("N", [1024, 2048])
def test_expanded_seeded_trlwes_decrypt_to_mu(N):
    """|phase - mu| < 2^-20 of the torus, the bound tests/test_pbs_enc_host.py holds the unseeded encryptor to (alpha = 2^-25: 30 standard
    deviations), production and deterministic."""
    import rustfhe_amd as R
    p = R.Params(n=16, N=N)
    rng = np.random.default_rng(N)
    key1 = rng.integers(0, 2, N).astype(np.int32)
    mu = random_words(rng, (16, N))
    for kw in ({}, {"noise_seed": 0xE17C, "seed": random_words(rng, 8), "first_row": (1 << 32) - 3}):
        seed, b = R.encrypt_lut_seeded(p, key1, mu, **kw)
        assert b.shape == (16, N) and seed.shape == (8,)
        ct = R.seeded_expand(p, seed, b, 1, first_row=kw.get("first_row", 0)).reshape(16, 2, N)
        ph = R.trlwe_phase(p, key1, ct)
        assert torus_dist_lsb(ph, mu).max() < 1 << 12
        assert np.any(ph != mu)
        assert np.array_equal(ct[:, 1], so.mask_rows(N, seed, kw.get("first_row", 0), 16)), "the a halves are the seed's keystream, all 32 bits"


@pytest.mark.parametrize("N", [1024, 2048])
def test_expanded_seeded_trgsw_selects(orc, N):
    """tests/test_cmux_tree_host.py's check of encrypt_selectors on the expanded seeded samples: TRGSW(bit).cmux(rep_1, rep_0) decrypts to pol_bit
    within 2e-3 * N / 1024, and every row's phase is bit * (the gadget); the polynomial form with a constant polynomial gives the bit form's words."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0xB1 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    pols = np.stack([np.full(N, 0xE0000000, np.uint32), np.full(N, 0x20000000, np.uint32)])
    reps = R.encrypt_lut(rp, key1, pols, seed=0x77)
    mseed = random_words(np.random.default_rng(N), 8)
    for kw in ({}, {"noise_seed": 0x5EED, "seed": mseed, "first_row": M64 - 12}):
        seed, b = R.encrypt_selectors_seeded(rp, key1, [0, 1], **kw)
        assert b.shape == (2, 2 * p.l, N)
        sel = R.seeded_expand(rp, seed, b, 2 * p.l, first_row=kw.get("first_row", 0))
        sel_f = bk_fft(orc, p, plan, sel.reshape(-1))
        for bit in (0, 1):
            got = oracle_cmux_tree(orc, p, plan, sel_f, [bit], reps)
            ph = R.trlwe_phase(rp, key1, got[None])[0]
            assert torus_dist(ph, pols[bit]).max() < 2e-3 * N / 1024, bit
            for j in range(2 * p.l):
                ph = R.trlwe_phase(rp, key1, np.stack([sel[bit, 0, j], sel[bit, 1, j]])[None])[0].astype(np.int64)
                g = bit << (32 - p.bgbit * ((j % p.l) + 1))
                want = np.zeros(N, np.int64)
                if j < p.l:
                    want[0] = g
                else:
                    want = (-g * key1.astype(np.int64)) % 2 ** 32
                err = ((ph - want + 2 ** 31) % 2 ** 32) - 2 ** 31
                assert np.abs(err).max() < 2 ** 12, (bit, j)
    const = np.zeros((2, N), np.int32)
    const[1, 0] = 1
    _, b_poly = R.encrypt_trgsw_polys_seeded(rp, key1, const, noise_seed=0x5EED, seed=mseed, first_row=M64 - 12)
    assert np.array_equal(b_poly, b), "a constant polynomial mu = bit under the same seeds: the bit form's words"


def test_expanded_seeded_trgsw_polys_carry_the_polynomial():
    """rows k < l of an expanded polynomial sample decrypt to mu(X) * 2^(32 - (k+1) bgbit); rows l + k to -that * s(X)"""
    import rustfhe_amd as R
    p = R.Params(n=8)
    N = p.N
    rng = np.random.default_rng(9)
    key1 = rng.integers(0, 2, N).astype(np.int32)
    mu = rng.integers(-3, 4, (1, N)).astype(np.int32)
    seed, b = R.encrypt_trgsw_polys_seeded(p, key1, mu)
    ct = R.seeded_expand(p, seed, b, 2 * p.l)[0]
    s = key1.astype(np.int64)
    for k in range(p.l):
        m = (mu[0].astype(np.int64) << (32 - (k + 1) * p.bgbit)) % 2 ** 32
        ph = R.trlwe_phase(p, key1, np.stack([ct[0, k], ct[1, k]])[None])[0]
        assert torus_dist_lsb(ph, m.astype(np.uint32)).max() < 1 << 12, k
        ms = np.zeros(N, np.int64)                               # m(X) * s(X) mod X^N + 1
        for j in np.nonzero(s)[0]:
            ms[j:] += m[:N - j]
            ms[:j] -= m[N - j:]
        ph = R.trlwe_phase(p, key1, np.stack([ct[0, p.l + k], ct[1, p.l + k]])[None])[0]
        assert torus_dist_lsb(ph, ((-ms) % 2 ** 32).astype(np.uint32)).max() < 1 << 12, k


def test_expanded_seeded_packing_key_rows_decrypt_to_the_packing_keys_messages():
    """row (i, j, d) of the expanded key is a TRLWE of the constant (d + 1) key0[i] / 2^(2 (j + 1)), as rtfhe_packing_keygen's (alpha = 2^-25)"""
    import rustfhe_amd as R
    p = R.Params(n=3)
    key0, key1, _, _ = R.keygen(p, 0x9A, want_bk=False, want_ksk=False)
    key0[:] = [1, 0, 1]
    for kw in ({}, {"noise_seed": 5, "seed": np.arange(8), "first_row": 7}):
        seed, b = R.packing_keygen_seeded(p, key0, key1, **kw)
        assert b.shape == (p.n, 8, 3, p.N)
        pk = R.seeded_expand(p, seed, b, 1, first_row=kw.get("first_row", 0)).reshape(p.n, 8, 3, 2, p.N)
        ph = R.trlwe_phase(p, key1, pk.reshape(-1, 2, p.N)).reshape(p.n, 8, 3, p.N)
        want = np.zeros_like(ph)
        for i in range(p.n):
            for j in range(8):
                for d in range(3):
                    want[i, j, d, 0] = (d + 1) * int(key0[i]) << (32 - 2 * (j + 1))
        assert torus_dist_lsb(ph, want).max() < 1 << 12
    full = R.packing_keygen(p, key0, key1, seed=5)
    assert torus_dist_lsb(R.trlwe_phase(p, key1, full.reshape(-1, 2, p.N)).reshape(want.shape), want).max() < 1 << 12, "the unseeded key's messages are these"


def test_seeds_fresh_in_production_and_deterministic_forms_reproducible():
    import rustfhe_amd as R
    p = R.Params(n=8)
    rng = np.random.default_rng(4)
    key1 = rng.integers(0, 2, p.N).astype(np.int32)
    mu = random_words(rng, (2, p.N))
    s1, b1 = R.encrypt_lut_seeded(p, key1, mu)
    s2, b2 = R.encrypt_lut_seeded(p, key1, mu)
    assert not np.array_equal(s1, s2) and not np.array_equal(b1, b2) and s1.any() and s2.any()
    t1, _ = R.encrypt_selectors_seeded(p, key1, [1])
    t2, _ = R.encrypt_selectors_seeded(p, key1, [1])
    assert not np.array_equal(t1, t2)
    seed = random_words(rng, 8)
    _, a = R.encrypt_lut_seeded(p, key1, mu, noise_seed=11, seed=seed, first_row=3)
    _, a2 = R.encrypt_lut_seeded(p, key1, mu, noise_seed=11, seed=seed, first_row=3)
    _, c = R.encrypt_lut_seeded(p, key1, mu, noise_seed=12, seed=seed, first_row=3)
    assert np.array_equal(a, a2) and not np.array_equal(a, c), "reproducible; the b halves change with the noise seed"
    ea, ec = R.seeded_expand(p, seed, a, first_row=3), R.seeded_expand(p, seed, c, first_row=3)
    assert np.array_equal(ea[:, 1], ec[:, 1]), "the a halves depend on the seed only"
    # the noise does not come from the mask seed: the same noise seed under another mask seed gives the same noise
    other = random_words(rng, 8)
    _, d = R.encrypt_lut_seeded(p, key1, mu, noise_seed=11, seed=other, first_row=3)
    pa = R.trlwe_phase(p, key1, ea.reshape(2, 2, p.N))
    pd = R.trlwe_phase(p, key1, R.seeded_expand(p, other, d, first_row=3).reshape(2, 2, p.N))
    assert np.array_equal(pa, pd)


def test_entries_refuse_bad_arguments():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=8)
    N = p.N
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = R._ffi.ERR_INVALID
    seed = np.arange(8, dtype=np.uint32)
    b = np.zeros((6, N), np.uint32)
    out = np.zeros((12, N), np.uint32)
    pp = C.byref(p)
    assert L.rtfhe_mask_expand(N, ptr(seed), 0, ptr(out), 6) == 0
    assert L.rtfhe_mask_expand(N, None, 0, ptr(out), 6) == INV
    assert L.rtfhe_mask_expand(N, ptr(seed), 0, None, 6) == INV
    for bad_n in (0, 8, 24, 1000, 4096, -1024):
        assert L.rtfhe_mask_expand(bad_n, ptr(seed), 0, ptr(out), 1) == INV, bad_n
    assert L.rtfhe_mask_expand(N, ptr(seed), M64 - 6, ptr(out), 6) == 0
    assert L.rtfhe_mask_expand(N, ptr(seed), M64 - 5, ptr(out), 6) == INV        # first_row + rows = 2^64 + 1
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(b), 6, ptr(out), 6) == 0
    assert L.rtfhe_seeded_expand(None, ptr(seed), 0, ptr(b), 6, ptr(out), 6) == INV
    assert L.rtfhe_seeded_expand(pp, None, 0, ptr(b), 6, ptr(out), 6) == INV
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, None, 6, ptr(out), 6) == INV
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(b), 6, None, 6) == INV
    before = out.copy()
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(b), 0, ptr(out), 6) == INV           # group = 0
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(b), -1, ptr(out), 6) == INV
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(b), 4, ptr(out), 6) == INV           # rows % group != 0
    assert L.rtfhe_seeded_expand(pp, ptr(seed), M64 - 5, ptr(b), 6, ptr(out), 6) == INV      # first_row + rows = 2^64 + 1
    assert L.rtfhe_seeded_expand(pp, ptr(seed), 0, ptr(out), 6, ptr(out), 6) == INV         # b inside out
    assert np.array_equal(out, before), "a refused call writes nothing"
    bad = R.Params(n=8)
    bad.N = 1000
    assert L.rtfhe_seeded_expand(C.byref(bad), ptr(seed), 0, ptr(b), 6, ptr(out), 6) == INV
    # the encryptors
    key1 = np.zeros(N, np.int32)
    key0 = np.zeros(p.n, np.int32)
    mu = np.zeros((1, N), np.uint32)
    bits = np.array([1], np.uint8)
    sd = np.zeros(8, np.uint32)
    assert L.rtfhe_trlwe_encrypt_torus_seeded(pp, ptr(key1), ptr(mu), ptr(sd), ptr(b), 1) == 0
    for args in ((None, ptr(key1), ptr(mu), ptr(sd), ptr(b)), (pp, None, ptr(mu), ptr(sd), ptr(b)), (pp, ptr(key1), None, ptr(sd), ptr(b)),
                 (pp, ptr(key1), ptr(mu), None, ptr(b)), (pp, ptr(key1), ptr(mu), ptr(sd), None)):
        assert L.rtfhe_trlwe_encrypt_torus_seeded(*args, 1) == INV
        assert L.rtfhe_trgsw_encrypt_bits_seeded(*args, 1) == INV
        assert L.rtfhe_trgsw_encrypt_polys_seeded(*args, 1) == INV
    assert L.rtfhe_trgsw_encrypt_bits_seeded(pp, ptr(key1), ptr(bits), ptr(sd), ptr(b), 1) == 0
    assert L.rtfhe_trlwe_encrypt_torus_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), M64 - 1, ptr(mu), ptr(b), 1) == 0
    assert L.rtfhe_trlwe_encrypt_torus_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), M64 - 1, ptr(mu), ptr(b), 2) == INV
    assert L.rtfhe_trgsw_encrypt_bits_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), M64 - 6, ptr(bits), ptr(b), 1) == 0
    assert L.rtfhe_trgsw_encrypt_bits_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), M64 - 5, ptr(bits), ptr(b), 1) == INV
    assert L.rtfhe_trgsw_encrypt_polys_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), M64 - 5, ptr(mu.view(np.int32)), ptr(b), 1) == INV
    assert L.rtfhe_trgsw_encrypt_polys_seeded_deterministic(pp, ptr(key1), 1, None, 0, ptr(mu.view(np.int32)), ptr(b), 1) == INV
    pkb = np.zeros((p.n, 8, 3, N), np.uint32)
    assert L.rtfhe_packing_keygen_seeded_deterministic(pp, 1, ptr(key0), ptr(key1), ptr(seed), 0, ptr(pkb)) == 0
    assert L.rtfhe_packing_keygen_seeded_deterministic(pp, 1, ptr(key0), ptr(key1), ptr(seed), M64 - p.n * 24 + 1, ptr(pkb)) == INV
    assert L.rtfhe_packing_keygen_seeded(pp, None, ptr(key1), ptr(sd), ptr(pkb)) == INV
    assert L.rtfhe_packing_keygen_seeded(pp, ptr(key0), ptr(key1), None, ptr(pkb)) == INV
    key0[1] = 2                                                    # non-binary keys
    assert L.rtfhe_packing_keygen_seeded(pp, ptr(key0), ptr(key1), ptr(sd), ptr(pkb)) == INV
    key1[3] = 2
    assert L.rtfhe_trlwe_encrypt_torus_seeded(pp, ptr(key1), ptr(mu), ptr(sd), ptr(b), 1) == INV
    assert L.rtfhe_trgsw_encrypt_bits_seeded_deterministic(pp, ptr(key1), 1, ptr(seed), 0, ptr(bits), ptr(b), 1) == INV
    assert L.rtfhe_trgsw_encrypt_polys_seeded(pp, ptr(key1), ptr(mu.view(np.int32)), ptr(sd), ptr(b), 1) == INV
    # the device entry points: a null context (there is none without a GPU) is refused before anything else is looked at
    h = C.c_void_p()
    assert L.rtfhe_seeded_expand_dev(None, ptr(seed), 0, None, 1, None, 1, None) == INV
    assert L.rtfhe_trgsw_create_seeded(None, ptr(seed), 0, ptr(b), 1, C.byref(h)) == INV and not h.value
    assert L.rtfhe_trgsw_update_seeded(None, ptr(seed), 0, ptr(b), 0, 1) == INV
    assert L.rtfhe_lut_create_encrypted_seeded(None, ptr(seed), 0, ptr(b), 1, C.byref(h)) == INV and not h.value
    assert L.rtfhe_load_bk_seeded(None, ptr(seed), 0, ptr(b)) == INV
    assert L.rtfhe_packing_key_create_seeded(None, ptr(seed), 0, ptr(b), C.byref(h)) == INV and not h.value
