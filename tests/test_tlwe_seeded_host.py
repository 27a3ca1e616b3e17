"""CPU: seeded lvl0 ciphertexts and the seeded key-switching key (include/rtfhe.h, "seeded lvl0 ciphertexts") without a GPU -- the host
expansions against the numpy restatement of the rule (tests/tlwe_seeded_oracle.py, which tests/test_gpu_tlwe_seeded.py's device words are held to
through the host expansion), the tie to the TRLWE rule, one RFC 8439 known answer, what the seeded encryptors' and the seeded key's words mean
once expanded, the seeds and the noise, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import tlwe_seeded_oracle as to
from kit import random_words, torus_dist_lsb
from seeded_oracle import KAT_KEY

M64 = 1 << 64
BOUND = 1 << 21      # sigma = 2^-15 is 2^17 LSB: the bound tests/test_abi.py holds the unseeded encryptor and key to


def _first_rows(rows):
    return (0, (1 << 32) - 2, M64 - rows)        # the carry into state word 15 between rows; the last rows there are


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32, 635, 766, 767])
def test_host_expansions_equal_the_oracle_word_for_word(n):
    import rustfhe_amd as R
    rng = np.random.default_rng(n)
    p = R.Params(n=n)
    for rows in (1, 5, 67):
        b = random_words(rng, rows)
        for first_row in _first_rows(rows):
            seed = random_words(rng, 8)
            a = R.tlwe_mask_expand(n, seed, rows, first_row=first_row)
            assert a.shape == (rows, n) and np.array_equal(a, to.mask_rows(n, seed, first_row, rows)), (rows, first_row)
            full = R.tlwe_seeded_expand(p, seed, b, first_row=first_row)
            assert full.shape == (rows, n + 1) and np.array_equal(full, to.expand(n, seed, first_row, b)), (rows, first_row)
            assert np.array_equal(full[:, :n], a) and np.array_equal(full[:, n], b)


@pytest.mark.parametrize("n", [16, 1024])
def test_rows_of_length_16k_are_the_trlwe_rules_masks(n):
    import rustfhe_amd as R
    seed = random_words(np.random.default_rng(n), 8)
    for first_row in _first_rows(3):
        assert np.array_equal(R.tlwe_mask_expand(n, seed, 3, first_row=first_row), R.mask_expand(n, seed, 3, first_row=first_row))


def test_rfc8439_2_4_2_keystream_through_the_new_call():
    """RFC 8439 2.4.2: key 00 .. 1f, nonce (0, 0x4a000000, 0), the keystream of block counter 1 -- words 16 .. 31 of row 0x4a000000; a row of
    n = 30 stops two words short of it"""
    import rustfhe_amd as R
    ks = bytes.fromhex("224f51f3401bd9e12fde276fb8631ded8c131f823d2c06e27e4fcaec9ef3cf78"
                       "8a3b0aa372600a92b57974cded2b9334794cba40c63e34cdea212c4cf07d41b7")
    want = np.frombuffer(ks, "<u4")
    assert np.array_equal(R.tlwe_mask_expand(32, KAT_KEY, 1, first_row=0x4A000000)[0, 16:], want)
    assert np.array_equal(R.tlwe_mask_expand(30, KAT_KEY, 1, first_row=0x4A000000)[0, 16:], want[:14])
    assert np.array_equal(to.mask_rows(32, KAT_KEY, 0x4A000000, 1)[0, 16:], want), "the oracle gives the same known answer"


@pytest.mark.parametrize("n", [40, 635])
def test_expanded_seeded_bits_and_torus_words_decrypt_as_the_unseeded_encryptors_do(n):
    import rustfhe_amd as R
    p = R.Params(n=n)
    rng = np.random.default_rng(n)
    key0 = rng.integers(0, 2, n).astype(np.int32)
    bits = rng.integers(0, 2, 24).astype(np.uint8)
    mu = random_words(rng, 24)
    want_bits = R.phases(p, key0, R.encrypt_bits(p, key0, bits, 3))
    for kw in ({}, {"noise_seed": 0xE17C, "seed": random_words(rng, 8), "first_row": (1 << 32) - 3}):
        first = kw.get("first_row", 0)
        seed, b = R.encrypt_bits_seeded(p, key0, bits, **kw)
        assert b.shape == (24,) and seed.shape == (8,)
        ct = R.tlwe_seeded_expand(p, seed, b, first_row=first)
        assert np.array_equal(ct[:, :n], to.mask_rows(n, seed, first, 24)), "the masks are the seed's keystream, all 32 bits"
        assert np.array_equal(R.decrypt_bits(p, key0, ct), bits)
        enc = np.where(bits == 1, 0x20000000, 0xE0000000).astype(np.uint32)
        assert torus_dist_lsb(R.phases(p, key0, ct), enc).max() < BOUND and torus_dist_lsb(want_bits, enc).max() < BOUND
        seed, b = R.encrypt_torus_seeded(p, key0, mu, **kw)
        ph = R.phases(p, key0, R.tlwe_seeded_expand(p, seed, b, first_row=first))
        assert torus_dist_lsb(ph, mu).max() < BOUND and np.any(ph != mu)
    assert torus_dist_lsb(R.phases(p, key0, R.encrypt_torus(p, key0, mu, 4)), mu).max() < BOUND, "the unseeded encryptor's words are held to the same"


def test_expanded_seeded_key_switching_rows_decrypt_to_their_messages():
    """row (i, l, d) of the expanded key: (d + 1) key1[i] 2^(32 - basebit (l + 1)) within 2^21, as tests/test_abi.py holds rtfhe_keygen's rows"""
    import rustfhe_amd as R
    p = R.Params(n=40)
    key0, key1, _, ksk = R.keygen(p, 5, want_bk=False, want_ksk=True)
    want = np.zeros((p.N, p.ks_t, 3), np.uint32)
    for l in range(p.ks_t):
        for d in range(3):
            want[:, l, d] = ((d + 1) * key1.astype(np.int64) << (32 - 2 * (l + 1))) % (1 << 32)
    for kw in ({}, {"noise_seed": 5, "seed": np.arange(8), "first_row": M64 - p.N * p.ks_t * 3}):
        seed, b = R.ksk_keygen_seeded(p, key0, key1, **kw)
        assert b.shape == (p.N, p.ks_t, 3)
        full = R.tlwe_seeded_expand(p, seed, b, first_row=kw.get("first_row", 0))
        assert full.shape == (p.N * p.ks_t * 3, p.n + 1)
        assert torus_dist_lsb(R.phases(p, key0, full).reshape(want.shape), want).max() < BOUND
    assert torus_dist_lsb(R.phases(p, key0, ksk.reshape(-1, p.n + 1)).reshape(want.shape), want).max() < BOUND, "the unseeded key's messages are these"


def test_keygen_seeded_returns_both_halves_under_independent_seeds():
    import rustfhe_amd as R
    p = R.Params(n=6)
    for s in (None, 7):
        key0, key1, (bk_seed, bk_b), (ksk_seed, ksk_b) = R.keygen_seeded(p, s)
        assert bk_b.shape == (p.n, 2 * p.l, p.N) and ksk_b.shape == (p.N, p.ks_t, 3) and not np.array_equal(bk_seed, ksk_seed)
        assert set(np.unique(key0)) <= {0, 1} and set(np.unique(key1)) <= {0, 1}
        full = R.tlwe_seeded_expand(p, ksk_seed, ksk_b)
        want = ((3 * key1[-1].astype(np.int64)) << 16) % (1 << 32)                 # row (N - 1, 7, 2)
        assert torus_dist_lsb(R.phases(p, key0, full[-1:]), np.uint32(want)).max() < BOUND
    again = R.keygen_seeded(p, 7)
    assert np.array_equal(again[3][1], ksk_b) and np.array_equal(again[2][1], bk_b), "an integer seed reproduces"


def test_seeds_fresh_in_production_and_deterministic_forms_reproducible():
    import rustfhe_amd as R
    p = R.Params(n=33)
    rng = np.random.default_rng(4)
    key0 = rng.integers(0, 2, p.n).astype(np.int32)
    key1 = rng.integers(0, 2, p.N).astype(np.int32)
    bits = rng.integers(0, 2, 5).astype(np.uint8)
    s1, b1 = R.encrypt_bits_seeded(p, key0, bits)
    s2, b2 = R.encrypt_bits_seeded(p, key0, bits)
    assert not np.array_equal(s1, s2) and not np.array_equal(b1, b2) and s1.any() and s2.any()
    t1, _ = R.encrypt_torus_seeded(p, key0, [1, 2])
    t2, _ = R.encrypt_torus_seeded(p, key0, [1, 2])
    k1, _ = R.ksk_keygen_seeded(p, key0, key1)
    k2, _ = R.ksk_keygen_seeded(p, key0, key1)
    assert not np.array_equal(t1, t2) and not np.array_equal(k1, k2)
    seed, other = random_words(rng, 8), random_words(rng, 8)
    for enc, msg in ((R.encrypt_bits_seeded, bits), (R.encrypt_torus_seeded, random_words(rng, 5))):
        _, a = enc(p, key0, msg, noise_seed=11, seed=seed, first_row=3)
        _, a2 = enc(p, key0, msg, noise_seed=11, seed=seed, first_row=3)
        _, c = enc(p, key0, msg, noise_seed=12, seed=seed, first_row=3)
        assert np.array_equal(a, a2) and not np.array_equal(a, c), "reproducible; b changes with the noise seed"
        ea, ec = R.tlwe_seeded_expand(p, seed, a, first_row=3), R.tlwe_seeded_expand(p, seed, c, first_row=3)
        assert np.array_equal(ea[:, :p.n], ec[:, :p.n]), "the masks depend on the seed only"
        # the noise does not come from the mask seed: the same noise seed under another mask seed gives the same phases
        _, d = enc(p, key0, msg, noise_seed=11, seed=other, first_row=3)
        assert np.array_equal(R.phases(p, key0, ea), R.phases(p, key0, R.tlwe_seeded_expand(p, other, d, first_row=3)))
    _, ka = R.ksk_keygen_seeded(p, key0, key1, noise_seed=11, seed=seed, first_row=9)
    _, ka2 = R.ksk_keygen_seeded(p, key0, key1, noise_seed=11, seed=seed, first_row=9)
    _, kd = R.ksk_keygen_seeded(p, key0, key1, noise_seed=11, seed=other, first_row=9)
    assert np.array_equal(ka, ka2) and not np.array_equal(ka, kd)
    assert np.array_equal(R.phases(p, key0, R.tlwe_seeded_expand(p, seed, ka, first_row=9)), R.phases(p, key0, R.tlwe_seeded_expand(p, other, kd, first_row=9)))


def _plan(L):
    f = L.rtfhe_tlwe_seeded_plan
    f.restype = C.c_int
    f.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return f


def test_every_refusal_of_the_plan():
    """addresses only: the plan never dereferences b or out.  what: 0 the CPU form, 1 the device form, 2 an upload"""
    import rustfhe_amd as R
    plan = _plan(R.load())
    INV = R._ffi.ERR_INVALID
    seed = np.arange(8, dtype=np.uint32).ctypes.data
    B, OUT = 0x10000000, 0x40000000

    def run(what=1, n=635, sd=seed, first_row=0, b=B, out=OUT, rows=4):
        err = C.create_string_buffer(b"x" * 199, 200)
        return plan(what, n, sd, first_row, b, out, rows, err, 200), err.value.decode()

    for kw in ({}, {"what": 0}, {"what": 2, "out": None}, {"n": 1}, {"n": 767}, {"what": 0, "n": 5000}, {"first_row": M64 - 4}, {"b": B + 4, "out": OUT + 12},
               {"rows": 0x7fffffff // 40}, {"what": 0, "rows": 0x7fffffff // 40 + 1}, {"out": B + 16}, {"out": B - 4 * 636 * 4}):
        assert run(**kw) == (0, ""), kw
    for kw, word in (({"sd": None}, "null"), ({"b": None}, "null"), ({"out": None}, "null"), ({"what": 0, "out": None}, "null"), ({"what": 2, "b": None}, "null"),
                     ({"n": 0}, "n = 0"), ({"what": 0, "n": -3}, "n = -3"), ({"n": 768}, "n = 768"), ({"what": 2, "n": 768}, "n = 768"),
                     ({"rows": 0}, "rows = 0"), ({"what": 2, "rows": 0}, "rows = 0"),
                     ({"first_row": M64 - 3}, "pass 2^64"), ({"what": 2, "first_row": M64 - 1, "rows": 2}, "pass 2^64"),
                     ({"rows": 0x7fffffff // 40 + 1}, "too large"), ({"what": 2, "n": 1, "rows": 1 << 31}, "too large"), ({"what": 0, "rows": 1 << 62}, "too large"),
                     ({"b": B + 2}, "aligned"), ({"out": OUT + 1}, "aligned"),
                     ({"out": B}, "overlaps"), ({"out": B + 12}, "overlaps"), ({"out": B - 4 * 636 * 4 + 4}, "overlaps")):
        rc, msg = run(**kw)
        assert rc == INV and word in msg, (kw, msg)
    assert plan(1, 768, seed, 0, B, OUT, 4, None, 0) == INV, "no err at all is fine"


def test_entries_refuse_bad_arguments_and_leave_the_output_untouched():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=20)
    n = p.n
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = R._ffi.ERR_INVALID
    pp = C.byref(p)
    seed = np.arange(8, dtype=np.uint32)
    both = np.full(6 * (n + 1) + 6, 0x5A5A5A5A, np.uint32)          # b [6] and out [6][n+1] in one allocation
    b, out = both[:6], both[6:]
    a = np.full((6, n), 0x5A5A5A5A, np.uint32)
    assert L.rtfhe_tlwe_mask_expand(n, ptr(seed), M64 - 6, ptr(a), 6) == 0
    a[:] = 0x5A5A5A5A
    for args in ((n, None, 0, ptr(a), 6), (n, ptr(seed), 0, None, 6), (0, ptr(seed), 0, ptr(a), 6), (-16, ptr(seed), 0, ptr(a), 6),
                 (n, ptr(seed), 0, ptr(a), 0), (n, ptr(seed), M64 - 5, ptr(a), 6)):
        assert L.rtfhe_tlwe_mask_expand(*args) == INV, args
    assert (a == 0x5A5A5A5A).all()
    assert L.rtfhe_tlwe_seeded_expand(pp, ptr(seed), M64 - 6, ptr(b), ptr(out), 6) == 0
    both[:] = 0x5A5A5A5A
    bad = R.Params(n=20)
    bad.n = 0
    for args in ((None, ptr(seed), 0, ptr(b), ptr(out), 6), (pp, None, 0, ptr(b), ptr(out), 6), (pp, ptr(seed), 0, None, ptr(out), 6),
                 (pp, ptr(seed), 0, ptr(b), None, 6), (pp, ptr(seed), 0, ptr(b), ptr(out), 0), (pp, ptr(seed), M64 - 5, ptr(b), ptr(out), 6),
                 (pp, ptr(seed), 0, ptr(out[3:]), ptr(out), 6), (pp, ptr(seed), 0, ptr(b), ptr(both[5:]), 6), (C.byref(bad), ptr(seed), 0, ptr(b), ptr(out), 6)):
        assert L.rtfhe_tlwe_seeded_expand(*args) == INV
    assert (both == 0x5A5A5A5A).all(), "a refused call writes nothing"
    # the encryptors and the key generation
    key0, key1 = np.zeros(n, np.int32), np.zeros(p.N, np.int32)
    bits, mu, sd = np.array([1, 0], np.uint8), np.zeros(2, np.uint32), np.zeros(8, np.uint32)
    kb = np.full(p.N * p.ks_t * 3, 0x5A5A5A5A, np.uint32)
    eb = np.full(2, 0x5A5A5A5A, np.uint32)
    for f, msg in ((L.rtfhe_tlwe_encrypt_bits_seeded, bits), (L.rtfhe_tlwe_encrypt_torus_seeded, mu)):
        for args in ((None, ptr(key0), ptr(msg), ptr(sd), ptr(eb)), (pp, None, ptr(msg), ptr(sd), ptr(eb)), (pp, ptr(key0), None, ptr(sd), ptr(eb)),
                     (pp, ptr(key0), ptr(msg), None, ptr(eb)), (pp, ptr(key0), ptr(msg), ptr(sd), None), (C.byref(bad), ptr(key0), ptr(msg), ptr(sd), ptr(eb))):
            assert f(*args, 2) == INV
    for f, msg in ((L.rtfhe_tlwe_encrypt_bits_seeded_deterministic, bits), (L.rtfhe_tlwe_encrypt_torus_seeded_deterministic, mu)):
        assert f(pp, ptr(key0), 1, ptr(seed), M64 - 1, ptr(msg), ptr(eb), 2) == INV          # first_row + count = 2^64 + 1
        assert f(pp, ptr(key0), 1, None, 0, ptr(msg), ptr(eb), 2) == INV
    for args in ((None, ptr(key0), ptr(key1), ptr(sd), ptr(kb)), (pp, None, ptr(key1), ptr(sd), ptr(kb)), (pp, ptr(key0), None, ptr(sd), ptr(kb)),
                 (pp, ptr(key0), ptr(key1), None, ptr(kb)), (pp, ptr(key0), ptr(key1), ptr(sd), None)):
        assert L.rtfhe_ksk_keygen_seeded(*args) == INV
    assert L.rtfhe_ksk_keygen_seeded_deterministic(pp, 1, ptr(key0), ptr(key1), ptr(seed), M64 - kb.size + 1, ptr(kb)) == INV
    key0[1] = 2                                                    # non-binary keys
    assert L.rtfhe_tlwe_encrypt_bits_seeded(pp, ptr(key0), ptr(bits), ptr(sd), ptr(eb), 2) == INV
    assert L.rtfhe_tlwe_encrypt_torus_seeded_deterministic(pp, ptr(key0), 1, ptr(seed), 0, ptr(mu), ptr(eb), 2) == INV
    assert L.rtfhe_ksk_keygen_seeded(pp, ptr(key0), ptr(key1), ptr(sd), ptr(kb)) == INV
    key0[1], key1[5] = 0, -1
    assert L.rtfhe_ksk_keygen_seeded_deterministic(pp, 1, ptr(key0), ptr(key1), ptr(seed), 0, ptr(kb)) == INV
    assert (kb == 0x5A5A5A5A).all() and (eb == 0x5A5A5A5A).all() and not sd.any(), "a refused call writes neither b nor the seed"
    key1[5] = 0
    assert L.rtfhe_tlwe_encrypt_bits_seeded_deterministic(pp, ptr(key0), 1, ptr(seed), M64 - 2, ptr(bits), ptr(eb), 2) == 0
    assert L.rtfhe_ksk_keygen_seeded_deterministic(pp, 1, ptr(key0), ptr(key1), ptr(seed), M64 - kb.size, ptr(kb)) == 0
    # the device entry points: a null context (there is none without a GPU) is refused before anything else is looked at
    assert L.rtfhe_tlwe_seeded_expand_dev(None, ptr(seed), 0, None, None, 1, None) == INV
    assert L.rtfhe_load_ksk_seeded(None, ptr(seed), 0, ptr(kb)) == INV
