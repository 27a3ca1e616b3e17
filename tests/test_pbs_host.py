"""CPU: programmable bootstrapping (include/rtfhe.h, rtfhe_pbs_batch) without a GPU -- the encoder of rustfhe_amd.pbs, the PBS restated with
the oracle's own building blocks (negacyclic rotation, CMUX, sample extract, key switch), torus encryption and the entry points' argument checks.
oracle_pbs (tests/pbs_oracle.py) is also what tests/test_gpu_pbs.py compares the device's words with."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from pbs_oracle import FUNCS, U32, bk_fft, coef0_after_rotation, oracle_pbs

@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("fname", sorted(FUNCS))
def test_encoder_every_rotation_of_every_box(N, P, fname):
    import rustfhe_amd as R
    f = lambda m: FUNCS[fname](m, P)  # noqa: E731
    tv = R.lut_polynomial(f, N, P)
    assert tv.dtype == np.uint32 and tv.shape == (N,)
    B = N >> P
    for m in range(1 << P):
        want = int(R.encode_msgs([f(m)], P)[0])
        # every mod-switched phase of the message's box, m B - B/2 .. m B + B/2 - 1, including the wrap below 0 (= k >= N after mod 2N)
        for k in range(m * B - B // 2, m * B + B // 2):
            assert coef0_after_rotation(tv, k) == want, (m, k)


def test_encoder_out_bits_and_raw_words():
    import rustfhe_amd as R
    N = 1024
    tv = R.lut_polynomial(lambda m: m >= 2, N, 2, out_bits=1)        # 2-bit in, 1-bit out
    for m in range(4):
        for k in range(m * 256 - 128, m * 256 + 128):
            assert coef0_after_rotation(tv, k) == int(m >= 2) << 30
    gate = R.lut_polynomial([0xE0000000, 0x20000000], N, 1, raw=True)   # a 1-bit message to -+1/8: the gates' encoding
    for k in range(-256, 256):
        assert coef0_after_rotation(gate, k) == 0xE0000000
    for k in range(256, 768):
        assert coef0_after_rotation(gate, k) == 0x20000000
    with pytest.raises(ValueError):
        R.lut_polynomial(lambda m: 4, N, 2)
    with pytest.raises(ValueError):
        R.encode_msgs([4], 2)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 6])
def test_encode_decode_roundtrip(P):
    import rustfhe_amd as R
    m = np.arange(1 << P)
    mu = R.encode_msgs(m, P)
    assert mu.dtype == np.uint32 and np.array_equal(mu.astype(np.int64), m << (32 - P - 1))
    assert np.array_equal(R.decode_msgs(mu, P), m)
    # noise of up to just under half a box either way, below zero included
    half = 1 << (32 - P - 2)
    for d in (1, -1, half - 1, -(half - 1)):
        assert np.array_equal(R.decode_msgs((mu.astype(np.int64) + d) & U32, P), m)


def test_oracle_pbs_with_the_gate_vector_is_the_oracle_bootstrap(orc):
    """tv = 1/8 everywhere: the restated PBS gives orc.gate(COPY)'s bootstrap word for word (small n, N = 1024)."""
    p = orc.Params(n=24)
    plan = orc.Plan(p.N)
    keys = orc.Keys(p, 0x5EED, plan=plan)
    tv = np.full(p.N, 0x20000000, np.uint32)
    rng = np.random.default_rng(7)
    cts = keys.encrypt_bits(rng.integers(0, 2, 6))
    cts[3] = rng.integers(0, 1 << 32, p.n + 1, dtype=np.uint64).astype(np.uint32)    # any words at all, not only fresh ciphertexts
    for t in cts:
        exp = orc.gate(p, plan, orc.COPY, keys.bk_f, None, keys.ksk, t, None)
        assert np.array_equal(oracle_pbs(orc, p, plan, keys.bk_f, keys.ksk, tv, t), exp)


def test_oracle_pbs_of_a_2bit_lut_decrypts_to_f(orc):
    """Keys from the product's keygen (deterministic seed) and its torus encryption: every 2-bit message through a non-linear table."""
    import rustfhe_amd as R
    rp = R.Params(n=64)
    key0, key1, bk, ksk = R.keygen(rp, 0xB00)
    p = orc.Params(n=64)
    plan = orc.Plan(p.N)
    bk_f = bk_fft(orc, p, plan, bk)
    f = lambda m: (m * m + 1) % 4  # noqa: E731
    tv = R.lut_polynomial(f, p.N, 2)
    msgs = np.array([0, 1, 2, 3, 3, 0])
    cts = R.encrypt_torus(rp, key0, R.encode_msgs(msgs, 2), seed=0xC7)
    outs = np.stack([oracle_pbs(orc, p, plan, bk_f, ksk, tv, t) for t in cts])
    assert list(R.decode_msgs(R.phases(rp, key0, outs), 2)) == [f(m) for m in msgs]


def test_encrypt_torus_deterministic_noise_and_fresh():
    import rustfhe_amd as R
    rp = R.Params()
    key0, _, _, _ = R.keygen(rp, 0xE7, want_bk=False, want_ksk=False)
    rng = np.random.default_rng(3)
    mu = rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    a = R.encrypt_torus(rp, key0, mu, seed=99)
    assert a.shape == (1000, rp.n + 1)
    assert np.array_equal(a, R.encrypt_torus(rp, key0, mu, seed=99))
    assert not np.array_equal(a, R.encrypt_torus(rp, key0, mu, seed=100))
    err = ((R.phases(rp, key0, a).astype(np.int64) - mu.astype(np.int64) + (1 << 31)) & U32) - (1 << 31)
    assert np.abs(err).max() <= 6 * 2 ** -15 * 2 ** 32
    # the production form draws from the OS CSPRNG: two calls differ, both decrypt
    b, c = R.encrypt_torus(rp, key0, mu), R.encrypt_torus(rp, key0, mu)
    assert not np.array_equal(b, c)
    for x in (b, c):
        e = ((R.phases(rp, key0, x).astype(np.int64) - mu.astype(np.int64) + (1 << 31)) & U32) - (1 << 31)
        assert np.abs(e).max() <= 6 * 2 ** -15 * 2 ** 32
    # the bits form is the torus form of -+1/8
    bits = rng.integers(0, 2, 64).astype(np.uint8)
    mu8 = np.where(bits == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    assert np.array_equal(R.encrypt_bits(rp, key0, bits, seed=5), R.encrypt_torus(rp, key0, mu8, seed=5))


def test_pbs_entries_reject_null_handles_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    tv = np.zeros(1024, np.uint32)
    h = C.c_void_p()
    assert L.rtfhe_lut_create(None, tv.ctypes.data_as(C.c_void_p), 1, C.byref(h)) == R._ffi.ERR_INVALID and not h.value
    ct = np.zeros((1, 636), np.uint32)
    assert L.rtfhe_pbs_batch(None, None, None, ct.ctypes.data_as(C.c_void_p), ct.ctypes.data_as(C.c_void_p), 1) == R._ffi.ERR_INVALID
    assert L.rtfhe_pbs_batch_dev(None, None, None, None, None, 1, None) == R._ffi.ERR_INVALID
    L.rtfhe_lut_destroy(None)
    p = R.Params()
    assert L.rtfhe_tlwe_encrypt_torus(C.byref(p), None, None, None, 1) == R._ffi.ERR_INVALID
