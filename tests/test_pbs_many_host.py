"""CPU: many-LUT programmable bootstrapping (include/rtfhe.h, rtfhe_pbs_many_batch) without a GPU -- the interleaving encoder
rustfhe_amd.many_lut_polynomial, the many-LUT PBS restated with the oracle's own building blocks (tests/pbs_oracle.py: oracle_pbs_many, which
tests/test_gpu_pbs_many.py compares the device's words with) and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
from pbs_oracle import FUNCS, bk_fft, coef0_after_rotation, oracle_pbs, oracle_pbs_many


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_one_function_is_lut_polynomial(N, P):
    import rustfhe_amd as R
    for fname in sorted(FUNCS):
        f = lambda m: FUNCS[fname](m, P)  # noqa: E731
        assert np.array_equal(R.many_lut_polynomial([f], N, P), R.lut_polynomial(f, N, P)), fname
    vals = [(3 * m + 1) % (1 << P) for m in range(1 << P)]
    assert np.array_equal(R.many_lut_polynomial([vals], N, P, out_bits=P + 1), R.lut_polynomial(vals, N, P, out_bits=P + 1))
    raw = [0x20000000 * (m + 1) for m in range(1 << P)]
    assert np.array_equal(R.many_lut_polynomial([raw], N, P, raw=True), R.lut_polynomial(raw, N, P, raw=True))


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("theta,P", [(1, 2), (2, 2), (4, 2), (8, 1), (2, 3), (4, 3), (8, 2), (8, 3)])
def test_every_coarse_rotation_of_every_box_gives_every_function(N, theta, P):
    """Noise-free: every rotation the coarse mod switch can produce for a phase in message m's box (the multiples of theta in
    [m B - B/2, m B + B/2), the wrap below 0 included) puts enc(f_j(m)) at coefficient j, for every j."""
    import rustfhe_amd as R
    names = sorted(FUNCS)
    fs = [(lambda k: (lambda m: FUNCS[names[k % len(names)]](m, P)))(k) for k in range(theta)]
    tv = R.many_lut_polynomial(fs, N, P)
    assert tv.dtype == np.uint32 and tv.shape == (N,)
    B = N >> P
    for m in range(1 << P):
        want = [int(R.encode_msgs([f(m)], P)[0]) for f in fs]
        start = m * B - B // 2
        assert start % theta == 0
        for k in range(start, m * B + B // 2, theta):
            for j in range(theta):
                assert coef0_after_rotation(tv, k + j) == want[j], (m, k, j)


def test_full_adder_table_and_out_bits():
    """The example adder's table: s = a + b + c in [0, 3] as a 2-bit message, (s & 1, s >> 1) out as 2-bit messages."""
    import rustfhe_amd as R
    N = 1024
    tv = R.many_lut_polynomial([lambda s: s & 1, lambda s: s >> 1], N, 2, out_bits=2)
    for s in range(4):
        for k in range(s * 256 - 128, s * 256 + 128, 2):
            assert coef0_after_rotation(tv, k) == (s & 1) << 29
            assert coef0_after_rotation(tv, k + 1) == (s >> 1) << 29


def test_encoder_errors():
    import rustfhe_amd as R
    f = lambda m: m  # noqa: E731
    for fs in ([], [f] * 3, [f] * 5, [f] * 16):
        with pytest.raises(ValueError):
            R.many_lut_polynomial(fs, 1024, 2)
    with pytest.raises(ValueError):
        R.many_lut_polynomial([[0, 1, 2], f], 1024, 2)          # a value list of the wrong length
    with pytest.raises(ValueError):
        R.many_lut_polynomial([f, lambda m: 4], 1024, 2)        # a value outside [0, 2^out_bits)
    # theta must not exceed half a box, N / 2^(p+1): at N = 1024, p = 7 leaves 4 coefficients, p = 8 leaves 2
    R.many_lut_polynomial([f] * 4, 1024, 7)
    with pytest.raises(ValueError):
        R.many_lut_polynomial([f] * 8, 1024, 7)
    with pytest.raises(ValueError):
        R.many_lut_polynomial([f] * 4, 1024, 8)
    with pytest.raises(ValueError):
        R.many_lut_polynomial([f] * 8, 2048, 8)
    with pytest.raises(ValueError):
        R.many_lut_polynomial([f], 1024, 10)


def test_oracle_restatement_with_one_output_is_oracle_pbs(orc):
    """n_out = 1 is rtfhe_pbs_batch: oracle_pbs_many(.., 1)[0] == oracle_pbs for random tables and random words (small n, N = 1024)."""
    p = orc.Params(n=24)
    plan = orc.Plan(p.N)
    keys = orc.Keys(p, 0x3A11, plan=plan)
    rng = np.random.default_rng(21)
    for _ in range(4):
        tv = rng.integers(0, 1 << 32, p.N, dtype=np.uint64).astype(np.uint32)
        t = rng.integers(0, 1 << 32, p.n + 1, dtype=np.uint64).astype(np.uint32)
        many = oracle_pbs_many(orc, p, plan, keys.bk_f, keys.ksk, tv, t, 1)
        assert many.shape == (1, p.n + 1)
        assert np.array_equal(many[0], oracle_pbs(orc, p, plan, keys.bk_f, keys.ksk, tv, t))


def test_oracle_many_pbs_decrypts_to_every_function(orc):
    """Keys from the product's keygen: 2-bit messages through two and four interleaved functions, every output decrypts."""
    import rustfhe_amd as R
    rp = R.Params(n=64)
    key0, key1, bk, ksk = R.keygen(rp, 0xB01)
    p = orc.Params(n=64)
    plan = orc.Plan(p.N)
    bk_f = bk_fft(orc, p, plan, bk)
    msgs = np.array([0, 1, 2, 3, 3, 0, 2, 1])
    cts = R.encrypt_torus(rp, key0, R.encode_msgs(msgs, 2), seed=0xC8)
    for fs in ([lambda s: s & 1, lambda s: s >> 1], [lambda s: s, lambda s: (s * s) % 4, lambda s: (s + 1) % 4, lambda s: 3 - s]):
        tv = R.many_lut_polynomial(fs, p.N, 2)
        outs = np.stack([oracle_pbs_many(orc, p, plan, bk_f, ksk, tv, t, len(fs)) for t in cts])
        assert outs.shape == (len(msgs), len(fs), p.n + 1)
        for j, f in enumerate(fs):
            assert list(R.decode_msgs(R.phases(rp, key0, outs[:, j]), 2)) == [f(m) for m in msgs], j


def test_pbs_many_entries_reject_null_handles_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    ct = np.zeros((1, 636), np.uint32)
    out = np.zeros((1, 2, 636), np.uint32)
    assert L.rtfhe_pbs_many_batch(None, None, 2, None, ct.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 1) == R._ffi.ERR_INVALID
    assert L.rtfhe_pbs_many_batch_dev(None, None, 2, None, None, None, 1, None) == R._ffi.ERR_INVALID
