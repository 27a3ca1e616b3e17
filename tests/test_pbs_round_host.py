"""CPU: the rounded gadget decomposition of the PBS family (include/rtfhe.h: rtfhe_set_decomposition) without a GPU -- the restatement of the
external product with a choice of constants (tests/round_oracle.py, which tests/test_gpu_pbs_round.py compares the device's words with)
against the oracle's own product, the digit identity, the noise it buys at n = 635, N = 1024, and the entry points' argument checks."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
import round_oracle as ro
from kit import random_words
from pbs_oracle import oracle_pbs, oracle_pbs_many

U32 = 0xFFFFFFFF


def test_constants():
    assert ro.constants(3, 6, ro.REFERENCE) == (0x02084000, 0x02084000)
    assert ro.constants(3, 6, ro.ROUNDED) == (0x82082000, 0x82080000)


@pytest.mark.parametrize("N", [1024, 2048])
def test_reference_constants_give_the_oracles_product_and_cmux(orc, N):
    """MA = MX = make_decomp_mask: the restatement is orc_external_product and orc_cmux word for word, on random words."""
    p = orc.Params(n=2, N=N)
    plan = orc.Plan(N)
    keys = orc.Keys(p, 0x51 + N, plan=plan)
    ma, mx = ro.constants(p.l, p.bgbit, ro.REFERENCE)
    rng = np.random.default_rng(N)
    trgsw = p.trgsw_words
    for i in range(p.n):
        bki = np.ascontiguousarray(keys.bk_f[i * trgsw:(i + 1) * trgsw])
        x, y = random_words(rng, 2 * N), random_words(rng, 2 * N)
        assert np.array_equal(ro.external_product(p, plan, bki, x, ma, mx), orc.external_product(p, plan, bki, None, x))
        exp = np.empty(2 * N, np.uint32)
        orc.lib().orc_cmux(C.byref(p), plan.h, bki.ctypes.data_as(C.POINTER(C.c_double)), None, x.ctypes.data_as(C.POINTER(C.c_uint32)),
                           y.ctypes.data_as(C.POINTER(C.c_uint32)), exp.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert np.array_equal(ro.cmux(p, plan, bki, x, y, ma, mx), exp)
    # ... and with the rounded constants it is another product
    mar, mxr = ro.constants(p.l, p.bgbit, ro.ROUNDED)
    assert not np.array_equal(ro.external_product(p, plan, bki, x, mar, mxr), ro.external_product(p, plan, bki, x, ma, mx))


def test_reference_mode_pbs_is_oracle_pbs(orc):
    """n = 24: the PBS built on the restatement equals oracle_pbs (and oracle_pbs_many) in reference mode, for random tables and words."""
    p = orc.Params(n=24)
    plan = orc.Plan(p.N)
    keys = orc.Keys(p, 0x51, plan=plan)
    rng = np.random.default_rng(24)
    for _ in range(2):
        tv, t = random_words(rng, p.N), random_words(rng, p.n + 1)
        assert np.array_equal(ro.pbs(p, plan, keys.bk_f, keys.ksk, tv, t, ro.REFERENCE), oracle_pbs(orc, p, plan, keys.bk_f, keys.ksk, tv, t))
    tv, t = random_words(rng, p.N), random_words(rng, p.n + 1)
    assert np.array_equal(ro.pbs_many(p, plan, keys.bk_f, keys.ksk, tv, t, 4, ro.REFERENCE), oracle_pbs_many(orc, p, plan, keys.bk_f, keys.ksk, tv, t, 4))
    assert not np.array_equal(ro.pbs(p, plan, keys.bk_f, keys.ksk, tv, t, ro.ROUNDED), ro.pbs(p, plan, keys.bk_f, keys.ksk, tv, t, ro.REFERENCE))


EDGES = [0, (1 << 13) - 1, 1 << 13, 0x7fffffff, 0x80000000, 0xffffffff]


def _decomp_error(x, d):
    """x - sum_j d_j 2^(32 - 6 (j+1)), wrapped into [-2^31, 2^31)"""
    rec = sum(d[j].astype(np.int64) << (32 - 6 * (j + 1)) for j in range(3))
    return ((x.astype(np.int64) - rec + (1 << 31)) & U32) - (1 << 31)


def test_rounded_digits_are_balanced_and_round_to_nearest():
    rng = np.random.default_rng(0xD161)
    x = np.concatenate([random_words(rng, 1 << 16), np.array(EDGES, np.uint32)])
    ma, mx = ro.constants(3, 6, ro.ROUNDED)
    d = ro.digits(x, 3, 6, ma, mx)
    assert d.min() >= -32 and d.max() <= 31
    err = _decomp_error(x, d)
    assert err.min() >= -(1 << 13) and err.max() < (1 << 13)
    assert abs(err.mean()) < (1 << 13) / 50, err.mean()
    # the same figures of the reference's constants, for the record: not nearest, and biased by half a unit of the last digit
    m, _ = ro.constants(3, 6, ro.REFERENCE)
    eref = _decomp_error(x, ro.digits(x, 3, 6, m, m))
    assert eref.min() < -(1 << 13) and abs(eref.mean() + (1 << 13)) < (1 << 13) / 50, (eref.min(), eref.max(), eref.mean())


def test_rounded_mode_carries_4bit_messages_at_n635(orc, params, keys):
    """n = 635, N = 1024, the suite's key set: 64 seeded fresh 4-bit ciphertexts through the table m -> 3m + 1 mod 16 in both modes.  Rounded:
    every output decodes right and the rms phase error after the key switch is below half of reference mode's on the same inputs (a float
    model of the blind rotation gives a ratio of 0.23: rounded 0.0025, reference 0.0111; the margin covers 64 samples)."""
    import rustfhe_amd as R
    P = 4
    rp = R.Params(n=params.n, N=params.N)
    plan = orc.Plan(params.N)
    msgs = np.arange(64) % 16
    f = lambda m: (3 * m + 1) % 16  # noqa: E731
    tv = R.lut_polynomial(f, params.N, P)
    cts = R.encrypt_torus(rp, keys.key0, R.encode_msgs(msgs, P), seed=0x4B17)
    want = np.array([f(m) for m in msgs])
    rms = {}
    for mode in (ro.ROUNDED, ro.REFERENCE):
        out = np.stack([ro.pbs(params, plan, keys.bk_f, keys.ksk, tv, t, mode) for t in cts])
        ph = R.phases(rp, keys.key0, out)
        d = (ph.astype(np.int64) - R.encode_msgs(want, P).astype(np.int64)) & U32
        err = np.where(d >= 1 << 31, d - (1 << 32), d) / 2.0 ** 32
        rms[mode] = float(np.sqrt(np.mean(err ** 2)))
        print("mode %d: rms %.5f max %.5f wrong %d" % (mode, rms[mode], np.abs(err).max(), int(np.sum(R.decode_msgs(ph, P) != want))))
        if mode == ro.ROUNDED:
            assert np.array_equal(R.decode_msgs(ph, P), want)
    assert rms[ro.ROUNDED] < 0.5 * rms[ro.REFERENCE], rms


def test_decomposition_entries_reject_null_handles_and_bad_modes_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    assert (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED) == (0, 1)
    for mode in (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED, 2, -1, 1 << 20):
        assert L.rtfhe_set_decomposition(None, mode) == R._ffi.ERR_INVALID
    assert L.rtfhe_get_decomposition(None) == R._ffi.ERR_INVALID
