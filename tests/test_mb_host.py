"""CPU: the host side of the multi-bit blind rotation (include/rtfhe.h: rtfhe_mbk_*, rtfhe_mb_roots, rtfhe_mb_point_exponents).  The two
tables of the key combination on their own -- the roots against numpy, the point map against the oracle's forward transform of monomials --,
the key's sizes, every TRGSW row of a generated key by its phase under key1, and tests/mb_oracle.py itself: its steps give the message the
single-bit PBS gives.  Nothing here needs a GPU."""
import numpy as np
import pytest

import mb_oracle as mo
import round_oracle as ro


@pytest.mark.parametrize("N", [1024, 2048])
def test_roots_table_against_numpy(N):
    """Every component within 2^-51 of numpy's cos / sin of pi t / N; W[0] = 1 exactly."""
    import rustfhe_amd as R
    W = R.mb_roots(N)
    assert W.shape == (2 * N, 2) and W[0, 0] == 1.0 and W[0, 1] == 0.0
    x = np.pi * np.arange(2 * N) / N
    assert np.abs(W[:, 0] - np.cos(x)).max() <= 2.0 ** -51 and np.abs(W[:, 1] - np.sin(x)).max() <= 2.0 ** -51
    for bad in (0, -1024, 1000, 1 << 30):
        with pytest.raises(R.RtfheError):
            R.mb_roots(bad)
    for bad in (0, 64, 1536):
        with pytest.raises(R.RtfheError):
            R.mb_point_exponents(bad)


@pytest.mark.parametrize("N", [1024, 2048])
def test_point_map_against_the_oracle_transform_of_monomials(orc, N):
    """The oracle's forward transform of the signed monomial X^e equals W[(e q_p) mod 2N] times the transform of the constant 1 at every point,
    to 2^-40 relative (an FP64 transform of a monomial errs by about log N * 2^-53; a wrong map is off by order 1)."""
    import rustfhe_amd as R
    tab = mo.Tables(R, N)
    plan = orc.Plan(N)
    P = N // 2
    assert sorted(R.mb_point_exponents(N).tolist()) == list(range(1, 2 * N, 4))
    one = np.zeros(N, np.int32)
    one[0] = 1
    u = plan.ifft_i32(one)
    u = u[:P] + 1j * u[P:]
    for e in (0, 1, 2, N - 1, N, N + 1, 2 * N - 1):
        mono = np.zeros(N, np.int32)
        mono[e % N] = 1 if e < N else -1
        v = plan.ifft_i32(mono)
        v = v[:P] + 1j * v[P:]
        w = tab.W[(e * tab.q) % (2 * N)]
        want = (w[:, 0] + 1j * w[:, 1]) * u
        assert np.abs(v - want).max() <= 2.0 ** -40 * np.abs(want).max(), e
        fx, fy = tab.F(e)
        assert np.abs((v - u) - (fx + 1j * fy) * u).max() <= 2.0 ** -40, e
    assert all((x == 0).all() for x in tab.F(0)), "F_0 is exactly zero"


def test_key_sizes():
    import rustfhe_amd as R
    p = R.Params()
    assert R.mbk_words(p, 2) == 952 * 12 * 1024 and R.mbk_words(p, 3) == 1480 * 12 * 1024
    for n, g, want in ((1, 2, 1), (1, 3, 1), (2, 2, 3), (2, 3, 3), (3, 2, 4), (3, 3, 7), (5, 2, 7), (5, 3, 10), (7, 2, 10), (7, 3, 15)):
        assert R.mbk_words(R.Params(n=n), g) == want * 12 * 1024 == mo.trgsw_count(n, g) * 12 * 1024
    for g in (0, 1, 4, -2):
        with pytest.raises(R.RtfheError):
            R.mbk_words(p, g)
        with pytest.raises(R.RtfheError):
            R.mbk_keygen(R.Params(n=5), np.zeros(5, np.int32), np.zeros(1024, np.int32), g, seed=1)
    with pytest.raises(R.RtfheError):      # a non-binary key
        R.mbk_keygen(R.Params(n=5), np.array([0, 1, 2, 0, 1], np.int32), np.zeros(1024, np.int32), 2, seed=1)


KEY0S = ([1, 0, 0, 0, 1], [0, 1, 1, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], None)      # None: the generated key


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("seed", [11, None])
def test_every_key_row_decrypts_to_its_constant_times_the_gadget(g, seed):
    """n = 5: every TRGSW row of every subset of every group, under key1, within the bootstrapping key's noise bound (2^12 LSB: alpha = 2^-25
    is 2^7 LSB); exactly one entry of a group holds 1, unless all its bits are 0."""
    import rustfhe_amd as R
    p = R.Params(n=5)
    gen0, key1, _, _ = R.keygen(p, 0x4D42, want_bk=False, want_ksk=False)
    for k0 in KEY0S:
        key0 = gen0 if k0 is None else np.array(k0, np.int32)
        mbk = R.mbk_keygen(p, key0, key1, g, seed=seed)
        assert mbk.shape == (mo.trgsw_count(p.n, g), 2, 2 * p.l, p.N)
        if seed is not None:
            assert np.array_equal(mbk, R.mbk_keygen(p, key0, key1, g, seed=seed))
        for i0, bits, first in mo.groups(p.n, g):
            held = []
            for j in range(1, 1 << bits):
                mu = int(all(int(key0[i0 + q]) == ((j >> q) & 1) for q in range(bits)))
                held.append(mu)
                ct = mbk[first + j - 1]
                rows = np.stack([ct[0], ct[1]], axis=1)                # [2l][2][N]: (b, a) of every row
                ph = R.trlwe_phase(p, key1, rows).astype(np.int64)
                for r in range(2 * p.l):
                    gad = mu << (32 - p.bgbit * (r % p.l + 1))
                    want = np.zeros(p.N, np.int64)
                    if r < p.l:
                        want[0] = gad                                  # b += mu / Bg^(r+1)
                    else:
                        want = (-gad * key1.astype(np.int64)) % 2 ** 32      # a += mu / Bg^(r+1): the phase gains -gad s(X)
                    err = ((ph[r] - want + 2 ** 31) % 2 ** 32) - 2 ** 31
                    assert np.abs(err).max() < 2 ** 12, (k0, i0, j, r)
            assert sum(held) == (1 if any(key0[i0:i0 + bits]) else 0), (k0, i0)


@pytest.mark.parametrize("g", [2, 3])
def test_the_oracle_steps_compute_the_single_bit_message(orc, g):
    """mb_oracle at n = 7 (a one-bit tail at g = 2 and at g = 3), both decomposition modes: every 2-bit message decodes to its table entry, as
    the single-bit PBS of round_oracle does; planted rotations 0, 1, N, 2N - 1 and a group summing to 0 mod 2N change the words, not the
    message's validity (the phase moves by the planted mask words only where the key bit is set)."""
    import rustfhe_amd as R
    N, n = 1024, 7
    P = orc.Params(n=n, N=N)
    plan = orc.Plan(N)
    K = orc.Keys(P, 0x4D42 + g, plan=plan)
    rp = R.Params(n=n, N=N)
    tab = mo.Tables(R, N)
    key_f = mo.key_spectra(P, plan, R.mbk_keygen(rp, K.key0, K.key1, g, seed=7))
    perm = [2, 0, 3, 1]
    tv = R.lut_polynomial(perm, N, 2)
    msgs = np.array([0, 1, 2, 3])
    ct = R.encrypt_torus(rp, K.key0, R.encode_msgs(msgs, 2), seed=9)
    for mode in (ro.REFERENCE, ro.ROUNDED):
        out = np.stack([mo.pbs_mb(P, plan, tab, key_f, K.ksk, tv, c, g, mode) for c in ct])
        assert list(R.decode_msgs(R.phases(rp, K.key0, out), 2)) == [perm[m] for m in msgs], mode
    # exponents: a group of g rotations summing to 2N gives e = 0 for the full subset
    assert mo.exponents([1, 2 * N - 1], N) == [1, 2 * N - 1, 0] and mo.exponents([1, N, N - 1], N)[-1] == 0
    planted = mo.plant(P, ct[0], [0, 1, N, 2 * N - 1])
    assert mo.rotations(P, planted)[1][:4] == [0, 1, N, 2 * N - 1]
