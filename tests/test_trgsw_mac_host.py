"""CPU: the TRLWE x TRGSW multiply-accumulate (include/rtfhe.h: rtfhe_trlwe_mul_trgsw_batch, rtfhe_trgsw_encrypt_polys) without a device -- the
restatement the GPU tests compare every word to (tests/trgsw_mac_oracle.py) against the oracle's own external product, the TRGSW encryption of
integer polynomials against the bits' and against its phases, the meaning of a sum of products against DESIGN.md 5.17's bound (the example's
arithmetic and the GPU meaning test's inputs), the range test's inputs against the narrow conversion, and the entry points' refusals that need
no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import round_oracle as ro
import trgsw_mac_oracle as O
from kit import ROOT, load_example, random_words


@pytest.mark.parametrize("N", [1024, 2048])
def test_one_term_is_the_external_product(orc, N):
    """K = 1 without acc: round_oracle.external_product word for word in both modes, and in reference mode orc_external_product itself.  Rows
    with the decomposition's edge words; three bootstrapping-key entries of a small key set serve as selectors.  Then the sum: K = 2 differs
    from the wrapping sum of two products somewhere (one truncation, not two), and acc adds wrapping."""
    p = orc.Params(n=3, N=N)
    plan = orc.Plan(N)
    keys = orc.Keys(p, 0x3A + N, plan=plan)
    x = O.rows_with_edges(N + 3, N, 3)
    trgsw = 2 * 2 * p.l * N
    s_idx = [[2], [0], [2]]
    for mode in (O.REFERENCE, O.ROUNDED):
        ma, mx = ro.constants(p.l, p.bgbit, mode)
        got = O.mac(p, plan, keys.bk_f, s_idx, x, None, None, mode)
        for g in range(3):
            S = keys.bk_f[s_idx[g][0] * trgsw:(s_idx[g][0] + 1) * trgsw]
            assert np.array_equal(got[g].reshape(-1), ro.external_product(p, plan, S, x[g].reshape(-1), ma, mx)), (mode, g)
            if mode == O.REFERENCE:
                St = keys.bk_t[s_idx[g][0] * trgsw:(s_idx[g][0] + 1) * trgsw]
                assert np.array_equal(got[g].reshape(-1), orc.external_product(p, plan, S, St, x[g].reshape(-1))), g
        # NULL indices are g * K + k
        assert np.array_equal(O.mac(p, plan, keys.bk_f, None, x, None, None, mode), O.mac(p, plan, keys.bk_f, [[0], [1], [2]], x, [[0], [1], [2]], None, mode))
        two = O.mac(p, plan, keys.bk_f, [[2, 0]], x, [[0, 1]], None, mode)
        apart = got[0] + got[1]
        assert not np.array_equal(two[0], apart) and np.abs((two[0] - apart).view(np.int32)).max() <= 2
        acc = random_words(np.random.default_rng(N), (1, 2, N))
        assert np.array_equal(O.mac(p, plan, keys.bk_f, [[2, 0]], x, [[0, 1]], acc, mode), two + acc)
    assert not np.array_equal(O.mac(p, plan, keys.bk_f, s_idx, x, None, None, O.REFERENCE), O.mac(p, plan, keys.bk_f, s_idx, x, None, None, O.ROUNDED))


def test_edge_words_sit_on_digit_boundaries_of_both_modes():
    e = O.edge_words()
    assert {0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF} <= set(e.tolist())
    for mode in (O.REFERENCE, O.ROUNDED):
        ma, mx = ro.constants(3, 6, mode)
        d = ro.digits(e, 3, 6, ma, mx).astype(np.int64)
        assert d.min() == -32 and d.max() > 0                       # the most negative digit, and digits of both signs
        # somewhere among the planted words two neighbours (x, x + 1) fall into different last digits: a boundary of this mode
        ee = e.astype(np.int64)
        pairs = [(a, a + 1) for a in ee if a + 1 in set(ee.tolist())]
        dd = {int(v): ro.digits(np.array([v], np.uint32), 3, 6, ma, mx)[:, 0].tolist() for a in pairs for v in a}
        assert any(dd[int(a)] != dd[int(b)] for a, b in pairs), mode


@pytest.mark.parametrize("N", [1024, 2048])
def test_encrypt_trgsw_polys_of_a_constant_bit_is_encrypt_selectors(N):
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0x51 + N, want_bk=False, want_ksk=False)
    bits = np.array([1, 0, 1, 1, 0], np.uint8)
    mu = np.zeros((bits.size, N), np.int32)
    mu[:, 0] = bits
    got = R.encrypt_trgsw_polys(rp, key1, mu, seed=0x99)
    assert got.shape == (5, 2, 2 * rp.l, N) and got.dtype == np.uint32
    assert np.array_equal(got, R.encrypt_selectors(rp, key1, bits, seed=0x99))
    assert not np.array_equal(got, R.encrypt_trgsw_polys(rp, key1, mu, seed=0x9A))
    a, b = R.encrypt_trgsw_polys(rp, key1, mu), R.encrypt_trgsw_polys(rp, key1, mu)      # production: never repeatable
    assert not np.array_equal(a, b)
    L = R.load()
    out = np.empty_like(got)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((None, ptr(key1), ptr(mu), ptr(out)), (C.byref(rp), None, ptr(mu), ptr(out)), (C.byref(rp), ptr(key1), None, ptr(out)),
                 (C.byref(rp), ptr(key1), ptr(mu), None)):
        assert L.rtfhe_trgsw_encrypt_polys(args[0], args[1], args[2], args[3], 5) == R._ffi.ERR_INVALID
        assert L.rtfhe_trgsw_encrypt_polys_deterministic(args[0], args[1], 7, args[2], args[3], 5) == R._ffi.ERR_INVALID
    bad = key1.copy()
    bad[3] = 2
    assert L.rtfhe_trgsw_encrypt_polys_deterministic(C.byref(rp), ptr(bad), 7, ptr(mu), ptr(out), 5) == R._ffi.ERR_INVALID


@pytest.mark.parametrize("N", [1024, 2048])
def test_encrypt_trgsw_polys_phases(N):
    """Random mu with entries in {-1, 0, 1}: under key1 the phase of row j < l (the gadget on the b polynomial; comp 0 of the layout) is
    mu * g_j, that of row l + j (the gadget on the a polynomial) is -mu * s * g_j, negacyclic, both within 6 * 2^-25; g_j = 2^(32 - (j+1) bgbit)."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0x52 + N, want_bk=False, want_ksk=False)
    rng = np.random.default_rng(N)
    mu = rng.integers(-1, 2, (3, N)).astype(np.int32)
    ct = R.encrypt_trgsw_polys(rp, key1, mu, seed=0x77)
    l = rp.l
    worst = 0.0
    for e in range(3):
        rows = np.stack([np.stack([ct[e, 0, j], ct[e, 1, j]]) for j in range(2 * l)])      # [2l][2][N]: b then a of every row
        ph = R.trlwe_phase(rp, key1, rows)
        mus = O.negacyclic_i64(mu[e], key1).view(np.int32).astype(np.int64)                # mu * s, small integers
        for j in range(l):
            g = 1 << (32 - (j + 1) * rp.bgbit)
            want_b = ((mu[e].astype(np.int64) * g) & 0xFFFFFFFF).astype(np.uint32)
            want_a = ((-mus * g) & 0xFFFFFFFF).astype(np.uint32)
            worst = max(worst, np.abs(O.torus_err(ph[j], want_b)).max(), np.abs(O.torus_err(ph[l + j], want_a)).max())
    assert worst <= 6 * 2.0 ** -25, worst


def test_meaning_of_the_sum_on_the_cpu(orc, capsys):
    """Rounded mode, through the restatement.  (a) The inputs of the GPU meaning test (trgsw_mac_oracle.meaning_world): K = 4 encrypted ternary
    polynomials times four fresh rows per sample; every coefficient of the phase is sum_k mu_k * m_k within
    6 sqrt(sum_k [2lN 18.5^2 2^-50 + ||mu_k||^2 ((N/2 + 1) 2^-38 / 3 + N 2^-50)]).  (b) The arithmetic of examples/private_dense_layer.py: the
    weight polynomial TRGSW-encrypted, three clients, the bias through acc; the M read coefficients are the sums within the same bound, and
    the example's budget is the docstring's.  Measured here: (a) max 0.57 of the bound over 3,072 coefficients (rms 1.0 of the
    model's deviation); (b) max 0.74 of the bound over the 48 read coefficients -- over all 3,072 the error has rms 1.5 and a mean of 0.6 model
    deviations, with or without the selector rows' noise: a fresh row's mask words lie on the 2^-24 grid of the sampler, so the rounding error
    of the decomposition has a mean of +166 units of 2^-32, which the key's partial sums (up to N/2) and sum(mu) = 18 carry to 1.7 deviations at
    the ends of the row.  Random signs (a) cancel it; a layer whose weights have a common sign pays it."""
    import rustfhe_amd as R
    m = O.meaning_world(R)
    p = orc.Params(n=m.rp.n, N=m.rp.N)
    plan = orc.Plan(p.N)
    got = O.mac(p, plan, O.spectra(p, plan, m.sel_t), np.arange(m.COUNT * m.K).reshape(m.COUNT, m.K), m.rows, None, None, O.ROUNDED)
    ph = R.trlwe_phase(m.rp, m.key1, got)
    ratios = [float(np.abs(O.torus_err(ph[g], m.want[g])).max()) / m.bound[g] for g in range(m.COUNT)]
    lines = ["meaning world: bound %.2e, max error / bound per sample %s" % (m.bound[0], ["%.2f" % r for r in ratios])]

    ex = load_example("private_dense_layer")
    rp = R.Params(n=40, N=1024)
    _, key1, _, _ = R.keygen(rp, 0x3AD0, want_bk=False, want_ksk=False)
    rng = np.random.default_rng(0x3AD1)
    W, bias = ex.draw_layer(rng)
    clients = 3
    x = rng.integers(0, 2, (clients, ex.D))
    sums = x @ W.T + bias
    trgsw, coef = ex.owner_weights(rp, key1, W, seed=0x3AD2)
    rows = ex.client_rows(rp, key1, x, seed=0x3AD3)
    acc = np.repeat(R.dense_layer_bias(bias, ex.D, rp.N, ex.UNIT), clients, axis=0)
    out = O.mac(p, plan, O.spectra(p, plan, trgsw), np.zeros((clients, 1), np.int64), rows, None, acc, O.ROUNDED)
    ph = R.trlwe_phase(rp, key1, out)
    want = ((sums.astype(np.int64) * ex.UNIT) & 0xFFFFFFFF).astype(np.uint32)
    bound = O.noise_bound(rp.N, [float((W ** 2).sum())])
    ex_ratio = float(np.abs(O.torus_err(ph[:, coef], want)).max()) / bound
    assert np.array_equal(R.decode_msgs(ph[:, coef], ex.MSG_BITS), sums)
    lines.append("example: bound %.2e, max error / bound %.2f over %d coefficients" % (bound, ex_ratio, want.size))
    with capsys.disabled():
        print("\nTRLWE x TRGSW meaning on the CPU:\n  " + "\n  ".join(lines))
    assert max(ratios) <= 1.0 and ex_ratio <= 1.0, (ratios, ex_ratio)

    # the example's budget: the docstring's figures
    dp = R.Params()
    full = np.ones((ex.M, ex.POS + ex.NEG), np.int64)
    sigma, margin = ex.noise_budget(dp.n, dp.N, full)
    assert abs(ex.product_sigma(dp.N, 112.0) - 2.7e-4) < 1e-5 and abs(sigma - 3.4e-3) < 1e-4 and abs(margin - 8.6) < 0.1
    assert abs(6 * ex.product_sigma(dp.N, 112.0) - O.noise_bound(dp.N, [112.0])) < 1e-12
    for _ in range(10):
        Wd, _ = ex.draw_layer(rng)
        assert ex.noise_budget(dp.n, dp.N, Wd)[1] >= ex.DEVIATIONS
    # dense_layer_trgsw is encrypt_trgsw_polys of dense_layer_polys
    polys, coef2 = R.dense_layer_polys(W, ex.D, rp.N)
    assert np.array_equal(coef, coef2) and np.array_equal(trgsw, R.encrypt_trgsw_polys(rp, key1, polys, seed=0x3AD2))


@pytest.mark.parametrize("N", [1024, 2048])
def test_the_range_inputs_pass_the_narrow_conversion(orc, N):
    """The GPU range test's inputs through the restatement: every selector word 0x80000000, every digit of every row -Bg/2, K = 8.  The sums
    reach K * 2l * N * (Bg/2) * 2^31 = 2^51.58 / 2^52.58, below 2^53; and the magic-add conversion (trunc(x) + 1.5 * 2^52, low word of the
    mantissa: exact only below 2^51) gives other words than Torus32(int64(x)) on them -- else the GPU test would show nothing."""
    p = orc.Params(n=1, N=N)
    plan = orc.Plan(N)
    sel_t = np.full((1, 2, 2 * p.l, N), 0x80000000, np.uint32)
    sel_f = O.spectra(p, plan, sel_t)
    peak = O.K_MAX * 2 * p.l * N * 32 * 2.0 ** 31
    assert abs(np.log2(peak) - (51.585 if N == 1024 else 52.585)) < 1e-3 and peak < 2.0 ** 53
    for mode in (O.REFERENCE, O.ROUNDED):
        ma, mx = ro.constants(p.l, p.bgbit, mode)
        x = O.extreme_rows(N, 1, mode)
        assert (ro.digits(x[0, 0], p.l, p.bgbit, ma, mx) == -32).all()
        sums = []
        got = O.mac(p, plan, sel_f, np.zeros((1, O.K_MAX), np.int64), x, np.zeros((1, O.K_MAX), np.int64), None, mode, sums=sums)
        differ = 0
        for g, c, s in sums:
            t = plan.fft_f64(s)                                       # the inverse-transformed sums before truncation
            assert 0.9 * peak < np.abs(t).max() < 1.1 * peak
            wide = (np.trunc(t).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
            assert np.array_equal(wide, got[g, c])
            narrow = ((np.trunc(t) + 6755399441055744.0).view(np.int64) & 0xFFFFFFFF).astype(np.uint32)
            differ += int(np.sum(narrow != wide))
        assert differ > 0, mode


def test_entry_points_refuse_null_handles_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    buf = np.zeros(4, np.uint32).ctypes.data_as(C.c_void_p)
    assert L.rtfhe_trlwe_mul_trgsw_batch(None, None, None, buf, 1, None, 1, 0, buf, 1) == R._ffi.ERR_INVALID
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trlwe_mul_trgsw_batch_dev(None, None, None, buf, 1, None, 1, 0, buf, 1, None) == R._ffi.ERR_INVALID
    hdr = open(os.path.join(ROOT, "rustfhe_amd", "csrc", "rtfhe_trgsw_mac_plan.h")).read()
    assert "#define RTFHE_TRGSW_MAC_K_MAX %d" % O.K_MAX in hdr
