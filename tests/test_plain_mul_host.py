"""CPU: the exact TRLWE x plain-polynomial product (include/rtfhe.h: rtfhe_trlwe_mul_plain_batch) without a device -- the numpy oracle the GPU
tests compare every word to against the definition in Python integers, the dense-layer layout against W @ x, the exactness domain against the
split-FFT backend's error model, and the parameter arithmetic of examples/encrypted_dense_layer.py."""
import os
import sys

import numpy as np
import pytest

import plain_mul_oracle as O
from kit import ROOT, load_example


@pytest.mark.parametrize("N", [16, 1024, 2048])
def test_oracle_equals_the_definition_in_python_integers(N):
    x = O.rows_with_edges(N, N, 2)
    at = [0, 1, N // 2 - 1, N // 2, N - 2, N - 1]
    for w in (O.weights(N + 1, N, 1, O.L1_PER_N * N)[0], O.extreme_weights(N, O.L1_PER_N)[3], np.eye(1, N, N - 1, dtype=np.int64)[0] * -5):
        for c in range(2):
            assert np.array_equal(O.negacyclic(w, x[0, c])[at], O.negacyclic_bigint(w, x[0, c], at))
    # the batch form: indices with duplicates, accumulation wrapping mod 2^32
    w = O.weights(N + 2, N, 3, 7 * N)
    w_idx, x_idx = [[0, 2], [2, 2], [1, 0]], [[0, 1], [1, 1], [0, 0]]
    acc = np.full((3, 2, N), 0xFFFFFFF0, np.uint32)
    got = O.mul_plain(w, x, 2, w_idx, x_idx, acc)
    for g in range(3):
        want = sum(int(v) for v in [0xFFFFFFF0]) + sum(int(O.negacyclic_bigint(w[w_idx[g][k]], x[x_idx[g][k], 1], [N - 1])[0]) for k in range(2))
        assert int(got[g, 1, N - 1]) == want & O.MASK
    assert np.array_equal(O.mul_plain(w, x, 2), (O.mul_plain(w[:1], x[:1]) + O.mul_plain(w[1:2], x[1:2])))      # w_idx NULL: entry k; x_idx NULL: row g K + k


def test_planted_edges_and_extreme_rows():
    for N in (1024, 2048):
        x = O.rows_with_edges(5, N, 3)
        for r in range(3):
            for c in range(2):
                assert set(O.EDGES.tolist()) <= set(x[r, c].tolist())
        # the aligned rows drive both halves' sums of the target coefficient to the domain's edge: |sum| = 192 N * 32767 or more, below 2^35
        w = O.extreme_weights(N, O.L1_PER_N)
        rows = O.aligned_rows(w, N)
        for e in range(4):
            for t, c in enumerate((0, N // 2, N - 1)):
                xs = rows[e * 3 + t].view(np.int32).astype(np.int64)
                lo = ((xs + 0x8000) & 0xFFFF) - 0x8000
                hi = (xs - lo) >> 16
                for half in (hi, lo):
                    for comp, sign in ((0, 1), (1, -1)):
                        full = np.convolve(w[e].astype(np.int64), half[comp])
                        s = int(full[c]) - (int(full[c + N]) if c + N < full.size else 0)
                        assert sign * s >= O.L1_PER_N * N * 32767 and abs(s) < 2 ** 35, (N, e, c, s)


@pytest.mark.parametrize("d", [1, 8, 1024])
def test_dense_layer_polys_equal_the_matrix_product(d):
    import rustfhe_amd as R
    N = 1024
    rng = np.random.default_rng(d)
    per = N // d
    for m in (1, per, per + 3 if per > 1 else 3):
        W = rng.integers(-8, 9, (m, d))
        x = rng.integers(-100, 100, d)
        polys, coef = R.dense_layer_polys(W, d, N)
        assert polys.dtype == np.int32 and polys.shape == (-(-m // per), N) and coef.tolist() == [r * d + d - 1 for r in range(min(m, per))]
        xin = R.dense_layer_input(x, d, N)
        assert np.array_equal(xin[:d].view(np.int32), x) and not xin[d:].any()
        want = (W @ x) & O.MASK
        for q in range(polys.shape[0]):
            prod = O.negacyclic(polys[q], xin)
            rows = min(per, m - q * per)
            assert np.array_equal(prod[coef[:rows]], want[q * per:q * per + rows]), (d, m, q)
    # the bias rows: trivial TRLWEs with the bias where the dot products arrive
    b = R.dense_layer_bias([3, -1, 2], 8, N, unit=1 << 28)
    assert b.shape == (1, 2, N) and not b[0, 1].any() and b[0, 0, [7, 15, 23]].tolist() == [3 << 28, (-(1 << 28)) & O.MASK, 2 << 28] and np.count_nonzero(b) == 3
    with pytest.raises(AssertionError):
        R.dense_layer_polys(np.zeros((2, 3), np.int64), 3, N)      # d must divide N


def test_the_domain_is_the_split_fft_backends_bound():
    """K * wmax <= 192 N is rows * N * digit_max = 6 * 32 * N of scripts/xfft/model.py: error_bound depends on its inputs only through that
    product and half_max, so the proven bound carries over with the roles of the operands reversed"""
    sys.path.insert(0, os.path.join(ROOT, "scripts", "xfft"))
    import model
    for N, log2_bound in ((1024, -8.25), (2048, -6.62)):
        proven = model.error_bound(N)
        assert model.error_bound(N, rows=1, digit_max=O.L1_PER_N) == proven
        assert proven < 2.0 ** -6 and abs(np.log2(proven) - log2_bound) < 0.01
        for K in range(1, O.K_MAX + 1):      # K terms of l1 norm wmax each: rows = K, digit_max = wmax / N
            assert model.error_bound(N, rows=K, digit_max=(O.L1_PER_N * N // K) / N) <= proven * (1 + 1e-12)
        # the half-product sums stay inside the magic constant's 2^35
        assert O.L1_PER_N * N * 2 ** 15 < 2 ** 35 and np.log2(O.L1_PER_N * N * 2.0 ** 15) < (32.6 if N == 1024 else 33.6)
    hdr = open(os.path.join(ROOT, "rustfhe_amd", "csrc", "rtfhe_plain_plan.h")).read()
    assert "#define RTFHE_PLAIN_L1_PER_N %d" % O.L1_PER_N in hdr and "#define RTFHE_PLAIN_K_MAX %d" % O.K_MAX in hdr


def test_example_parameter_arithmetic():
    import rustfhe_amd as R
    ex = load_example("encrypted_dense_layer")
    p = R.Params()
    assert int(R.encode_msgs([1], ex.MSG_BITS)[0]) == ex.UNIT == 1 << 28 and p.N % ex.D == 0 and ex.M <= p.N // ex.D
    rng = np.random.default_rng(11)
    worst = None
    for _ in range(20):
        W, bias = ex.draw_layer(rng)
        assert set(np.unique(W)) <= {-1, 0, 1} and ((W == 1).sum(axis=1) <= ex.POS).all() and ((W == -1).sum(axis=1) <= ex.NEG).all()
        # every binary input keeps every sum a 3-bit message with its padding bit clear
        lo, hi = bias - (W == -1).sum(axis=1), bias + (W == 1).sum(axis=1)
        assert lo.min() >= 0 and hi.max() <= 7
        polys, coef = R.dense_layer_polys(W, ex.D, p.N)
        assert np.abs(polys.astype(np.int64)).sum() <= O.L1_PER_N * p.N          # K = 1 is inside the exactness domain
        sigma, margin = ex.noise_budget(p.n, p.N, W)
        worst = margin if worst is None else min(worst, margin)
        assert margin >= ex.DEVIATIONS
    # the budget the docstring states: 3.4e-3 and 8.6 deviations; the product's share is invisible beside the key switch's; 4 bits would not stand
    full = np.ones((ex.M, ex.D), np.int64)
    full[:, ex.POS + ex.NEG:] = 0
    sigma, margin = ex.noise_budget(p.n, p.N, full)
    assert abs(sigma - 3.4e-3) < 1e-4 and abs(margin - 8.6) < 0.1 and abs(worst - 8.6) < 0.1
    assert np.sqrt((full ** 2).sum()) * ex.FRESH_SIGMA < 3.3e-7 and np.abs(full).sum() * ex.FRESH_MEAN < 2.7e-7
    assert (2.0 ** -6 - ex.KEY_SWITCH_MEAN) / sigma < ex.DEVIATIONS
    tv = R.lut_polynomial(lambda m: int(m >= 4), p.N, ex.MSG_BITS, out_bits=1)
    B = p.N >> ex.MSG_BITS
    assert [int(tv[m * B]) for m in range(8)] == [0] * 4 + [1 << 30] * 4
