"""CPU: the TRLWE key switch (include/rtfhe.h: rtfhe_trlwe_ksk_keygen, rtfhe_trlwe_automorphism, rtfhe_trlwe_auto_batch) without a device --
the automorphism's algebra, the restatement the GPU tests compare every word to (tests/auto_oracle.py) against the oracle's own external
product on the padded TRGSW, the switching key against its phases and its refusals, the meaning of one step, of a chain and of a partial trace
against DESIGN.md 5.25's bounds, and the entry points' refusals that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import auto_oracle as A
import round_oracle as ro
import trgsw_mac_oracle as O
from kit import ROOT, random_words, torus_err


@pytest.mark.parametrize("N", [16, 1024, 2048])
def test_automorphism_algebra(N):
    """sigma_t o sigma_u = sigma_(tu mod 2N); sigma_1 is the identity; sigma_(2N-1) reverses with the known signs (coefficient 0 stays, j goes
    to N - j negated); sigma_t is multiplicative on small integer polynomials under the negacyclic product; the library's CPU form equals
    the numpy form."""
    import rustfhe_amd as R
    rng = np.random.default_rng(N)
    x = random_words(rng, (3, N))
    assert np.array_equal(A.automorphism(x, 1), x)
    rev = A.automorphism(x, 2 * N - 1)
    assert np.array_equal(rev[:, 0], x[:, 0]) and np.array_equal(rev[:, 1:], (0 - x[:, :0:-1].astype(np.int64)).astype(np.uint32))
    ts = [1, 3, 5, N // 2 + 1, N + 1, 2 * N - 1, 2 * N - 3]
    for t in ts:
        assert np.array_equal(R.trlwe_automorphism(x, t), A.automorphism(x, t)), t
        assert np.array_equal(A.automorphism(A.automorphism(x, t), A.inverse_exponent(N, t)), x), t
        assert R.load().rtfhe_trlwe_auto_inverse(N, t) == A.inverse_exponent(N, t), t
        for u in ts:
            assert np.array_equal(A.automorphism(A.automorphism(x, u), t), A.automorphism(x, t * u % (2 * N))), (t, u)
    p, q = rng.integers(-3, 4, N), rng.integers(-3, 4, N)
    for t in (3, N + 1, 2 * N - 1):
        sp = A.automorphism((p & 0xFFFFFFFF).astype(np.uint32), t).view(np.int32)
        sq = A.automorphism((q & 0xFFFFFFFF).astype(np.uint32), t).view(np.int32)
        assert np.array_equal(O.negacyclic_i64(sp, sq), A.automorphism(O.negacyclic_i64(p, q), t)), t
    # in place, and the refusals
    y = x.copy()
    L = R.load()
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.rtfhe_trlwe_automorphism(N, 3, ptr(y), ptr(y), 3) == 0 and np.array_equal(y, A.automorphism(x, 3))
    for bad_N, bad_t in ((N, 2), (N, 0), (N, 2 * N + 1), (N, -1), (N + 1, 3), (0, 1)):
        assert L.rtfhe_trlwe_automorphism(bad_N, bad_t, ptr(x), ptr(y), 1) == R._ffi.ERR_INVALID, (bad_N, bad_t)
    assert L.rtfhe_trlwe_automorphism(N, 3, None, ptr(y), 1) == R._ffi.ERR_INVALID
    assert L.rtfhe_trlwe_automorphism(N, 3, ptr(x), None, 1) == R._ffi.ERR_INVALID
    with pytest.raises(R.RtfheError):
        R.trlwe_automorphism(x, 4)
    assert R.trace_exponents(N, 3) == [N + 1, N // 2 + 1, N // 4 + 1]
    # the partial trace on plain polynomials: every 2^steps-th coefficient, times 2^steps
    z = x[0].copy()
    for t in R.trace_exponents(N, 3):
        z = z + A.automorphism(z, t)
    want = np.zeros(N, np.uint32)
    want[::8] = x[0, ::8] * np.uint32(8)
    assert np.array_equal(z, want)


@pytest.mark.parametrize("N", [1024, 2048])
def test_a_step_is_the_external_product_on_the_padded_trgsw(orc, N):
    """step == (sigma_t b, 0) + round_oracle.external_product(T, (sigma_t a, 0)), word for word, both modes, on rows with the decomposition's
    edge words and a key of random words; add mode adds wrapping; the two modes differ."""
    p = orc.Params(n=3, N=N)
    plan = orc.Plan(N)
    rng = np.random.default_rng(0xA0 + N)
    t_list = [1, 3, N // 2 + 1, N + 1, 2 * N - 1]
    key = random_words(rng, (len(t_list), p.l, 2, N))
    key_f = A.spectra(p, plan, key)
    x = O.rows_with_edges(N + 5, N, len(t_list))
    got = {}
    for mode in (A.REFERENCE, A.ROUNDED):
        ma, mx = ro.constants(p.l, p.bgbit, mode)
        assert (ro.digits(np.zeros(4, np.uint32), p.l, p.bgbit, ma, mx) == 0).all()      # the word 0 has the digits 0: the a = 0 half adds nothing
        for e, t in enumerate(t_list):
            T_f = O.spectra(p, plan, A.padded_trgsw(p, key, e)[None])
            inp = np.concatenate([A.automorphism(x[e, 1], t), np.zeros(N, np.uint32)])
            want = ro.external_product(p, plan, T_f, inp, ma, mx).reshape(2, N)
            want[0] = want[0] + A.automorphism(x[e, 0], t)
            got[mode, e] = A.step(p, plan, key_f, e, t, x[e], False, mode)
            assert np.array_equal(got[mode, e], want), (mode, t)
            assert np.array_equal(A.step(p, plan, key_f, e, t, x[e], True, mode), want + x[e]), (mode, t)
        both = A.program(p, plan, key_f, t_list, x[:2], [1, 0, 1], [0, 1, 0], mode)
        for g in range(2):
            y = A.step(p, plan, key_f, 1, 3, x[g], False, mode)
            y = A.step(p, plan, key_f, 0, 1, y, True, mode)
            assert np.array_equal(both[g], A.step(p, plan, key_f, 1, 3, y, False, mode))
    assert any(not np.array_equal(got[A.REFERENCE, e], got[A.ROUNDED, e]) for e in range(len(t_list)))


@pytest.mark.parametrize("N", [1024, 2048])
def test_switching_key_phases_and_refusals(N):
    """Under key_to the phase of row (e, j) is -sigma_t(key_from) * g_j within 6 * 2^-25, g_j = 2^(32 - (j+1) bgbit); the deterministic form
    is repeatable, the production form is not; every refusal of the key generator."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, kf, _, _ = R.keygen(rp, 0x61 + N, want_bk=False, want_ksk=False)
    _, kt, _, _ = R.keygen(rp, 0x62 + N, want_bk=False, want_ksk=False)
    t = [1, 3, 5, N // 2 + 1, N + 1, 2 * N - 1]
    for key_to in (kt, kf):
        K = R.trlwe_ksk_keygen(rp, kf, key_to, t, seed=0x77)
        assert K.shape == (len(t), rp.l, 2, N) and K.dtype == np.uint32
        ph = R.trlwe_phase(rp, key_to, K.reshape(-1, 2, N)).reshape(len(t), rp.l, N)
        worst = 0.0
        for e, te in enumerate(t):
            s = A.automorphism(kf.astype(np.uint32), te).view(np.int32).astype(np.int64)
            for j in range(rp.l):
                want = ((-s * (1 << (32 - (j + 1) * rp.bgbit))) & 0xFFFFFFFF).astype(np.uint32)
                worst = max(worst, float(np.abs(torus_err(ph[e, j], want)).max()))
        assert 0 < worst <= 6 * 2.0 ** -25, worst
    assert np.array_equal(K, R.trlwe_ksk_keygen(rp, kf, kf, t, seed=0x77))
    assert not np.array_equal(K, R.trlwe_ksk_keygen(rp, kf, kf, t, seed=0x78))
    # an entry's rows do not depend on its neighbours' exponents being there ... but on its position (one generator per entry)
    assert np.array_equal(K[:2], R.trlwe_ksk_keygen(rp, kf, kf, t[:2], seed=0x77))
    a, b = R.trlwe_ksk_keygen(rp, kf, kt, [1]), R.trlwe_ksk_keygen(rp, kf, kt, [1])      # production: never repeatable
    assert not np.array_equal(a, b)

    L = R.load()
    ptr = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full((64, rp.l, 2, N), 0x5A5A5A5A, np.uint32)

    def both(params, f, to, tt, n_t, dst):
        tt = None if tt is None else np.array(tt, np.int32)
        r1 = L.rtfhe_trlwe_ksk_keygen(params, ptr(f), ptr(to), ptr(tt), n_t, ptr(dst))
        r2 = L.rtfhe_trlwe_ksk_keygen_deterministic(params, ptr(f), ptr(to), 7, ptr(tt), n_t, ptr(dst))
        assert r1 == r2
        return r1

    ok = list(range(1, 129, 2))
    assert both(C.byref(rp), kf, kt, ok, 64, out) == 0                                   # the limits, accepted exactly: 64 exponents, t = 1
    assert both(C.byref(rp), kf, kt, [2 * N - 1], 1, out) == 0                           # ... and t = 2N - 1
    out[:] = 0x5A5A5A5A
    bad_key = kf.copy()
    bad_key[5] = 2
    for args in ((None, kf, kt, [1], 1, out), (C.byref(rp), None, kt, [1], 1, out), (C.byref(rp), kf, None, [1], 1, out), (C.byref(rp), kf, kt, None, 1, out),
                 (C.byref(rp), kf, kt, [1], 1, None), (C.byref(rp), kf, kt, [1], 0, out), (C.byref(rp), kf, kt, ok + [129], 65, out),
                 (C.byref(rp), kf, kt, [2], 1, out), (C.byref(rp), kf, kt, [0], 1, out), (C.byref(rp), kf, kt, [-1], 1, out), (C.byref(rp), kf, kt, [2 * N + 1], 1, out),
                 (C.byref(rp), kf, kt, [3, 5, 3], 3, out), (C.byref(rp), bad_key, kt, [1], 1, out), (C.byref(rp), kf, bad_key, [1], 1, out)):
        assert both(*args) == R._ffi.ERR_INVALID, args[3:5]
    assert (out == 0x5A5A5A5A).all()                                                     # a refusal draws nothing
    with pytest.raises(R.RtfheError):
        R.trlwe_ksk_keygen(rp, kf, kt, [3, 3])


def test_meaning_of_steps_chains_and_the_partial_trace_on_the_cpu(orc, capsys):
    """Rounded mode, through the restatement, N = 1024, fresh rows of 3-bit messages (auto_oracle.meaning_world).
    (a) One replace step gives sigma_t(phase) on every coefficient within 6 sqrt(l N 18.5^2 2^-50 + (hw(key_from) + 1) 2^-38 / 3 + N 2^-50),
        for t = 1 with a change of key (A -> B) and for t = 3, N + 1, 2N - 1 under B.
    (b) A chain of m = 4 replace steps (3, N + 1, 2N - 1, 3) is held to sqrt(m) times that.
    (c) The 4-step partial trace (add steps N + 1, N/2 + 1, N/4 + 1, N/8 + 1) is held to 6 sqrt(V_4), V_m = 4 V_(m-1) + v, V_0 = 2^-50:
        exactly the coefficients = 0 mod 16 carry 16 x the message, the others decrypt to 0.  The traced rows hold the messages 16 times
        smaller (m 2^24), so that 16 x a surviving word is the 3-bit encoding m 2^28, not 0 mod 2^32: the survivors decode to the messages
        (auto_oracle.check_trace).
    Nothing is asserted for the full 10-step trace (sigma ~ 0.023 on coefficient 0).
    Measured here (max error / bound over 2 rows = 2,048 coefficients): (a) 0.83 (t = 1, re-key), 0.66 (3), 0.67 (N + 1), 0.62 (2N - 1);
    (b) 0.73; (c) 0.49.  (A fresh row's mask words lie on the sampler's 2^-24 grid, so the rounding error of the decomposition is not
    zero-mean and the key's partial sums carry it: the re-key, whose a' is the fresh mask itself, sits highest -- tests/test_trgsw_mac_host.py
    measured the same effect.)"""
    import rustfhe_amd as R
    m = A.meaning_world(R)
    p = orc.Params(n=m.rp.n, N=m.rp.N)
    N = p.N
    plan = orc.Plan(N)
    kr_f, ka_f = A.spectra(p, plan, m.k_rekey), A.spectra(p, plan, m.k_auto)
    lines, ratios = [], []

    def check(name, got, key, want, bound):
        ph = R.trlwe_phase(m.rp, key, got)
        r = float(np.abs(torus_err(ph, want)).max()) / bound
        lines.append("%-28s bound %.2e, max error / bound %.2f over %d coefficients" % (name, bound, r, want.size))
        ratios.append(r)
        return ph

    # (a)
    got = A.program(p, plan, kr_f, m.t_rekey, m.rowsA, [0], None, A.ROUNDED)
    ph = check("re-key A -> B (t = 1)", got, m.keyB, m.plain, A.step_bound(N, m.hwA))
    assert np.array_equal(R.decode_msgs(ph, m.MSG_BITS), m.msgs)
    under_A = R.decode_msgs(R.trlwe_phase(m.rp, m.keyA, got), m.MSG_BITS)
    assert np.mean(under_A == m.msgs) < 0.5                                              # nothing decodes under the old key
    for e, t in enumerate(m.t_auto[:3]):
        got = A.program(p, plan, ka_f, m.t_auto, m.rowsB, [e], None, A.ROUNDED)
        check("sigma_%d" % t, got, m.keyB, A.automorphism(m.plain, t), A.step_bound(N, m.hwB))
    # (b)
    chain = [0, 1, 2, 0]
    want = m.plain
    for e in chain:
        want = A.automorphism(want, m.t_auto[e])
    got = A.program(p, plan, ka_f, m.t_auto, m.rowsB, chain, None, A.ROUNDED)
    check("chain of %d replace steps" % len(chain), got, m.keyB, want, A.step_bound(N, m.hwB, len(chain)))
    # (c)
    assert [m.t_auto[e] for e in m.trace_entries] == R.trace_exponents(N, 4)
    got = A.program(p, plan, ka_f, m.t_auto, m.rows_trace, m.trace_entries, [1, 1, 1, 1], A.ROUNDED)
    check("4-step partial trace", got, m.keyB, m.trace_want, A.trace_bound(N, m.hwB, 4))
    A.check_trace(R, m, got, A.trace_bound(N, m.hwB, 4))      # ... and the survivors decode to the messages, the others to 0
    with capsys.disabled():
        print("\nTRLWE key switch meaning on the CPU:\n  " + "\n  ".join(lines))
    assert max(ratios) <= 1.0, ratios


def test_entry_points_refuse_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    buf = np.zeros(4, np.uint32).ctypes.data_as(C.c_void_p)
    ent = np.zeros(1, np.int32).ctypes.data_as(C.c_void_p)
    assert L.rtfhe_trlwe_auto_batch(None, None, ent, None, 1, buf, buf, 1) == R._ffi.ERR_INVALID
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_trlwe_auto_batch_dev(None, None, ent, None, 1, buf, buf, 1, None) == R._ffi.ERR_INVALID
    h = C.c_void_p()
    assert L.rtfhe_trlwe_ksk_create(None, buf, ent, 1, C.byref(h)) == R._ffi.ERR_INVALID and not h
    L.rtfhe_trlwe_ksk_destroy(None)
    hdr = open(os.path.join(ROOT, "rustfhe_amd", "csrc", "rtfhe_trlwe_auto_plan.h")).read()
    assert "#define RTFHE_TRLWE_AUTO_MAX_STEPS %d" % A.MAX_STEPS in hdr and "#define RTFHE_TRLWE_AUTO_MAX_EXPONENTS %d" % A.MAX_EXPONENTS in hdr
    assert "rtfhe_trlwe_auto_plan.cpp" in open(os.path.join(ROOT, "rustfhe_amd", "build.py")).read()
