"""CPU: the rounded gadget decomposition of the leveled entry points (include/rtfhe.h: rtfhe_set_leveled_decomposition) without a GPU -- the
restated tree, rotation and netlist (tests/leveled_round_oracle.py, which tests/test_gpu_leveled_round.py compares the device's words with)
against the oracle's own three, the noise the rounded mode buys for 6-bit rows through a depth-8 tree and a 10-step rotation, the seeds of
the GPU meaning tests, and the entry points' argument checks."""
import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
import leveled_round_oracle as lo
from kit import random_words
from leveled_oracle import as_trlwe, oracle_cmux_net, oracle_cmux_tree, oracle_trgsw_rotate, rotate_clear, three_of_five
from pbs_oracle import bk_fft


@pytest.mark.parametrize("N", [1024, 2048])
def test_reference_constants_give_the_oracles_tree_rotation_and_net(orc, N):
    """MA = MX = make_decomp_mask: the restatements are oracle_cmux_tree, oracle_trgsw_rotate and oracle_cmux_net word for word -- depth 2 and
    3, plain and TRLWE rows of random words, the TRLWE and the extract forms; five bootstrapping-key entries of a small key set serve as
    selectors.  With the rounded constants every one of them is another function."""
    import rustfhe_amd as R
    p = orc.Params(n=5, N=N)
    plan = orc.Plan(N)
    keys = orc.Keys(p, 0x17 + N, plan=plan)
    rng = np.random.default_rng(N + 17)
    tables = {"plain": as_trlwe(random_words(rng, (8, N)), N), "encrypted": random_words(rng, (8, 2, N))}
    for depth in (2, 3):
        sel_idx = [int(k) for k in rng.integers(0, p.n, depth)]
        rot = [int(r) for r in rng.integers(0, 2 * N, depth)]
        for kind, table in tables.items():
            rows = table[:1 << depth]
            for coef in (None, int(rng.integers(0, N))):
                want = oracle_cmux_tree(orc, p, plan, keys.bk_f, sel_idx, rows, coef, keys.ksk)
                assert np.array_equal(lo.cmux_tree(p, plan, keys.bk_f, sel_idx, rows, coef, keys.ksk, lo.REFERENCE), want), (depth, kind, coef)
                assert not np.array_equal(lo.cmux_tree(p, plan, keys.bk_f, sel_idx, rows, coef, keys.ksk, lo.ROUNDED), want), (depth, kind, coef)
            for r in (rot, None):
                for extract in (False, True):
                    want = oracle_trgsw_rotate(orc, p, plan, keys.bk_f, sel_idx, r, rows[1], extract, keys.ksk)
                    assert np.array_equal(lo.trgsw_rotate(p, plan, keys.bk_f, sel_idx, r, rows[1], extract, keys.ksk, lo.REFERENCE), want), (depth, kind, extract)
                    assert not np.array_equal(lo.trgsw_rotate(p, plan, keys.bk_f, sel_idx, r, rows[1], extract, keys.ksk, lo.ROUNDED), want)
    # the netlist: the reduced diagram of three_of_five (TRLWE outputs), and a small one with rotations, a shared node and coefficients
    bdd = R.bdd_netlist(5, three_of_five)
    mixed = R.CmuxNetlist(3)
    a = mixed.node(0, mixed.row(1), mixed.row(0), rot=-3)
    b = mixed.node(1, a, mixed.row(2))
    c = mixed.node(2, b, a, rot=N + 5)
    mixed.output(c, coef=N - 1)
    mixed.output(a, coef=0)
    for net, idx in ((bdd, [3, 0, 4, 1, 2]), (mixed, [4, 4, 1])):
        for kind, table in tables.items():
            want = oracle_cmux_net(orc, p, plan, keys.bk_f, idx, table, net, keys.ksk)
            assert np.array_equal(lo.cmux_net(p, plan, keys.bk_f, idx, table, net, keys.ksk, lo.REFERENCE), want), (net.n_nodes, kind)
            assert not np.array_equal(lo.cmux_net(p, plan, keys.bk_f, idx, table, net, keys.ksk, lo.ROUNDED), want), (net.n_nodes, kind)


def test_noise_bound_figures():
    assert abs(lo.noise_bound(8, 1024) - 1.41e-4) < 1e-6 and abs(lo.noise_bound(8, 2048) - 2.0e-4) < 1e-6


# margins of the absolute bound: the restatement on this file's seeds gave rms 0.90 .. 1.31 r and max 3.0 .. 4.3 r over all rounded-mode
# cases below (both N, both kinds, every address).  r models the selector noise and the rounding error only (not the transforms' rounding
# nor the spread of the key's weight), and the largest of N Gaussian samples lies near 3.5 .. 4.3 standard deviations: rms is held to
# 1.5 r (15 % over the largest measured), max to 6 r (4.6 standard deviations at the largest measured rms, 40 % over the largest measured).
RMS_BOUND, MAX_BOUND = 1.5, 6.0


@pytest.mark.parametrize("N", [1024, 2048])
def test_rounded_mode_carries_6bit_rows_through_a_depth8_tree_and_a_10_step_rotation(orc, N, capsys):
    """Keys from the product's keygen (n = 8), selectors from encrypt_selectors, 256 rows of N random 6-bit messages, plain and encrypt_lut's.
    The depth-8 tree at addresses 255 (all ones), 0 and 0xA5, and the 10-step rotation with the default rot at 1023, 0 and 0x2B5, in both
    modes on the same inputs.  Rounded mode: every coefficient decodes at every address; rms < 1.5 r and max < 6 r with r = noise_bound; at
    the all-ones address its largest distance is below 0.5 x reference mode's (measured 0.04 .. 0.10), and reference mode fails the decode
    there (measured at N = 1024: 509 / 529 of 1,024 wrong in the tree, plain / encrypted; 417 / 465 in the rotation).  At address 0 no ratio is
    asserted: the systematic term appears only under selector bits that are 1, and the two modes are equal there (measured ratio 0.8 .. 1.3)."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0x6B17 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    msgs, plain, rows = lo.meaning_setup(R, rp, key1, 256, 0x17 + N)
    lines = []

    def check(what, depth, addr, ones, want, run):
        for kind in ("plain", "encrypted"):
            worst = {}
            for mode in (lo.REFERENCE, lo.ROUNDED):
                ph = R.trlwe_phase(rp, key1, run(kind, mode)[None])[0]
                err = lo.torus_err(ph, want)
                r = lo.noise_bound(depth, N)
                rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
                wrong = int(np.sum(R.decode_msgs(ph, lo.MSG_BITS) != R.decode_msgs(want, lo.MSG_BITS)))
                lines.append("%s, %s, address %d, %s: max %.2e (%.2f r) rms %.2e (%.2f r), %d of %d wrong"
                             % (what, kind, addr, "rounded" if mode == lo.ROUNDED else "reference", mx, mx / r, rms, rms / r, wrong, N))
                worst[mode] = mx
                if mode == lo.ROUNDED:
                    assert wrong == 0, (what, kind, addr)
                    assert rms < RMS_BOUND * r and mx < MAX_BOUND * r, (what, kind, addr, rms / r, mx / r)
                elif ones:
                    assert wrong > 0, "the reference decomposition is expected to lose 6-bit coefficients at the all-ones address"
            if ones:
                assert worst[lo.ROUNDED] < 0.5 * worst[lo.REFERENCE], (what, kind, worst)

    try:
        for addr in (255, 0, 0xA5):
            sel_f = bk_fft(orc, p, plan, lo.address_selectors(R, rp, key1, 8, addr, 0x5E1).reshape(-1))
            check("tree depth 8", 8, addr, addr == 255, plain[addr], lambda kind, mode: lo.cmux_tree(p, plan, sel_f, range(8), rows[kind], mode=mode))
        for addr in (1023, 0, 0x2B5):
            sel_f = bk_fft(orc, p, plan, lo.address_selectors(R, rp, key1, 10, addr, 0x5E2).reshape(-1))
            check("rotation, 10 steps", 10, addr, addr == 1023, rotate_clear(plain[3], addr),
                  lambda kind, mode: lo.trgsw_rotate(p, plan, sel_f, range(10), None, rows[kind][3], mode=mode))
    finally:
        with capsys.disabled():
            print("\nleveled decomposition modes, N = %d, r(8) = %.2e, r(10) = %.2e:\n  %s" % (N, lo.noise_bound(8, N), lo.noise_bound(10, N), "\n  ".join(lines)))


def test_seeds_of_the_gpu_meaning_tests(orc, capsys):
    """The setup of tests/test_gpu_leveled_round.py's meaning tests (leveled_round_oracle.gpu_meaning_world: n = 40, N = 1024) through the restatement: at the
    all-ones addresses the reference mode decodes wrong and the rounded mode right, for plain and encrypted rows -- else those tests would
    show nothing."""
    import rustfhe_amd as R
    m = lo.gpu_meaning_world(R)
    p = orc.Params(n=m.rp.n, N=m.rp.N)
    plan = orc.Plan(p.N)
    lines = []
    for kind in ("plain", "encrypted"):
        sel_f = bk_fft(orc, p, plan, m.tree_sel[255].reshape(-1))
        rot_f = bk_fft(orc, p, plan, m.rot_sel[1023].reshape(-1))
        for mode in (lo.REFERENCE, lo.ROUNDED):
            tree = R.trlwe_phase(m.rp, m.key1, lo.cmux_tree(p, plan, sel_f, range(8), m.rows[kind], mode=mode)[None])[0]
            rotn = R.trlwe_phase(m.rp, m.key1, lo.trgsw_rotate(p, plan, rot_f, range(10), None, m.rows[kind][m.ROT_ROW], mode=mode)[None])[0]
            wrong = (int(np.sum(R.decode_msgs(tree, lo.MSG_BITS) != m.msgs[255])),
                     int(np.sum(R.decode_msgs(rotn, lo.MSG_BITS) != R.decode_msgs(rotate_clear(m.plain[m.ROT_ROW], 1023), lo.MSG_BITS))))
            lines.append("%s rows, %s: tree address 255 %d wrong, rotation address 1023 %d wrong" % (kind, "rounded" if mode else "reference", *wrong))
            assert wrong == (0, 0) if mode == lo.ROUNDED else min(wrong) > 0, (kind, mode, wrong)
    with capsys.disabled():
        print("\nseeds of the GPU meaning tests on the CPU:\n  " + "\n  ".join(lines))


def test_leveled_decomposition_entries_reject_null_handles_and_bad_modes_without_a_gpu():
    import rustfhe_amd as R
    L = R.load()
    for mode in (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED, 2, -1, 1 << 20):
        assert L.rtfhe_set_leveled_decomposition(None, mode) == R._ffi.ERR_INVALID
        assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_get_leveled_decomposition(None) == R._ffi.ERR_INVALID
