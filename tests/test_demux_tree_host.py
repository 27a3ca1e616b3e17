"""CPU: the CMUX demultiplexer tree (include/rtfhe.h, rtfhe_demux_tree_batch) without a GPU -- the demultiplexer restated with the oracle's
own building blocks (tests/leveled_oracle.py: oracle_demux_tree, which tests/test_gpu_demux_tree.py compares the device's words with), what it means with keys and
selectors the product generated, that it is the inverse of the CMUX tree, and the entry points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import orc as _orc_mod  # noqa: F401  (conftest puts tests/ on the path)
import round_oracle as ro
from kit import torus_dist
from leveled_oracle import as_trlwe, oracle_cmux_tree, oracle_demux_tree
from pbs_oracle import bk_fft

@pytest.mark.parametrize("N", [1024, 2048])
def test_oracle_demux_writes_the_addressed_leaf(orc, N, capsys):
    """Keys from the product's keygen, selectors from encrypt_selectors: for every address of a depth-2 and of a depth-3 demultiplexer of a row
    of N random 2-bit messages -- the trivial (tv, 0) and a TRLWE encryption of it -- the addressed leaf's phase decodes to the row at every
    coefficient and every other leaf's to 0, and all stay within depth * 2e-3 * N / 1024 of that: the reference's own per-product bound
    (hom_nand/src/trgsw.rs:365-393) as tests/test_cmux_tree_host.py scales it, summed over the depth products every leaf has passed.  Then the
    inverse property: oracle_cmux_tree over the leaves with the same selectors decodes to the row again."""
    import rustfhe_amd as R
    rp = R.Params(n=8, N=N)
    key0, key1, _, _ = R.keygen(rp, 0xD3 + N, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    rng = np.random.default_rng(N + 5)
    worst = {}
    for depth in (2, 3):
        msgs = rng.integers(0, 4, N)
        plain = R.encode_msgs(msgs, 2)
        zero = R.encode_msgs(np.zeros(N, np.int64), 2)
        for kind, x in (("trivial", as_trlwe(plain, N)[0]), ("encrypted", R.encrypt_lut(rp, key1, plain, seed=0xE5 + depth)[0])):
            for addr in range(1 << depth):
                bits = [(addr >> k) & 1 for k in range(depth)]
                sel = R.encrypt_selectors(rp, key1, bits, seed=0x5E7 + 16 * depth + addr)
                sel_f = bk_fft(orc, p, plan, sel.reshape(-1))
                leaves = oracle_demux_tree(orc, p, plan, sel_f, range(depth), x)
                assert leaves.shape == (1 << depth, 2, N)
                ph = R.trlwe_phase(rp, key1, leaves)
                want = np.zeros((1 << depth, N), np.int64)
                want[addr] = msgs
                assert np.array_equal(R.decode_msgs(ph, 2), want), (depth, kind, addr)
                target = np.tile(zero, (1 << depth, 1))
                target[addr] = plain
                worst[depth, kind] = max(worst.get((depth, kind), 0.0), float(torus_dist(ph, target).max()))
                back = oracle_cmux_tree(orc, p, plan, sel_f, range(depth), leaves)
                assert np.array_equal(R.decode_msgs(R.trlwe_phase(rp, key1, back[None])[0], 2), msgs), (depth, kind, addr, "inverse")
    with capsys.disabled():
        print("\noracle CMUX demultiplexer, N = %d: largest torus distance of a leaf from its message %s" % (N, {k: round(v, 5) for k, v in worst.items()}))
    for (depth, kind), w in worst.items():
        assert w < depth * 2e-3 * N / 1024, (depth, kind, w)


def test_rounded_restatement_with_reference_constants_is_the_oracles(orc):
    """oracle_demux_tree's two branches agree where they must: round_oracle.cmux with the reference constants is orc_cmux word for word, so
    forcing the restated product with (MA, MX) = the reference's gives the same leaves; the rounded constants give other words."""
    import rustfhe_amd as R
    N = 1024
    rp = R.Params(n=8, N=N)
    _, key1, _, _ = R.keygen(rp, 0xD9, want_bk=False, want_ksk=False)
    p = orc.Params(n=8, N=N)
    plan = orc.Plan(N)
    sel_f = bk_fft(orc, p, plan, R.encrypt_selectors(rp, key1, [1, 0], seed=3).reshape(-1))
    x = np.random.default_rng(7).integers(0, 1 << 32, (2, N), dtype=np.uint64).astype(np.uint32)
    ref = oracle_demux_tree(orc, p, plan, sel_f, [0, 1], x)
    ma, mx = ro.constants(p.l, p.bgbit, ro.REFERENCE)
    zeros = np.zeros(2 * N, np.uint32)
    trgsw = 2 * 2 * p.l * N
    hi = ro.cmux(p, plan, sel_f[trgsw:2 * trgsw], x.reshape(-1), zeros, ma, mx)             # level 0 splits on selector depth - 1 = 1
    assert np.array_equal(ref[2:].sum(axis=0, dtype=np.uint32).reshape(-1), hi)              # leaves 2 + 3 = the level-0 high child
    assert np.array_equal(ref.sum(axis=0, dtype=np.uint32), x)                               # the leaves always sum to x, word for word
    rounded = oracle_demux_tree(orc, p, plan, sel_f, [0, 1], x, mode=ro.ROUNDED)
    assert not np.array_equal(rounded, ref) and np.array_equal(rounded.sum(axis=0, dtype=np.uint32), x)


def test_demux_level_selector_is_the_trees_order_reversed():
    import rustfhe_amd as R
    for depth in (1, 2, 5, 16):
        order = [R.demux_level_selector(depth, t) for t in range(depth)]
        assert order == list(range(depth))[::-1]            # the tree's level k joins on selector k: the demultiplexer undoes the levels last to first


def test_entries_reject_null_handles_without_a_device():
    import rustfhe_amd as R
    L = R.load()
    p = R.Params(n=8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    INV = R._ffi.ERR_INVALID
    for name in ("rtfhe_demux_tree_batch", "rtfhe_demux_tree_batch_dev", "rtfhe_lut_accumulate_dev"):
        assert name in R._ffi.EXPORTED_SYMBOLS
    x = np.zeros((1, 2, p.N), np.uint32)
    out = np.zeros((1, 2, 2, p.N), np.uint32)
    # a null context (there is none without a GPU) is refused before anything else is looked at
    assert L.rtfhe_demux_tree_batch(None, None, None, 1, ptr(x), ptr(out), 1) == INV
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_demux_tree_batch_dev(None, None, None, 1, None, None, 1, None) == INV
    assert b"null context" in L.rtfhe_last_error(None)
    assert L.rtfhe_lut_accumulate_dev(None, None, 0, 1, 1, None) == INV
    assert b"null table" in L.rtfhe_last_error(None)
