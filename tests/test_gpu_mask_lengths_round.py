"""GPU: the rounded gadget decomposition (rtfhe_set_decomposition; the 32 k_pbs_round_* kernels, code objects of their own with their own register
allocation) at the edges of the TLWE dimension n: the mask lengths and engines of tests/mask_kit.py, where tests/test_gpu_pbs_round.py holds the
words at n = 24 only and tests/test_gpu_mask_lengths.py never leaves the reference mode.  What n changes in these kernels is what it changes
in their reference twins (the LDS carve by npad, the step count, the gates per CU of the time-sliced launch and of the N = 2048 whole rounds).

One test item is one batch size of gk.sizes (each reaches another launch shape of the default dispatch) at one (N, n).  The oracle is
tests/round_oracle.py on the first and the last gate and on the gates either side of every segment boundary the dispatch can make at that size
(mask_kit.boundary_picks: no random picks here).  n_out = 8 is compared with the oracle on the first and the last gate: round_oracle.blind_rotate
switches b and every a_i at 32 - nbit - 1 + log2(n_out) bits and scales back, so with n_out = 8 every rotation is a multiple of 8 and differs
from the n_out = 1 rotation for all but one word in eight.  Output 0 equals the n_out = 1 row only on the gates whose n + 1 rotations all agree
(_same_rotations: a few dozen gates of a batch at n = 1, none from n = 63 on); on those it is asserted too.
Every comparison is np.array_equal on uint32 words: there is no tolerance in this file."""
import numpy as np
import pytest

import gpu_kit as gk
import round_oracle as ro
from kit import random_words
from mask_kit import FORCED, FORCED_MASKS, MASKS, Mask, boundary_picks

pytestmark = pytest.mark.gpu

N_SIZES = {N: len(gk.sizes(N, 256)) for N in (1024, 2048)}      # how many batch sizes a ring has (the sizes themselves follow the device's CUs)


def _order(N):
    """small first, as mask_kit.ORDER"""
    return sorted(MASKS[N], key=lambda n: (n in (1, 2), n > 64, n))


@pytest.fixture(scope="module", params=_order(1024), ids=lambda n: "n%d" % n)
def mask1024(request, orc):
    m = Mask(orc, 1024, request.param)
    yield m
    m.e.close()


@pytest.fixture(scope="module", params=_order(2048), ids=lambda n: "n%d" % n)
def mask2048(request, orc):
    m = Mask(orc, 2048, request.param)
    yield m
    m.e.close()


def _same_rotations(P, ct, n_out):
    """the gates of ct whose n + 1 rotations under n_out outputs are those under one output (round_oracle.blind_rotate's bbar and abar, for every
    gate at once): there the two blind rotations are the same arithmetic and output 0 is the n_out = 1 row.  One gate in 64 at n = 1, one in
    512 at n = 2, none to speak of from n = 63 on."""
    lt = int(n_out).bit_length() - 1
    s0 = 32 - P.nbit - 1
    s = s0 + lt
    t = ct.astype(np.uint64)
    a1 = ((t[:, :-1] + (1 << (s0 - 1))) & ro.U32) >> s0
    a8 = (((t[:, :-1] + (1 << (s - 1))) & ro.U32) >> s) << lt
    b1, b8 = t[:, -1] >> s0, (t[:, -1] >> s) << lt
    return np.flatnonzero((a1 == a8).all(axis=1) & (b1 == b8))


def _rounded_words_at_one_batch_size(m, k):
    import rustfhe_amd as R
    orc, P, K, e = m.orc, m.P, m.K, m.e
    sizes = gk.sizes(m.N, m.C)
    assert len(sizes) == N_SIZES[m.N]
    G = sizes[k]
    rng = np.random.default_rng([m.N, m.n, k])
    tv = random_words(rng, (3, m.N))
    trl = random_words(rng, (3, 2, m.N))      # any words: an encrypted table is data to the kernel
    ct = random_words(rng, (G, m.n + 1))
    idx = rng.integers(0, 3, G).astype(np.int32)
    ends = sorted({0, G - 1})
    pick = boundary_picks(G, m.N, m.C)

    def want(rows, gates, n_out):
        return np.stack(gk.pmap(lambda g: ro.pbs_many(P, gk.oracle_plan(orc, m.N), K.bk_f, K.ksk, rows[idx[g]], ct[g], n_out), gates))
    try:
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        with e.lut(tv) as plain, e.lut_encrypted(trl) as enc:
            got = e.pbs_many_batch(plain, ct, 2, idx)
            assert got.shape == (G, 2, m.n + 1)
            assert np.array_equal(got[pick], want(tv, pick, 2)), ("plain, n_out 2", G)
            got = e.pbs_many_batch(enc, ct, 4, idx)
            assert np.array_equal(got[ends], want(trl, ends, 4)), ("encrypted, n_out 4", G)
            one = e.pbs_many_batch(plain, ct, 1, idx)
            assert np.array_equal(e.pbs_batch(plain, ct, idx), one[:, 0]), ("pbs_batch against n_out 1", G)
            got = e.pbs_many_batch(plain, ct, 8, idx)
            assert got.shape == (G, 8, m.n + 1)
            assert np.array_equal(got[ends], want(tv, ends, 8)), ("plain, n_out 8", G)
            same = _same_rotations(P, ct, 8)
            assert np.array_equal(got[same, 0], one[same, 0]), ("n_out 8, output 0 of the gates whose rotations are those of n_out 1", G)
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)


@pytest.mark.parametrize("k", range(N_SIZES[1024]))
def test_rounded_words_at_every_batch_size_n1024(mask1024, k):
    """pbs_many_batch(plain, 2) on the boundary gates, pbs_many_batch(encrypted, 4) and pbs_many_batch(plain, 8) on the first and the last
    gate against round_oracle; pbs_batch equals pbs_many_batch(n_out = 1) on the whole batch."""
    _rounded_words_at_one_batch_size(mask1024, k)


@pytest.mark.parametrize("k", range(N_SIZES[2048]))
def test_rounded_words_at_every_batch_size_n2048(mask2048, k):
    _rounded_words_at_one_batch_size(mask2048, k)


def _forced_shapes(m, monkeypatch):
    """One engine per forced shape, same keys, rounded mode: pbs_batch, pbs_many_batch(n_out = 4) and the encrypted table give the default
    engine's rounded words on whole batches of gk.forced_sizes (mask_kit.FORCED_MASKS only)."""
    import rustfhe_amd as R
    e = m.e
    if m.n not in FORCED_MASKS[m.N]:
        return
    rng = np.random.default_rng([3, m.N, m.n])
    tv = random_words(rng, (3, m.N))
    trl = random_words(rng, (3, 2, m.N))
    cases = []
    try:
        e.set_decomposition(R._ffi.DECOMP_ROUNDED)
        with e.lut(tv) as lut, e.lut_encrypted(trl) as enc:
            for G in gk.forced_sizes(m.N, m.C):
                c0, c1 = random_words(rng, (G, m.n + 1)), random_words(rng, (G, m.n + 1))
                idx = rng.integers(0, 3, G).astype(np.int32)
                cases.append((c0, c1, idx, e.pbs_batch(lut, c0, idx), e.pbs_many_batch(lut, c1, 4, idx), e.pbs_many_batch(enc, c0, 4, idx)))
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
        with e.lut(tv) as lut:
            c0, _, idx, pbs = cases[0][:4]
            assert not np.array_equal(e.pbs_batch(lut, c0, idx), pbs), "the rounded words are not the reference words"
    finally:
        e.set_decomposition(R._ffi.DECOMP_REFERENCE)
    for env in FORCED[m.N]:
        f = m.engine(monkeypatch, env)
        try:
            f.set_decomposition(R._ffi.DECOMP_ROUNDED)
            with f.lut(tv) as lut, f.lut_encrypted(trl) as enc:
                for c0, c1, idx, pbs, many, many_enc in cases:
                    G = len(idx)
                    assert np.array_equal(f.pbs_batch(lut, c0, idx), pbs), (env, "pbs_batch", G)
                    assert np.array_equal(f.pbs_many_batch(lut, c1, 4, idx), many), (env, "pbs_many_batch", G)
                    assert np.array_equal(f.pbs_many_batch(enc, c0, 4, idx), many_enc), (env, "encrypted table", G)
        finally:
            f.close()


def test_forced_shapes_equal_the_default_engine_in_rounded_mode_n1024(mask1024, monkeypatch):
    _forced_shapes(mask1024, monkeypatch)


def test_forced_shapes_equal_the_default_engine_in_rounded_mode_n2048(mask2048, monkeypatch):
    _forced_shapes(mask2048, monkeypatch)
