"""CPU: tests/rotation_kit.py does what it claims.  The schedule of prescribed rotations covers the coarse parts, the fine parts, the parity
planes and the landmark rotations it is run for; its mask words are switched to exactly the rotations they prescribe; the edge words stand
where the mod switch changes its answer; and the kit's numpy restatement of the mod switch (rtfhe_kernels.hpp: mod_switch) is the expression
the PBS oracles use.  The rounding adds half a step mod 2^32 -- tfhe.rs:108 uses wrapping_add -- so the top half-step wrapping to 0 is the
reference's behaviour, pinned here."""
import numpy as np
import pytest

import pbs_oracle
import rotation_kit as rk

KS = (0, 1, 2, 3)


@pytest.mark.parametrize("N", rk.RINGS)
def test_the_schedule_covers_what_it_claims(N):
    Q = 2 * N // 64
    rs = [[rk.rotation(N, g, i) for i in range(rk.STEPS)] for g in range(rk.GATES)]
    assert all(0 <= r < 2 * N for row in rs for r in row)
    for g in range(rk.GATES):
        assert {r >> 6 for r in rs[g]} == set(range(Q)), g                               # every gate alone: every coarse part
    pairs = {(r >> 6, r & 63) for row in rs for r in row}
    assert pairs == {(c, f) for c in range(Q) for f in rk.FINE} and len(pairs) == Q * 8  # the eight together: every (coarse, fine) pair
    assert {0, N, 2 * N - 1} <= set(rs[0])                                               # gate 0 alone
    assert {1, N - 1, N + 1, 2 * N - 2} <= {r for row in rs for r in row}
    assert {(r >> 6, r & 1) for row in rs[:3] for r in row} == {(c, h) for c in range(Q) for h in (0, 1)}   # a count of 3: both planes of every coarse part


@pytest.mark.parametrize("N", rk.RINGS)
def test_a_shifted_rotation_is_switched_to_itself(N):
    sh = rk.sh_of(N)
    r = np.arange(2 * N, dtype=np.uint64)
    assert np.array_equal(rk.mod_switch(r << sh, False, sh, 0), r.astype(np.int64))
    assert np.array_equal(rk.mod_switch(r << sh, True, sh, 0), r.astype(np.int64))
    assert np.array_equal(rk.mod_switch((r << sh) + ((1 << sh) - 1), True, sh, 0), r.astype(np.int64))    # the floor drops the low bits


@pytest.mark.parametrize("N", rk.RINGS)
def test_schedule_inputs_hold_the_schedule_and_the_body_edges(N):
    n, sh = 64, rk.sh_of(N)
    t = rk.schedule_inputs(np.random.default_rng(1), N, n)
    assert t.shape == (rk.GATES, n + 1) and t.dtype == np.uint32
    for g in range(rk.GATES):
        assert rk.mod_switch(t[g, :n], False, sh, 0).tolist() == [rk.rotation(N, g, i) for i in range(rk.STEPS)]
        assert int(rk.mod_switch(t[g, n:], True, sh, 0)[0]) == rk.b_edges(N)[g]
        assert (int(t[g, n]) & ((1 << sh) - 1)) == (((1 << sh) - 1) if g % 2 else 0)
    long = rk.schedule_inputs(np.random.default_rng(1), N, 100)
    assert np.array_equal(long[:, :rk.STEPS], t[:, :rk.STEPS])
    assert len(set(long[:, rk.STEPS:100].reshape(-1).tolist())) > 200                   # behind the prefix: random words


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", rk.RINGS)
def test_edge_words_stand_on_the_rounding_and_floor_boundaries(N, k):
    S = rk.sh_of(N) + k
    ew, bw = rk.edge_words(N, k), rk.body_edge_words(N, k)
    assert ew.shape == (22,) and bw.shape == (16,) and ew.dtype == bw.dtype == np.uint32
    assert int(ew[-2]) == 0xFFFFFFFF and int(ew[-1]) == 0 and int(bw[-1]) == 0xFFFFFFFF
    got = rk.mod_switch(ew, False, S, k)
    assert np.array_equal(got, rk.edge_rounds_to(N, k))                                  # q - 1, q, q, q + 1 by construction
    top = ew[ew >= np.uint32(2 ** 32 - (1 << (S - 1)))]
    assert top.size >= 3 and not rk.mod_switch(top, False, S, k).any()                   # the top half-step wraps to 0 ...
    assert np.array_equal(rk.mod_switch(bw, True, S, k), rk.body_floors_to(N, k))
    for words, is_body in ((ew, False), (bw, False), (ew, True), (bw, True)):
        r = rk.mod_switch(words, is_body, S, k)
        assert (r >= 0).all() and (r < 2 * N).all() and not (r % (1 << k)).any()         # ... and nothing ever gives 2N
        fn = pbs_oracle.switch_body if is_body else pbs_oracle.switch_mask
        assert r.tolist() == [fn(w, S, k) for w in words]                                # the oracles' own expression


@pytest.mark.parametrize("N", rk.RINGS)
def test_the_restatement_is_the_oracles_expression_on_every_boundary_of_the_grid(N):
    """not only on the edge words: every multiple of half a step of the finest grid, one word below and one above, at every k"""
    sh = rk.sh_of(N)
    base = np.arange(4 * N + 1, dtype=np.int64) << (sh - 1)
    words = (np.concatenate([base - 1, base, base + 1]) & 0xFFFFFFFF).astype(np.uint32)
    for k in KS:
        for is_body, fn in ((False, pbs_oracle.switch_mask), (True, pbs_oracle.switch_body)):
            r = rk.mod_switch(words, is_body, sh + k, k)
            assert r.tolist() == [fn(w, sh + k, k) for w in words]
            assert (r >= 0).all() and (r < 2 * N).all() and not (r % (1 << k)).any()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("N", rk.RINGS)
def test_edge_inputs_put_every_edge_word_into_every_gate(N, k):
    n = 64
    ew, bw = rk.edge_words(N, k), rk.body_edge_words(N, k)
    rows = rk.edge_rows(np.random.default_rng(2), N, n, k)
    assert rows.shape == (2 * rk.GATES, n + 1) and rows.dtype == np.uint32
    assert np.array_equal(rows[:rk.GATES], rk.edge_inputs(None, N, n, k)) and np.array_equal(rows[rk.GATES:], rk.edge_inputs(None, N, n, k, 1))
    for g in range(2 * rk.GATES):
        assert rows[g, :n].tolist() == [int(ew[(i + 5 * (g % rk.GATES)) % 22]) for i in range(n)]
        for j in range(22):
            assert np.count_nonzero(rows[g, :n] == ew[j]) >= 2, (g, j)                   # at several step indices of every gate
    for j in range(22):                                                                  # at different step indices in different gates
        assert len({int(np.flatnonzero(rows[g, :n] == ew[j])[0]) for g in range(rk.GATES)}) >= 4, j
    assert rows[:, n].tolist() == bw.tolist()                                            # every body edge word once
