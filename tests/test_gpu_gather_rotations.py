"""GPU: the pair kernels' coarse/fine rotated gather (rotated_gather, rustfhe_amd/csrc/rtfhe_device.hpp) under PRESCRIBED rotation amounts.
The mask words of the inputs are a[i] = r_i << 21, which the mod switch turns into abar_i = r_i exactly, so the blind rotation walks a
schedule of rotations instead of whatever a ciphertext happens to hold: every coarse part r >> 6 (the 16 cases of the dispatch under both
global signs), the fine parts r & 63 in {0, 1, 31, 63} (no lane wraps, one, half, all but one), and r = 0, N, 2N - 1.  The accumulators after
64 steps are the oracle's blind-rotate prefix bit for bit, at 1, 3 and 8 gates in the 2- and 4-gates-per-workgroup instantiations of
k_bootstrap_pair, in the 3-gates one and in the time-sliced kernel (both take more than two gates per CU: the 8 gates tiled), and a whole
programmable bootstrap over the same schedule is the oracle's PBS through k_pbs_pair."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from pbs_oracle import oracle_pbs

pytestmark = pytest.mark.gpu

GATES, STEPS, FINE = 8, 64, (0, 1, 31, 63)
PAIR2 = {"RTFHE_WG_MAX_GATES": "0", "RTFHE_PAIR4": "0"}      # small batches on k_bootstrap_pair<2>, 2 C < count <= 3 C gates on <3>
PAIR4 = {"RTFHE_FORCE_WAVES": "2"}                           # every batch on k_bootstrap_pair<4> / k_pbs_pair<4>


def rotation(g, i):
    """gate g, step i: coarse part (i + 6 g) mod 32, fine part from FINE so that one gate sees every coarse part under two fine parts and
    gates g, g + 1 together every (coarse, fine) combination"""
    i %= STEPS
    return 64 * ((i + 6 * g) % 32) + FINE[(2 * (i // 32) + i % 2 + g) % 4]


def test_the_schedule_covers_what_it_claims():
    N = 1024
    for g in range(GATES):
        rs = [rotation(g, i) for i in range(STEPS)]
        assert {r >> 6 for r in rs} == set(range(32)) and {r & 63 for r in rs} == set(FINE)
    r0 = {rotation(0, i) for i in range(STEPS)}
    assert {0, N, 2 * N - 1} <= r0
    both = {(r >> 6, r & 63) for g in (0, 1) for r in (rotation(g, i) for i in range(STEPS))}
    assert len(both) == 32 * len(FINE)


@pytest.fixture(scope="module")
def world(orc, params, keys):
    """the 8 inputs, their oracle accumulators after 64 steps (computed once, read-only) and the two forced-shape contexts"""
    import rustfhe_amd as R
    assert params.N == 1024 and params.n >= STEPS
    rng = np.random.default_rng(0x6A7)
    t = random_words(rng, (GATES, params.n + 1))      # the b word and the mask words behind the prefix: random
    for g in range(GATES):
        for i in range(params.n):
            t[g, i] = rotation(g, i) << 21
    pl = orc.Plan(params.N)
    exp = np.stack([orc.blind_rotate(params, pl, keys.bk_f, None, x, STEPS) for x in t])
    t.setflags(write=False); exp.setflags(write=False)
    p = R.Params(n=params.n, N=params.N, l=params.l, bgbit=params.bgbit, ks_t=params.ks_t, ks_basebit=params.ks_basebit)
    mp = pytest.MonkeyPatch()
    engines = {}
    try:
        engines["pair2"] = gk.engine(R, p, keys.bk_t, keys.ksk, mp, PAIR2)
        engines["pair4"] = gk.engine(R, p, keys.bk_t, keys.ksk, mp, PAIR4)
        yield t, exp, engines
    finally:
        mp.undo()
        for e in engines.values():
            e.close()


@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("shape", ["pair2", "pair4"])
def test_prescribed_rotations_match_the_oracle(world, shape, count):
    t, exp, engines = world
    acc = engines[shape].blind_rotate_batch(t[:count], STEPS)
    assert np.array_equal(acc.reshape(count, -1), exp[:count])


def test_prescribed_rotations_three_gates_per_workgroup(world):
    """2 C + 8 gates, the 8 tiled: one workgroup of three gates per CU (k_bootstrap_pair<3>), the last ones partly filled"""
    t, exp, engines = world
    reps = (2 * gk.cus() + GATES) // GATES
    acc = engines["pair2"].blind_rotate_batch(np.tile(t, (reps, 1)), STEPS)
    assert np.array_equal(acc.reshape(reps * GATES, -1), np.tile(exp, (reps, 1)))


def test_prescribed_rotations_time_sliced(world, engine):
    """4 C + 8 gates on the default dispatch: one launch of five gates per CU on k_bootstrap_pair_rr, which shares the gather"""
    t, exp, _ = world
    reps = (4 * gk.cus() + GATES) // GATES
    acc = engine.blind_rotate_batch(np.tile(t, (reps, 1)), STEPS)
    assert np.array_equal(acc.reshape(reps * GATES, -1), np.tile(exp, (reps, 1)))


def test_prescribed_rotations_through_the_pbs_twin(world, orc, params, keys):
    """k_pbs_pair<4>: a whole programmable bootstrap of random tables whose n steps cycle through the schedule"""
    t, _, engines = world
    rng = np.random.default_rng(0x6A8)
    tv = random_words(rng, (2, params.N))
    idx = np.array([0, 1, 1], np.int32)
    e = engines["pair4"]
    with e.lut(tv) as lut:
        out = e.pbs_batch(lut, t[:3], idx)
    pl = orc.Plan(params.N)
    for g in range(3):
        assert np.array_equal(out[g], oracle_pbs(orc, params, pl, keys.bk_f, keys.ksk, tv[idx[g]], t[g])), g
