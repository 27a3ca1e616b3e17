"""GPU: the FP64 mirror's bootstrap kernel families under PRESCRIBED rotations (tests/rotation_kit.py: rotation, schedule_inputs).

The rotation X^abar_i * acc in front of every CMUX step has index, sign and layout arithmetic of its own in every family: the shared wave
step (rtfhe_body_wave.hpp), eight waves on one gate (rtfhe_body_wg.hpp), (polynomial, parity) per wave with abar as u16
(rtfhe_body_pair4.hpp), and at N = 2048 the accumulator in two parity planes (rtfhe_body_eo.hpp, rtfhe_body_eo4.hpp: source plane
(H - r) & 1, word shift (H - r) >> 1, the sign from bit 10 of the word index).  Here the 64 mask words of 8 inputs are r << SH, which the mod
switch turns into abar_i = r exactly: every gate walks every coarse part r >> 6, the eight together every (coarse, fine) pair with fine in
(0, 1, 2, 31, 32, 33, 62, 63), gate 0 alone sees 0, N and 2N - 1, and gates 0 .. 2 both parity planes of every coarse part.  The body words
are b_edges << SH (odd gates with the low bits set), so the prologue's start X^-bbar stands on its edges too.  n = 64: 64 steps are the
whole schedule and n + 1 = 65 is odd.

Expectations come from the oracle once per ring and are read-only; batches of more than 8 gates are the 8 inputs tiled and are compared with
the tiled expectation.  Which kernel an (engine, count, call) reaches is read from launch_bootstrap_n1024 / launch_bootstrap_n2048,
walk_ladder and pair4_tail_gates (rtfhe_dispatch_fft.hip, rtfhe_host.hpp) with C = the device's CU count, and stated in each docstring.
Every comparison is np.array_equal on uint32 words; a failure names the engine, the count, the first differing gate, and for the
accumulators the first wrong step with its rotation's coarse part, fine part and plane."""
import numpy as np
import pytest

import gpu_kit as gk
import rotation_kit as rk
import round_oracle as ro
from kit import random_words
from mask_kit import Mask
from pbs_oracle import oracle_pbs, oracle_pbs_enc, oracle_pbs_many

pytestmark = pytest.mark.gpu

N_MASK = 64
DEFAULT = None
WAVES1, WAVES4, WAVES8 = {"RTFHE_FORCE_WAVES": "1"}, {"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_FORCE_WAVES": "8"}
NO_PAIR4, NO_EO4, FUSED = {"RTFHE_PAIR4": "0"}, {"RTFHE_N2048_EO4": "0"}, {"RTFHE_KS_MM_MIN": "0"}


class World:
    """one ring: the n = 64 key set with its default engine, the 8 schedule inputs, and what the oracle makes of them"""

    def __init__(self, orc, N):
        import rustfhe_amd as R
        self.orc, self.N = orc, N
        self.m = m = Mask(orc, N, N_MASK)
        P, K = m.P, m.K
        rng = np.random.default_rng(0x5C4ED + N)
        self.t = t = rk.schedule_inputs(rng, N, N_MASK)
        self.tv = tv = random_words(rng, (3, N))
        self.trl = trl = R.encrypt_lut(m.p, K.key1, tv, seed=N)
        self.idx = idx = (np.arange(rk.GATES) % 3).astype(np.int32)

        def per_gate(fn):
            return np.stack(gk.pmap(lambda g: fn(g, gk.oracle_plan(orc, N)), range(rk.GATES)))
        self.acc = per_gate(lambda g, pl: orc.blind_rotate(P, pl, K.bk_f, None, t[g], rk.STEPS))
        self.boot = m.gates(orc.COPY, t, None)
        self.pbs = per_gate(lambda g, pl: oracle_pbs(orc, P, pl, K.bk_f, K.ksk, tv[idx[g]], t[g]))
        self.many = {o: per_gate(lambda g, pl: oracle_pbs_many(orc, P, pl, K.bk_f, K.ksk, tv[idx[g]], t[g], o)) for o in (2, 8)}
        self.enc = {o: per_gate(lambda g, pl: oracle_pbs_enc(orc, P, pl, K.bk_f, K.ksk, trl[idx[g]], t[g], o)) for o in (1, 4)}
        self.rounded = per_gate(lambda g, pl: ro.pbs(P, pl, K.bk_f, K.ksk, tv[idx[g]], t[g]))
        for a in (t, tv, trl, idx, self.acc, self.boot, self.pbs, self.rounded, *self.many.values(), *self.enc.values()):
            a.setflags(write=False)

    def close(self):
        self.m.e.close()


@pytest.fixture(scope="module")
def worlds(orc):
    w = gk.Worlds(lambda N: World(orc, N))
    yield w
    w.close()


class Forced:
    """the world's default engine, or one created under `env` and closed on the way out"""

    def __init__(self, w, monkeypatch, env):
        self.w, self.mp, self.env = w, monkeypatch, env

    def __enter__(self):
        self.e = self.w.m.e if not self.env else self.w.m.engine(self.mp, self.env)
        return self.e

    def __exit__(self, *exc):
        if self.env:
            self.e.close()


def check_accumulators(w, e, env, sym):
    """blind_rotate_batch(t, 64) of `sym` gates against the oracle's accumulators"""
    count, P, K = rk.size(sym, w.m.C), w.m.P, w.m.K
    text = rk.accumulators_differ(lambda rows, s: e.blind_rotate_batch(rows, s).reshape(len(rows), -1),
                                  lambda row, s: w.orc.blind_rotate(P, gk.oracle_plan(w.orc, w.N), K.bk_f, None, row, s), w.t, w.acc, w.N, count)
    assert text is None, "%s, %s = %d gates, N = %d: %s" % (gk.env_id(env), sym, count, w.N, text)


def same(got, exp, w, env, sym, call, k=0):
    count = got.shape[0]
    diff = rk.first_difference(got, rk.tiled(exp, count), w.t, w.N, k)
    assert diff is None, "%s, %s = %d gates, N = %d, %s: %s" % (gk.env_id(env), sym, count, w.N, call, diff[1])


def check_whole_bootstraps(w, e, env, sym):
    """bootstrap_batch, pbs_batch (three tables, indices cycling), pbs_many_batch with n_out 2 and 8 (the mod switch at SH + 1 and SH + 3 turns
    the schedule into another one, which the oracle follows), the encrypted table with n_out 1 and 4, and pbs_batch in rounded mode"""
    import rustfhe_amd as R
    count = rk.size(sym, w.m.C)
    t, idx = rk.tiled(w.t, count), rk.tiled(w.idx, count)
    with e.lut(w.tv) as lut, e.lut_encrypted(w.trl) as enc:
        same(e.bootstrap_batch(t), w.boot, w, env, sym, "bootstrap_batch")
        same(e.pbs_batch(lut, t, idx), w.pbs, w, env, sym, "pbs_batch")
        for n_out, k in ((2, 1), (8, 3)):
            same(e.pbs_many_batch(lut, t, n_out, idx), w.many[n_out], w, env, sym, "pbs_many_batch n_out %d" % n_out, k)
        same(e.pbs_batch(enc, t, idx), w.enc[1][:, 0], w, env, sym, "encrypted table, pbs_batch")
        same(e.pbs_many_batch(enc, t, 4, idx), w.enc[4], w, env, sym, "encrypted table, n_out 4", 2)
        try:
            e.set_decomposition(R._ffi.DECOMP_ROUNDED)
            same(e.pbs_batch(lut, t, idx), w.rounded, w, env, sym, "pbs_batch, rounded")
        finally:
            e.set_decomposition(R._ffi.DECOMP_REFERENCE)


# ---- the accumulators after 64 prescribed steps, N = 1024 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["1", "3", "8"])
def test_N1024_accumulators_one_gate_per_workgroup(worlds, sym):
    """default engine, count <= wg_max = C: the tail's `count <= wg_max` branch of launch_bootstrap_n1024 launches k_bootstrap_wg, one gate on the
    eight waves of a workgroup, in MODE_BLIND_ROTATE"""
    w = worlds(1024)
    check_accumulators(w, w.m.e, DEFAULT, sym)


def test_N1024_accumulators_one_gate_per_workgroup_more_workgroups_than_cus(worlds, monkeypatch):
    """RTFHE_FORCE_WAVES=1, C + 8 gates: force == 1 sends the whole batch to k_bootstrap_wg, C + 8 workgroups on C CUs"""
    w = worlds(1024)
    with Forced(w, monkeypatch, WAVES1) as e:
        check_accumulators(w, e, WAVES1, "C+8")


@pytest.mark.parametrize("sym", ["C+8", "2C+8"])
def test_N1024_accumulators_four_waves_per_gate(worlds, sym):
    """default engine: C + 8 gates are a tail of two gates per CU, 2C + 8 of three; both pass wg_max, the mode is MODE_BLIND_ROTATE and pair4 = 3,
    so pair4_tail_gates gives 2 / 3 and the tail runs k_bootstrap_pair4<2> / k_bootstrap_pair4<3> ((polynomial, parity) per wave, abar as u16),
    the last workgroup partly filled"""
    w = worlds(1024)
    check_accumulators(w, w.m.e, DEFAULT, sym)


@pytest.mark.parametrize("sym", ["1", "3", "8", "4C+8"])
@pytest.mark.parametrize("env", [WAVES4, WAVES8], ids=gk.env_id)
def test_N1024_accumulators_one_wave_per_gate(worlds, monkeypatch, env, sym):
    """RTFHE_FORCE_WAVES=4 / 8: force sends the whole batch to k_bootstrap<10, .., 4> / <10, .., 8> (Wave10: the shared wave step, cmux_step),
    one gate per wave; at 1 and 3 gates the only workgroup is partly filled, at 4C + 8 the batch is more than a round and ends on a full one"""
    w = worlds(1024)
    with Forced(w, monkeypatch, env) as e:
        check_accumulators(w, e, env, sym)


# ---- the accumulators after 64 prescribed steps, N = 2048 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8"])
def test_N2048_accumulators_four_waves_per_gate(worlds, sym):
    """default engine: launch_bootstrap_n2048 walks the ladder in rounds of eo_round = 4 gates per CU; up to C gates are a tail of one gate per
    workgroup, C + 8 of two, and with eo4 = 1 in MODE_BLIND_ROTATE both run k_bootstrap_eo4<1> / k_bootstrap_eo4<2>.  A count of 3 already holds
    both parity planes of every coarse part."""
    w = worlds(2048)
    check_accumulators(w, w.m.e, DEFAULT, sym)


@pytest.mark.parametrize("sym", ["2C+8", "4C"])
def test_N2048_accumulators_two_waves_per_transform_three_and_four_gates(worlds, sym):
    """default engine: 2C + 8 gates are a tail of three gates per CU (k_bootstrap_eo<3>), 4C one whole round (k_bootstrap_eo<4>, tail = false);
    more than two gates per workgroup never take the four-wave kernel"""
    w = worlds(2048)
    check_accumulators(w, w.m.e, DEFAULT, sym)


@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8"])
def test_N2048_accumulators_two_waves_per_transform_one_and_two_gates(worlds, monkeypatch, sym):
    """RTFHE_N2048_EO4=0: eo4 = 0 keeps tails of one and two gates per CU on k_bootstrap_eo<1> / k_bootstrap_eo<2>"""
    w = worlds(2048)
    with Forced(w, monkeypatch, NO_EO4) as e:
        check_accumulators(w, e, NO_EO4, sym)


@pytest.mark.parametrize("sym", ["1", "8", "4C+8"])
def test_N2048_accumulators_one_wave_per_gate(worlds, monkeypatch, sym):
    """RTFHE_FORCE_WAVES=4: force_waves == 4 sends the whole batch to k_bootstrap<11, .., 4> (Wave11), the shared wave step at N = 2048"""
    w = worlds(2048)
    with Forced(w, monkeypatch, WAVES4) as e:
        check_accumulators(w, e, WAVES4, sym)


# ---- whole bootstraps over the same inputs: the prologue's start from bbar, the epilogue, and every twin -------------------------------------
# bootstrap_batch and a plain-table pbs_batch are MODE_GATE batches that take the split path (ks_mm_min = 1) and walk the ladder in MODE_EXTRACT on
# k_bootstrap_* / k_pbs_*; pbs_many_batch, an encrypted table and rounded mode go through launch_pbs_many in MODE_EXTRACT on k_pbs_many_*,
# k_pbs_enc_* and k_pbs_round_*<.., false>.  In MODE_EXTRACT the dispatch chooses as in MODE_BLIND_ROTATE, so every twin of a family is reached at
# the counts at which the accumulator tests reach its gate kernel; no twin of these families is out of the dispatch's reach.  (k_pbs_round_*<..,
# true>, the encrypted table in rounded mode, has its words checked in tests/test_gpu_pbs_round.py; here rounded mode runs the plain table.)
@pytest.mark.parametrize("sym", ["8", "C+8"])
@pytest.mark.parametrize("env", [DEFAULT, WAVES1, WAVES4, NO_PAIR4], ids=gk.env_id)
def test_N1024_whole_bootstraps_and_twins(worlds, monkeypatch, env, sym):
    """default: 8 gates on the _wg twins, C + 8 on the _pair4<2> twins.  RTFHE_FORCE_WAVES=1: the _wg twins at both counts, C + 8 workgroups.
    RTFHE_FORCE_WAVES=4: the one-wave-per-gate twins k_pbs*<10, .., 4>.  RTFHE_PAIR4=0: pair4_tail_gates gives 0, so C + 8 gates run the
    _pair<2> twins (8 gates: _wg)."""
    w = worlds(1024)
    with Forced(w, monkeypatch, env) as e:
        check_whole_bootstraps(w, e, env, sym)


@pytest.mark.parametrize("env,sym", [(DEFAULT, "8"), (DEFAULT, "2C+8"), (NO_EO4, "8"), (NO_EO4, "C+8"), (WAVES4, "8"), (WAVES4, "C+8")],
                         ids=lambda v: v if isinstance(v, str) else gk.env_id(v))
def test_N2048_whole_bootstraps_and_twins(worlds, monkeypatch, env, sym):
    """default: 8 gates on the _eo4<1> twins, 2C + 8 on the _eo<3> twins.  RTFHE_N2048_EO4=0: the _eo<1> twins at 8 gates, _eo<2> at C + 8.
    RTFHE_FORCE_WAVES=4: the one-wave-per-gate twins k_pbs*<11, .., 4>."""
    w = worlds(2048)
    with Forced(w, monkeypatch, env) as e:
        check_whole_bootstraps(w, e, env, sym)


@pytest.mark.parametrize("sym", ["8", "C+8"])
@pytest.mark.parametrize("N", rk.RINGS)
def test_fused_key_switch_route(worlds, monkeypatch, N, sym):
    """RTFHE_KS_MM_MIN=0: split_ok is false, so bootstrap_batch and a plain-table pbs_batch stay in MODE_GATE with the key switch fused into the
    kernel, where the four-wave kernels are not chosen (they have no fused key switch).  N = 2048: k_bootstrap_eo<1> / k_pbs_eo<1> at 8 gates,
    <2> at C + 8 -- the two-wave kernels in MODE_GATE.  N = 1024: k_bootstrap_wg / k_pbs_wg at 8 gates, k_bootstrap_pair<2> / k_pbs_pair<2> at
    C + 8."""
    w = worlds(N)
    count = rk.size(sym, w.m.C)
    t, idx = rk.tiled(w.t, count), rk.tiled(w.idx, count)
    with Forced(w, monkeypatch, FUSED) as e, e.lut(w.tv) as lut:
        same(e.bootstrap_batch(t), w.boot, w, FUSED, sym, "bootstrap_batch")
        same(e.pbs_batch(lut, t, idx), w.pbs, w, FUSED, sym, "pbs_batch")
