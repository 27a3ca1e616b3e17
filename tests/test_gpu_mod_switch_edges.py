"""GPU: the mod switch of every bootstrap prologue on the words where it changes its answer (tests/rotation_kit.py: edge_words,
body_edge_words, edge_rows).

The switch that makes abar_i and bbar is written out in gate_mask (rtfhe_gate_frame.hpp), in mod_switch (rtfhe_kernels.hpp) for the many-LUT
grid S = SH + k, and in the bodies that carry a pre-step of their own.  A mask word is rounded: the words half a step below and above q << S,
for q in (0, 1, N/2^k - 1, N/2^k, 2N/2^k - 1), one word to either side of each boundary, 0xFFFFFFFF and 0 -- the top half-step rounds up to 2N
and must come out as 0, as the reference's wrapping_add does (tfhe.rs:108).  A body word is floored: the last word of q - 1, the first and
the last of q.  In the 16 input rows every mask edge word stands at several step indices of every gate and every body edge word in one gate.

Every call is compared with the oracle's restatement (tests/pbs_oracle.py, orc.blind_rotate, orc.gate_batch_mt), computed once per ring and
read-only; batches of more than 16 gates are the 16 rows tiled.  Engines: the default one of both rings and one per other prologue -- the
wave body's own pre-step (RTFHE_FORCE_WAVES=4), the pair body's (RTFHE_FORCE_WAVES=2), the time-sliced pair body's u16 abar (a count in the
pair_rr window), the four-wave N = 1024 kernel, the one family of that ring on the shared gate_mask (a count of two gates per CU), and at
N = 2048 the two-wave kernels (RTFHE_N2048_EO4=0).  Every comparison is np.array_equal on uint32 words; a failure
names the engine, the count, the call, the first differing gate and its switched words."""
import numpy as np
import pytest

import gpu_kit as gk
import rotation_kit as rk
from kit import random_words
from mask_kit import Mask
from pbs_oracle import oracle_pbs, oracle_pbs_enc, oracle_pbs_many

pytestmark = pytest.mark.gpu

N_MASK = 64
ROWS = 2 * rk.GATES
DEFAULT, WAVES2, WAVES4, NO_EO4 = None, {"RTFHE_FORCE_WAVES": "2"}, {"RTFHE_FORCE_WAVES": "4"}, {"RTFHE_N2048_EO4": "0"}


class World:
    """one ring: the n = 64 key set with its default engine, the edge rows of every grid k = 0 .. 3 and what the oracle makes of them"""

    def __init__(self, orc, N):
        import rustfhe_amd as R
        self.orc, self.N = orc, N
        self.m = m = Mask(orc, N, N_MASK)
        P, K = m.P, m.K
        rng = np.random.default_rng(0xED6E + N)
        self.rows = rows = [rk.edge_rows(rng, N, N_MASK, k) for k in range(4)]
        self.zero = np.zeros_like(rows[0])
        self.tv = tv = random_words(rng, (3, N))
        self.trl = trl = R.encrypt_lut(m.p, K.key1, tv, seed=N + 1)
        self.idx = idx = (np.arange(ROWS) % 3).astype(np.int32)

        def per_gate(fn):
            return np.stack(gk.pmap(lambda g: fn(g, gk.oracle_plan(orc, N)), range(ROWS)))
        t = rows[0]
        self.acc = {s: per_gate(lambda g, pl: orc.blind_rotate(P, pl, K.bk_f, None, t[g], s)) for s in (1, rk.STEPS)}
        self.exact = np.stack(gk.pmap(lambda g: self.exact_oracle(t[g], rk.STEPS), range(ROWS)))
        self.boot = m.gates(orc.COPY, t, None)
        self.gate = {op: m.gates(op, t, self.zero) for op in (orc.NAND, orc.XOR)}
        self.pre = {op: np.stack([orc.gate_linear(P, op, x, z) for x, z in zip(t, self.zero)]) for op in (orc.NAND, orc.XOR)}
        self.pbs = per_gate(lambda g, pl: oracle_pbs(orc, P, pl, K.bk_f, K.ksk, tv[idx[g]], t[g]))
        self.enc1 = per_gate(lambda g, pl: oracle_pbs_enc(orc, P, pl, K.bk_f, K.ksk, trl[idx[g]], t[g], 1)[0])
        self.many = {k: per_gate(lambda g, pl: oracle_pbs_many(orc, P, pl, K.bk_f, K.ksk, tv[idx[g]], rows[k][g], 1 << k)) for k in (1, 2, 3)}
        self.enc4 = per_gate(lambda g, pl: oracle_pbs_enc(orc, P, pl, K.bk_f, K.ksk, trl[idx[g]], rows[2][g], 4))
        for a in (*rows, self.zero, tv, trl, idx, self.exact, self.boot, self.pbs, self.enc1, self.enc4, *self.acc.values(), *self.gate.values(),
                  *self.pre.values(), *self.many.values()):
            a.setflags(write=False)

    def exact_oracle(self, row, steps):
        orc = self.orc
        return orc.blind_rotate(self.m.P, gk.oracle_plan(orc, self.N, orc.BACKEND_EXACT), None, self.m.K.bk_t, row, steps)

    def close(self):
        self.m.e.close()


@pytest.fixture(scope="module")
def worlds(orc):
    w = gk.Worlds(lambda N: World(orc, N))
    yield w
    w.close()


def check_every_call(w, e, env, sym):
    import rustfhe_amd as R
    orc, N = w.orc, w.N
    count = rk.size(sym, w.m.C)

    def same(call, got, exp, t, k=0, steps=None):
        diff = rk.first_difference(got, rk.tiled(exp, count), t, N, k, steps)
        assert diff is None, "%s, %s = %d gates, N = %d, %s: %s" % (gk.env_id(env), sym, count, N, call, diff[1])
    t0, idx = rk.tiled(w.rows[0], count), rk.tiled(w.idx, count)
    for s in (1, rk.STEPS):
        same("blind_rotate_batch(t, %d)" % s, e.blind_rotate_batch(t0, s), w.acc[s], w.rows[0], steps=s)
    same("bootstrap_batch", e.bootstrap_batch(t0), w.boot, w.rows[0])
    zero = rk.tiled(w.zero, count)
    for op, gpu_op, name in ((orc.NAND, R.NAND, "NAND"), (orc.XOR, R.XOR, "XOR")):      # the pre-step moves the words before the switch
        same("gate_batch(%s, edge rows, zero rows); the words below are the pre-stepped ones" % name, e.gate_batch(gpu_op, t0, zero), w.gate[op], w.pre[op])
    with e.lut(w.tv) as lut, e.lut_encrypted(w.trl) as enc:
        same("pbs_batch", e.pbs_batch(lut, t0, idx), w.pbs, w.rows[0])
        same("encrypted table, n_out 1", e.pbs_batch(enc, t0, idx), w.enc1, w.rows[0])
        for k in (1, 2, 3):
            same("pbs_many_batch n_out %d" % (1 << k), e.pbs_many_batch(lut, rk.tiled(w.rows[k], count), 1 << k, idx), w.many[k], w.rows[k], k)
        same("encrypted table, n_out 4", e.pbs_many_batch(enc, rk.tiled(w.rows[2], count), 4, idx), w.enc4, w.rows[2], 2)


@pytest.mark.parametrize("env,sym", [(DEFAULT, "16"), (DEFAULT, "C+8"), (DEFAULT, "4C+8"), (WAVES4, "16"), (WAVES2, "16")],
                         ids=lambda v: v if isinstance(v, str) else gk.env_id(v))
def test_N1024_every_call_on_the_edge_words(worlds, monkeypatch, env, sym):
    """default, 16 gates: the _wg kernels and twins (k_bootstrap_wg, k_pbs_wg, k_pbs_many_wg, k_pbs_enc_wg), the workgroup body's pre-step.
    default, C + 8 gates: a tail of two gates per CU on k_bootstrap_pair4<2> and twins, the only N = 1024 family that takes the shared
    gate_mask (abar as u16); the gates go there through the split path.  default, 4C + 8 gates: more than a round and at most rr C, so
    rr_applies and the whole batch is one launch of the time-sliced pair kernels (k_bootstrap_pair_rr and twins), whose abar is u16.
    RTFHE_FORCE_WAVES=4: k_bootstrap<10, .., 4> and twins, the wave body's own pre-step.  RTFHE_FORCE_WAVES=2: k_bootstrap_pair<4> and twins,
    the pair body's."""
    w = worlds(1024)
    e = w.m.e if env is None else w.m.engine(monkeypatch, env)
    try:
        check_every_call(w, e, env, sym)
    finally:
        if env is not None:
            e.close()


@pytest.mark.parametrize("env", [DEFAULT, NO_EO4, WAVES4], ids=gk.env_id)
def test_N2048_every_call_on_the_edge_words(worlds, monkeypatch, env):
    """16 gates.  default: k_bootstrap_eo4<1> and twins.  RTFHE_N2048_EO4=0: k_bootstrap_eo<1> and twins.  RTFHE_FORCE_WAVES=4:
    k_bootstrap<11, .., 4> and twins, the wave body's own pre-step."""
    w = worlds(2048)
    e = w.m.e if env is None else w.m.engine(monkeypatch, env)
    try:
        check_every_call(w, e, env, "16")
    finally:
        if env is not None:
            e.close()


@pytest.mark.parametrize("backend", ["ntt", "xfft"])
@pytest.mark.parametrize("N", rk.RINGS)
def test_exact_backends_on_the_edge_words(worlds, N, backend):
    """blind_rotate_batch(t, 64) of the 16 k = 0 rows against the exact oracle: the prologues of k_bootstrap_ntt_wg / k_bootstrap_ntt_halves<1> /
    k_bootstrap_xpair<1> / k_bootstrap_xquad<1>"""
    import rustfhe_amd as R
    w = worlds(N)
    e = w.m.e
    try:
        e.set_backend({"ntt": R._ffi.BACKEND_NTT_EXACT, "xfft": R._ffi.BACKEND_FFT_SPLIT_EXACT}[backend])
        text = rk.accumulators_differ(lambda rows, s: e.blind_rotate_batch(rows, s).reshape(len(rows), -1), w.exact_oracle, w.rows[0], w.exact, N, ROWS)
    finally:
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert text is None, "%s, 16 gates, N = %d: %s" % (backend, N, text)
