"""GPU: the exact backends' bootstrap kernels -- the NTT (rtfhe_kernels_ntt*.hpp) and the split FFT (rtfhe_kernels_xfft*.hpp), each with a
prologue and a rotated gather of its own -- under the PRESCRIBED rotations of tests/rotation_kit.py, as tests/test_gpu_rotation_schedules.py
runs them on the FP64 mirror: the same n = 64 key sets, the same 8 inputs.

The expectation is the exact-integer oracle's blind rotation (schoolbook products, BACKEND_EXACT) of the 8 inputs after 64 steps, computed
once per ring and read-only; both backends are compared with it, which also makes them equal each other.  Batches of more than 8 gates are the
8 inputs tiled.  Which kernel a count reaches is read from launch_bootstrap_ntt (rtfhe_dispatch_ntt.hip), launch_bootstrap_xfft
(rtfhe_dispatch_xfft.hip) and walk_ladder (rtfhe_host.hpp) with C = the device's CU count, and stated in each docstring.  Every comparison is
np.array_equal on uint32 words; a failure names the backend, the count, the first differing gate and its first wrong step with the
rotation's coarse and fine part."""
import numpy as np
import pytest

import gpu_kit as gk
import rotation_kit as rk
from mask_kit import Mask

pytestmark = pytest.mark.gpu

N_MASK = 64
WAVES2, WAVES4 = {"RTFHE_FORCE_WAVES": "2"}, {"RTFHE_FORCE_WAVES": "4"}


class World:
    """one ring: the n = 64 key set with its default engine, the 8 schedule inputs and the exact oracle's accumulators and gates"""

    def __init__(self, orc, N):
        self.orc, self.N = orc, N
        self.m = m = Mask(orc, N, N_MASK)
        self.t = t = rk.schedule_inputs(np.random.default_rng(0x5C4ED + N), N, N_MASK)
        self.acc = np.stack(gk.pmap(lambda g: self.oracle(t[g], rk.STEPS), range(rk.GATES)))
        self.boot = m.gates(orc.COPY, t, None, backend=orc.BACKEND_EXACT)
        for a in (t, self.acc, self.boot):
            a.setflags(write=False)

    def oracle(self, row, steps):
        orc = self.orc
        return orc.blind_rotate(self.m.P, gk.oracle_plan(orc, self.N, orc.BACKEND_EXACT), None, self.m.K.bk_t, row, steps)

    def close(self):
        self.m.e.close()


@pytest.fixture(scope="module")
def worlds(orc):
    w = gk.Worlds(lambda N: World(orc, N))
    yield w
    w.close()


def backend_of(name):
    import rustfhe_amd as R
    return {"ntt": R._ffi.BACKEND_NTT_EXACT, "xfft": R._ffi.BACKEND_FFT_SPLIT_EXACT}[name]


def check_accumulators(w, e, backend, sym, env=None):
    """blind_rotate_batch(t, 64) of `sym` gates on `backend` against the exact oracle; the mirror backend is restored on the way out"""
    import rustfhe_amd as R
    count = rk.size(sym, w.m.C)
    try:
        e.set_backend(backend_of(backend))
        text = rk.accumulators_differ(lambda rows, s: e.blind_rotate_batch(rows, s).reshape(len(rows), -1), w.oracle, w.t, w.acc, w.N, count)
    finally:
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    assert text is None, "%s, %s, %s = %d gates, N = %d: %s" % (backend, gk.env_id(env), sym, count, w.N, text)


@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8", "2C+8", "3C+8", "4C", "4C+8"])
def test_N1024_ntt_every_tail_shape_and_a_whole_round(worlds, sym):
    """Rounds of four gates per CU.  Up to C gates: a tail of one gate per CU, k_bootstrap_ntt_wg.  C + 8, 2C + 8, 3C + 8: tails of two, three,
    four gates per workgroup, k_bootstrap_ntt_pair<2>, <3>, <4>.  4C: one whole round on k_bootstrap_ntt_pair<4> (tail = false).  4C + 8: the
    round and behind it a tail of 8 gates on k_bootstrap_ntt_wg, which reads its segment of the batch."""
    w = worlds(1024)
    check_accumulators(w, w.m.e, "ntt", sym)


@pytest.mark.parametrize("env,sym", [(WAVES4, "3"), (WAVES4, "8"), (WAVES4, "C+8"), (WAVES2, "8")], ids=lambda v: v if isinstance(v, str) else gk.env_id(v))
def test_N1024_ntt_forced_shapes(worlds, monkeypatch, env, sym):
    """RTFHE_FORCE_WAVES=4: the whole batch on k_bootstrap_ntt, one gate per wave in four-wave workgroups (3 gates: a partly filled workgroup;
    C + 8: more than one).  RTFHE_FORCE_WAVES=2: a tail of one gate per CU stays on two waves per gate, k_bootstrap_ntt_pair<1>."""
    w = worlds(1024)
    e = w.m.engine(monkeypatch, env)
    try:
        check_accumulators(w, e, "ntt", sym, env)
    finally:
        e.close()


@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8", "4C"])
def test_N2048_ntt_halves_at_tails_and_a_whole_round(worlds, sym):
    """k_bootstrap_ntt_halves<GATES>, two waves per gate, one per half of the transform: up to C gates <1>, C + 8 a tail of two gates per
    workgroup <2>, 4C one whole round <4>"""
    w = worlds(2048)
    check_accumulators(w, w.m.e, "ntt", sym)


@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8", "2C+8", "3C+8", "4C+8"])
def test_N1024_split_fft_every_shape_and_the_time_sliced_window(worlds, sym):
    """Up to C gates k_bootstrap_xpair<1>; C + 8, 2C + 8, 3C + 8 tails of two, three, four gates per workgroup, k_bootstrap_xpair<2>, <3>, <4>.
    4C + 8: one whole round and a remainder of 8, 4C + 8 <= xrr C, so the round rides with the remainder in ONE launch of five gates per CU
    on k_bootstrap_xpair_rr (time_sliced in launch_bootstrap_xfft)."""
    w = worlds(1024)
    check_accumulators(w, w.m.e, "xfft", sym)


@pytest.mark.parametrize("sym", ["1", "3", "8", "C+8", "2C+8"])
def test_N2048_split_fft_four_waves_per_gate(worlds, sym):
    """Rounds of two gates per CU: up to C gates a tail on k_bootstrap_xquad<1>, C + 8 a tail on k_bootstrap_xquad<2>, 2C + 8 a whole round on
    <2> (tail = false) and 8 gates on <1> behind it"""
    w = worlds(2048)
    check_accumulators(w, w.m.e, "xfft", sym)


@pytest.mark.parametrize("backend", ["ntt", "xfft"])
@pytest.mark.parametrize("N", rk.RINGS)
def test_whole_gates_on_the_exact_backends(worlds, N, backend):
    """bootstrap_batch (gate_batch(COPY): rtfhe_bootstrap_batch is that call) on the 8 inputs against the exact oracle's gates: the prologue's
    start from bbar on its edges, the sample extract and the key switch behind the prescribed rotations.  8 gates: k_bootstrap_ntt_wg /
    k_bootstrap_ntt_halves<1> / k_bootstrap_xpair<1> / k_bootstrap_xquad<1>, a MODE_GATE batch that walks the ladder in MODE_EXTRACT."""
    import rustfhe_amd as R
    w = worlds(N)
    e = w.m.e
    try:
        e.set_backend(backend_of(backend))
        diff = rk.first_difference(e.bootstrap_batch(w.t), w.boot, w.t, N)
        assert diff is None, "%s, bootstrap_batch, N = %d: %s" % (backend, N, diff[1])
    finally:
        e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
