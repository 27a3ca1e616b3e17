"""GPU: the TRLWE key switch (rtfhe_trlwe_ksk_create, rtfhe_trlwe_auto_batch[_dev]; k_trlwe_auto).  Every word against the restatement
(tests/auto_oracle.py: the oracle's own blocks in round_oracle.external_product's order) in both leveled decomposition modes, on rows of random
words with the decomposition's edge words planted and on rows of real encryptions, with real switching keys of one and of six exponents; the
anchor on the device (the stage-level external product on the padded TRGSW); sigma_t followed by sigma_(t^-1) under trivial keys; meaning with
real keys and the example; capture and replay, launch counts, refusals, the exact backends, a two-entry context, a destroyed context and a
destroyed key.  Contexts hold no key unless a test needs one: n = 40 (n = 24 at N = 2048, as the extract tests use)."""
import numpy as np
import pytest

import auto_oracle as A
import gpu_kit as gk
import trgsw_mac_oracle as O
from gpu_kit import FILL
from kit import SMALL_N, i32, load_example, torus_err

pytestmark = pytest.mark.gpu

ROWS = 5


def exponents(N):
    """entry 0 re-keys (t = 1, key A -> key B); the others are automorphisms under key B"""
    return [1, 3, 5, N // 2 + 1, N + 1, 2 * N - 1]


class World:
    """per N, built on first use: a context with nothing loaded, two lvl1 keys, the six-exponent switching key (entry 0 from key A to key B, the
    rest under B) and a one-exponent key (t = 2N - 1 under B), five rows -- planted edge words at 0, 2, 4, real encryptions under A and B at
    1, 3 --, the oracle's plan and spectra, and a memo of oracle words -- computed once, shared, read-only"""

    def __init__(self, R, orc, N):
        self.R, self.orc, self.N = R, orc, N
        self.rp = R.Params(n=SMALL_N[N], N=N)
        self.p = orc.Params(n=SMALL_N[N], N=N)
        self.plan = orc.Plan(N)
        _, self.keyA, _, _ = R.keygen(self.rp, 0xA70 + N, want_bk=False, want_ksk=False)
        _, self.keyB, _, _ = R.keygen(self.rp, 0xA71 + N, want_bk=False, want_ksk=False)
        self.t = {"k6": exponents(N), "k1": [2 * N - 1]}
        self.words = {"k6": np.concatenate([R.trlwe_ksk_keygen(self.rp, self.keyA, self.keyB, [1], seed=0xA72 + N),
                                            R.trlwe_ksk_keygen(self.rp, self.keyB, self.keyB, self.t["k6"][1:], seed=0xA73 + N)]),
                      "k1": R.trlwe_ksk_keygen(self.rp, self.keyB, self.keyB, self.t["k1"], seed=0xA74 + N)}
        self.key_f = {k: A.spectra(self.p, self.plan, w) for k, w in self.words.items()}
        rng = np.random.default_rng(0xA75 + N)
        self.msgs = rng.integers(0, 8, (2, N))
        x = O.rows_with_edges(0xA76 + N, N, ROWS)
        x[1] = R.encrypt_lut(self.rp, self.keyA, R.encode_msgs(self.msgs[0], 3), seed=0xA77 + N)[0]
        x[3] = R.encrypt_lut(self.rp, self.keyB, R.encode_msgs(self.msgs[1], 3), seed=0xA78 + N)[0]
        x.setflags(write=False)
        self.x = x
        self.eng = R.Engine(self.rp, 0)
        self.keys = {k: self.eng.trlwe_switch_key(w, self.t[k]) for k, w in self.words.items()}
        self.memo = {}

    def oracle(self, mode, which, entry, add, count):
        return gk.memo(self.memo, (mode, which, list(entry), "none" if add is None else list(add), count),
                       lambda: A.program(self.p, self.plan, self.key_f[which], self.t[which], self.x[:count], entry, add, mode))

    def mode(self, mode):
        self.eng.set_leveled_decomposition(self.R._ffi.DECOMP_ROUNDED if mode == A.ROUNDED else self.R._ffi.DECOMP_REFERENCE)

    def close(self):
        for k in self.keys.values():
            k.close()
        self.eng.close()


@pytest.fixture(scope="module")
def worlds(orc):
    import rustfhe_amd as R
    made = gk.Worlds(lambda N: World(R, orc, N))

    def get(N):
        w = made(N)
        w.mode(A.REFERENCE)
        return w
    yield get
    made.close()


def _dev(eng, key, x, entry, add=None, in_place=False, stream=None):
    """the _dev form.  Out of place: into a 0x5A-filled buffer with CANARY words behind it; in place: the rows themselves sit in front of the
    CANARY words.  The canaries are checked here; u32[count][2][N]"""
    import torch
    count, N = x.shape[0], x.shape[2]
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    if in_place:
        d_out = gk.guarded_out(count * 2 * N, init=x)
        eng.trlwe_auto_batch_dev(key, d_out, d_out, count, entry, add, st)
    else:
        d_out = gk.guarded_out(count * 2 * N)
        eng.trlwe_auto_batch_dev(key, gk.to_device(x, np.uint32), d_out, count, entry, add, st)
    eng.sync(st)
    return gk.read_guarded(d_out, count * 2 * N).reshape(count, 2, N)


# (count, key, entries, add, in place): ragged four-wave workgroups (count 1, 2, 3, 5), programs of 1, 2, 3 and 16 steps that mix replace and
# add, the one-exponent and the six-exponent key with every entry, an entry used twice, add given and NULL, out of place and in place
SHAPES = [
    (1, "k1", [0], None, False),
    (2, "k6", [1, 4], [0, 1], True),
    (3, "k6", [2, 2, 5], [1, 0, 1], False),
    (5, "k6", [(3 * k + 1) % 6 for k in range(16)], [int(k % 3 == 1) for k in range(16)], False),
    (5, "k6", [0], [1], True),
    (3, "k6", [3, 0], None, False),
    (2, "k1", [0, 0, 0], [0, 1, 0], True),
]


@pytest.mark.parametrize("N", [1024, 2048])
@pytest.mark.parametrize("mode", [A.REFERENCE, A.ROUNDED])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_every_word_equals_the_restatement(worlds, N, mode, shape):
    """host and _dev forms"""
    w = worlds(N)
    w.mode(mode)
    count, which, entry, add, in_place = SHAPES[shape]
    want = w.oracle(mode, which, entry, add, count)
    got = w.eng.trlwe_auto_batch(w.keys[which], w.x[:count], entry, add)
    assert got.shape == (count, 2, N) and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])
    dev = _dev(w.eng, w.keys[which], w.x[:count], entry, add, in_place)
    bad = np.argwhere(dev != want)
    assert bad.size == 0, (len(bad), bad[:5])


@pytest.mark.parametrize("N", [1024, 2048])
def test_anchor_the_stage_level_external_product_on_the_padded_trgsw(worlds, N):
    """one step == (sigma_t b, 0) + rtfhe_external_product_batch(T, (sigma_t a, 0)), word for word, in both modes: T, the entry's rows padded
    with zero rows, loaded as a bootstrapping key of a second context"""
    w, R = worlds(N), worlds(N).R
    t = w.t["k6"]
    bk = np.zeros((w.rp.n, 2, 2 * w.rp.l, N), np.uint32)
    for e in range(len(t)):
        bk[e] = A.padded_trgsw(w.rp, w.words["k6"], e)
    keyed = R.Engine(w.rp, 0)
    try:
        keyed.load_bk_torus(bk)
        for mode in (A.REFERENCE, A.ROUNDED):
            w.mode(mode)
            keyed.set_leveled_decomposition(R._ffi.DECOMP_ROUNDED if mode == A.ROUNDED else R._ffi.DECOMP_REFERENCE)
            for e in range(len(t)):
                inp = np.zeros((ROWS, 2, N), np.uint32)
                inp[:, 0] = R.trlwe_automorphism(w.x[:, 1], t[e])
                want = keyed.external_product_batch(i32([e] * ROWS), inp)
                want[:, 0] += R.trlwe_automorphism(w.x[:, 0], t[e])
                assert np.array_equal(w.eng.trlwe_auto_batch(w.keys["k6"], w.x, [e]), want), (mode, t[e])
    finally:
        keyed.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_sigma_t_then_its_inverse_under_trivial_keys(worlds, N):
    """Noiseless trivial keys, rows (-sigma_t(s) g_j, 0).  With s = 0 (all-zero rows) a step is (sigma_t b, 0) exactly, and sigma_t followed by
    sigma_(t^-1) returns (b, 0): the phase under s = 0, word for word.  With a binary s the pair returns (b - a s - sigma_(t^-1)(e) s, 0) with
    e the recomposition error of sigma_t(a)'s digits (the second step decomposes a = 0: nothing): within hw(s) max|e| of the row's phase under
    s, plus one unit of 2^-32 per transform's truncation -- max|e| is 2^13 in rounded mode and 2^15 in reference mode
    (tests/test_gpu_trgsw_mac.py, the anchors)."""
    w, R = worlds(N), worlds(N).R
    pairs = [(t, A.inverse_exponent(N, t)) for t in (3, N // 2 + 1, 2 * N - 1)]      # (2N - 1 is its own inverse)
    t_list = sorted({v for pr in pairs for v in pr})
    for s, name in ((None, "zero"), (w.keyB, "binary")):
        with w.eng.trlwe_switch_key(A.trivial_key(w.rp, t_list, s), t_list) as key:
            for mode, emax in ((A.REFERENCE, 2 ** 15), (A.ROUNDED, 2 ** 13)):
                w.mode(mode)
                for t, ti in pairs:
                    back = w.eng.trlwe_auto_batch(key, w.x, [t_list.index(t), t_list.index(ti)])
                    assert (back[:, 1] == 0).all()
                    if s is None:
                        assert np.array_equal(back[:, 0], w.x[:, 0]), (mode, t)
                    else:
                        ph = R.trlwe_phase(w.rp, s, w.x)
                        e = np.abs((back[:, 0] - ph).view(np.int32).astype(np.int64))
                        assert 0 < e.max() <= int(np.sum(s)) * emax + 2, (mode, t, e.max())


def test_meaning_with_real_keys(worlds, orc):
    """auto_oracle.meaning_world on the device, rounded mode, N = 1024: the re-key (t = 1, key A -> key B) and the 4-step partial trace against
    the bounds tests/test_trlwe_auto_host.py holds the restatement to; exactly the coefficients = 0 mod 16 carry 16 x the message (rows encoded 16
    times smaller, so that the survivors decode to the messages), the others decrypt to 0; nothing decodes under the old key"""
    w, R = worlds(1024), worlds(1024).R
    m = A.meaning_world(R)
    assert (m.rp.n, m.rp.N) == (w.rp.n, w.rp.N)
    N = m.rp.N
    w.mode(A.ROUNDED)
    with w.eng.trlwe_switch_key(m.k_rekey, m.t_rekey) as rekey, w.eng.trlwe_switch_key(m.k_auto, m.t_auto) as auto:
        moved = w.eng.trlwe_auto_batch(rekey, m.rowsA, [0])
        traced = w.eng.trlwe_auto_batch(auto, m.rows_trace, m.trace_entries, [1] * 4)
    ph = R.trlwe_phase(m.rp, m.keyB, moved)
    err, bound = float(np.abs(torus_err(ph, m.plain)).max()), A.step_bound(N, m.hwA)
    print("re-key: largest |error| %.3e, bound %.3e" % (err, bound))
    assert err <= bound and np.array_equal(R.decode_msgs(ph, m.MSG_BITS), m.msgs)
    assert np.mean(R.decode_msgs(R.trlwe_phase(m.rp, m.keyA, moved), m.MSG_BITS) == m.msgs) < 0.5
    bound = A.trace_bound(N, m.hwB, 4)
    ratio = A.check_trace(R, m, traced, bound)      # within the bound of 16 x the message at = 0 mod 16 and of 0 elsewhere; the survivors decode
    print("4-step partial trace: largest |error| %.3e, bound %.3e" % (ratio * bound, bound))


def test_key_rotation_example(engine, keys):
    """examples/key_rotation.py on the session's engine and key set (key set B) at 8 rows: table and packed row re-keyed from a fresh key A,
    the bootstrap over the re-keyed table decodes under B, the packed row decodes under B and not under A, the 3-step partial trace keeps
    every 8th coefficient"""
    import rustfhe_amd as R
    ex = load_example("key_rotation")
    _, key1_a, _, _ = R.keygen(engine.p, 0xCE1, want_bk=False, want_ksk=False)
    before = (engine.decomposition(), engine.leveled_decomposition())
    res = ex.run(engine, key1_a, keys.key0, keys.key1, rows=8, seed=0xCE2)
    assert (engine.decomposition(), engine.leveled_decomposition()) == before
    N = engine.p.N
    assert np.array_equal(res["got"], res["want"]), (res["got"], res["want"])
    assert np.array_equal(res["packed_under_b"], res["packed_want"]) and res["packed_want"].any()
    assert np.sum(res["packed_under_a"] == res["packed_want"]) < N // 2 and res["table_words_under_a"] < 0.5
    assert float(np.abs(torus_err(res["trace_phase"], res["trace_want"])).max()) < 2.0 ** -(ex.MSG_BITS + 2)
    survivors = np.flatnonzero(res["trace_want"])
    assert (survivors % 8 == 0).all() and survivors.size > N // 16      # the packed row is full: of the N / 8 kept coefficients 3 in 4 hold a non-zero message
    dec = R.decode_msgs(res["trace_phase"], ex.MSG_BITS)
    assert np.array_equal(dec[::8], res["packed_want"][::8]) and (np.delete(dec, np.arange(0, N, 8)) == 0).all()


def test_capture_first_thing_on_a_fresh_stream_and_replay():
    """a fresh context whose first key switch sits in a capture, on a stream nothing has run on; two replays"""
    import torch
    import rustfhe_amd as R
    import orc as orc_mod
    N = 1024
    rp = R.Params(n=SMALL_N[N], N=N)
    p, plan = orc_mod.Params(n=SMALL_N[N], N=N), orc_mod.Plan(N)
    _, key1, _, _ = R.keygen(rp, 0xA81, want_bk=False, want_ksk=False)
    t = [3, N + 1]
    words = R.trlwe_ksk_keygen(rp, key1, key1, t, seed=0xA82)
    x = O.rows_with_edges(0xA83, N, 5)
    entry, add = [1, 0, 1], [0, 1, 1]
    want = A.program(p, plan, A.spectra(p, plan, words), t, x, entry, add, A.REFERENCE)
    e = R.Engine(rp, 0)
    try:
        with e.trlwe_switch_key(words, t) as key:
            s = torch.cuda.Stream()
            d_x = gk.to_device(x, np.uint32)
            d_out = torch.zeros((5, 2, N), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):      # nothing has run on s, and no key switch on this context: the call allocates nothing
                    e.trlwe_auto_batch_dev(key, d_x, d_out, 5, entry, add, s.cuda_stream)
                for _ in range(2):
                    d_out.zero_()
                    g.replay()
                    torch.cuda.synchronize()
                    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
            e.sync(s.cuda_stream)
            del g
    finally:
        e.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_one_launch_per_call(worlds, N):
    import torch
    w = worlds(N)
    st = torch.cuda.current_stream().cuda_stream
    d_x = gk.to_device(w.x, np.uint32)
    for count, which, entry, add, _ in (SHAPES[0], SHAPES[3], SHAPES[5]):
        d_out = torch.zeros((count, 2, N), dtype=torch.int32, device="cuda")
        w.eng.timer_begin(st)
        w.eng.trlwe_auto_batch_dev(w.keys[which], d_x, d_out, count, entry, add, st)
        assert w.eng.timer_end(st)[1] == 1
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), w.oracle(A.REFERENCE, which, entry, add, count))


def test_refusals_leave_the_output_untouched(worlds):
    import torch
    N = 1024
    w = worlds(N)
    R, e = w.R, w.eng
    key = w.keys["k6"]
    d_x = gk.to_device(w.x, np.uint32)
    d_out = torch.full((ROWS, 2, N), FILL, dtype=torch.int32, device="cuda")
    d_both = torch.full((6, 2, N), FILL, dtype=torch.int32, device="cuda")      # rows and output in one allocation
    out_host = np.full((ROWS, 2, N), FILL, np.uint32)
    e.timer_begin()

    alive = []      # the host arrays of the calls below, kept until the test ends

    def arr(v):
        if v is None:
            return None
        alive.append(i32(v))
        return alive[-1].ctypes.data

    def dev(key=key, entry=(0,), add=None, n=None, x=d_x.data_ptr(), out=d_out.data_ptr(), count=3, h=e.h):
        entry = None if entry is None else list(entry)
        return e.L.rtfhe_trlwe_auto_batch_dev(h, key.h if key is not None else None, arr(entry), arr(add), len(entry) if n is None else n, x, out, count, None)

    def host(entry=(0,), add=None, n=None, count=3, x=w.x):
        entry = None if entry is None else list(entry)
        return e.L.rtfhe_trlwe_auto_batch(e.h, key.h, arr(entry), arr(add), len(entry) if n is None else n, x.ctypes.data, out_host.ctypes.data, count)

    for call, word in ((lambda: dev(n=0), "n_steps = 0"), (lambda: host(n=0), "n_steps = 0"), (lambda: dev(entry=[0] * 17), "n_steps = 17"),
                       (lambda: host(entry=[0] * 17), "n_steps = 17"), (lambda: dev(entry=[0, 6]), "step 1: entry = 6"), (lambda: host(entry=[5, 0, -1]), "step 2: entry = -1"),
                       (lambda: dev(entry=[0, 1], add=[0, 2]), "step 1: add = 2"), (lambda: host(entry=[0, 1], add=[-1, 0]), "step 0: add = -1"),
                       (lambda: dev(count=1 << 31), "count"), (lambda: dev(entry=None, n=1), "null"), (lambda: dev(x=0), "null"), (lambda: dev(out=0), "null"),
                       (lambda: dev(key=None), "null switching key"),
                       (lambda: dev(x=d_both.data_ptr(), out=d_both[2].data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[2].data_ptr(), out=d_both.data_ptr()), "overlaps"),
                       (lambda: dev(x=d_both[3].data_ptr(), out=d_both[3].data_ptr() - 4), "overlaps"),
                       (lambda: dev(x=w.x.ctypes.data), "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(call())
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (word, str(ei.value))
    assert e.L.rtfhe_trlwe_auto_batch_dev(None, key.h, arr([0]), None, 1, d_x.data_ptr(), d_out.data_ptr(), 3, None) == R._ffi.ERR_INVALID      # null context
    # a key's creation: the exponent rules, before anything is allocated
    h = e.L.rtfhe_trlwe_ksk_create
    import ctypes as C
    words = w.words["k6"]
    for tt, n_t, word in (([2], 1, "entry 0: t = 2"), ([1, 3, 1], 3, "entry 2"), ([2 * N + 1], 1, "entry 0"), ([1], 0, "n_t = 0"), (list(range(1, 131, 2)), 65, "n_t = 65")):
        out_h = C.c_void_p()
        with pytest.raises(R.RtfheError) as ei:
            e._ck(h(e.h, words.ctypes.data, arr(tt), n_t, C.byref(out_h)))
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value) and not out_h, (word, str(ei.value))
    assert dev(count=0) == 0 and host(count=0) == 0
    assert e.timer_end()[1] == 0, "the checks come before any launch"
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all() and (d_both.cpu().numpy().view(np.uint32) == FILL).all() and (out_host == FILL).all()
    # accepted exactly at each limit: 16 steps with the last entry of the key and every step adding (SHAPES[3] mixes them); d_out right behind
    # the rows does not overlap them; exactly in place
    entry16, add16 = [5] * 16, [1] * 16
    assert np.array_equal(e.trlwe_auto_batch(key, w.x[:2], entry16, add16), w.oracle(A.REFERENCE, "k6", entry16, add16, 2))
    d_both[:3].copy_(gk.to_device(w.x[:3], np.uint32))
    e.trlwe_auto_batch_dev(key, d_both[:3], d_both[3:], 3, [1])
    e.trlwe_auto_batch_dev(key, d_both[:3], d_both[:3], 3, [1])
    e.sync()
    assert np.array_equal(d_both[3:].cpu().numpy().view(np.uint32), w.oracle(A.REFERENCE, "k6", [1], None, 3))
    assert np.array_equal(d_both[:3].cpu().numpy().view(np.uint32), w.oracle(A.REFERENCE, "k6", [1], None, 3))
    # ... and a key's creation at its limit: 64 exponents, t = 2N - 1 among them, the LAST entry used in a step
    t64 = [2 * N - 1 - 2 * k for k in range(64)]
    words64 = R.trlwe_ksk_keygen(w.rp, w.keyB, w.keyB, t64, seed=0xA79)
    with e.trlwe_switch_key(words64, t64) as key64:
        assert key64.n == 64
        want64 = A.program(w.p, w.plan, A.spectra(w.p, w.plan, words64), t64, w.x[:2], [63, 0], [0, 1], A.REFERENCE)
        assert np.array_equal(e.trlwe_auto_batch(key64, w.x[:2], [63, 0], [0, 1]), want64)
    # a key of another context, and a key whose context is gone
    other = R.Engine(w.rp, 0)
    key_other = other.trlwe_switch_key(w.words["k1"], w.t["k1"])
    with pytest.raises(R.RtfheError) as ei:
        e._ck(dev(key=key_other))
    assert ei.value.code == R._ffi.ERR_INVALID and "another context" in str(ei.value)
    other.close()
    rc = dev(key=key_other)
    assert rc == R._ffi.ERR_STATE and b"destroyed" in e.L.rtfhe_last_error(e.h)
    key_other.close()            # rtfhe_trlwe_ksk_destroy still frees the handle
    e.sync()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all()


def test_a_destroyed_context_and_a_destroyed_key():
    """the context destroyed under a live key: both forms, called on another live context, return RTFHE_ERR_STATE and touch nothing, and
    rtfhe_trlwe_ksk_destroy still frees the handle; a key destroyed before its context leaves the context and its other keys working"""
    import torch
    import rustfhe_amd as R
    N = 1024
    rp = R.Params(n=SMALL_N[N], N=N)
    e = R.Engine(rp, 0)
    zero = np.zeros((1, rp.l, 2, N), np.uint32)
    key = e.trlwe_switch_key(zero, [3])
    x = O.rows_with_edges(0xA90, N, 1)
    out = np.full((1, 2, N), FILL, np.uint32)
    d_x = gk.to_device(x, np.uint32)
    d_out = torch.full((1, 2, N), FILL, dtype=torch.int32, device="cuda")
    ent = i32([0])
    e.close()
    live = R.Engine(rp, 0)
    try:
        L = live.L
        assert L.rtfhe_trlwe_auto_batch(live.h, key.h, ent.ctypes.data, None, 1, x.ctypes.data, out.ctypes.data, 1) == R._ffi.ERR_STATE
        assert b"destroyed" in L.rtfhe_last_error(live.h)
        assert L.rtfhe_trlwe_auto_batch_dev(live.h, key.h, ent.ctypes.data, None, 1, d_x.data_ptr(), d_out.data_ptr(), 1, None) == R._ffi.ERR_STATE
        live.sync()
        key.close()
        torch.cuda.synchronize()
        assert (out == FILL).all() and (d_out.cpu().numpy().view(np.uint32) == FILL).all()
        # a key destroyed first: the other key of the context still runs (the zero key: a step is (sigma_t b, 0))
        first, second = live.trlwe_switch_key(zero, [3]), live.trlwe_switch_key(zero, [5])
        first.close()
        got = live.trlwe_auto_batch(second, x, [0])
        assert np.array_equal(got[:, 0], A.automorphism(x[:, 0], 5)) and (got[:, 1] == 0).all()
        second.close()
    finally:
        live.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_exact_backends_refuse_and_a_two_entry_context_runs(worlds, N):
    w, R = worlds(N), worlds(N).R
    count, which, entry, add, _ = SHAPES[3]
    want = w.oracle(A.REFERENCE, which, entry, add, count)
    e = R.Engine(w.rp, 0)            # nothing loaded
    try:
        with e.trlwe_switch_key(w.words[which], w.t[which]) as key:
            for backend in (R._ffi.BACKEND_NTT_EXACT, R._ffi.BACKEND_FFT_SPLIT_EXACT):
                e.set_backend(backend)
                for call in (lambda: e.trlwe_auto_batch(key, w.x[:count], entry, add), lambda: _dev(e, key, w.x[:count], entry, add)):
                    with pytest.raises(R.RtfheError) as ei:
                        call()
                    assert ei.value.code == R._ffi.ERR_INVALID and "mirror" in str(ei.value)
            e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
            assert np.array_equal(e.trlwe_auto_batch(key, w.x[:count], entry, add), want)      # the context works afterwards
    finally:
        e.close()
    multi = R.Engine(w.rp, devices=[0, 0])
    try:
        assert multi.device_count() == 2
        with multi.trlwe_switch_key(w.words[which], w.t[which]) as key:
            assert np.array_equal(multi.trlwe_auto_batch(key, w.x[:count], entry, add), want)
            assert np.array_equal(_dev(multi, key, w.x[:count], entry, add), want)
            assert np.array_equal(_dev(multi, key, w.x[:count], entry, add, in_place=True), want)
    finally:
        multi.close()
