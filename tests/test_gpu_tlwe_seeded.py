"""GPU: seeded lvl0 ciphertexts and the seeded key-switching key (rtfhe_tlwe_seeded_expand_dev, rtfhe_load_ksk_seeded; k_tlwe_seeded_expand).
The device expansion word for word against the host expansion, itself held to its numpy restatement by tests/test_tlwe_seeded_host.py
(tests/tlwe_seeded_oracle.py), at every n around a ChaCha20 block's end and the ends of the supported range, several workgroups with a partial
last one, the edge row numbers, behind a canary and as a range of rows inside a wire table whose rows start at any word; refusals before any
launch; capture first thing on a fresh stream; gates on seeded inputs; the seeded key against the unseeded load of its host expansion on both
key-switch routes; the example."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import load_example, random_words

pytestmark = pytest.mark.gpu

M64 = 1 << 64


def _R():
    import rustfhe_amd as R
    return R


@pytest.fixture(scope="module")
def worlds():
    """one keyless context per TLWE dimension"""
    R = _R()
    w = gk.Worlds(lambda n: R.Engine(R.Params(n=n), 0))
    yield w
    w.close()


def _first_rows(rows):
    return (0, (1 << 32) - 2, M64 - rows)        # the carry into state word 15 between rows; the last rows there are


@pytest.mark.parametrize("n", [1, 15, 16, 17, 635, 766, 767])
def test_device_expansion_equals_the_host_expansion_word_for_word(worlds, n):
    """300 rows at n = 767 are 14,400 blocks: 57 workgroups, the last one a quarter full; 67 rows at n = 1 end inside the second wave"""
    import torch
    R = _R()
    e = worlds(n)
    rng = np.random.default_rng(n)
    st = torch.cuda.current_stream().cuda_stream
    for rows in (1, 5, 67, 300):
        b = random_words(rng, rows)
        d_b = gk.to_device(b, np.uint32)
        for first_row in _first_rows(rows):
            seed = random_words(rng, 8)
            d_out = gk.guarded_out(rows * (n + 1))
            e.timer_begin(st)
            e.tlwe_seeded_expand_dev(seed, d_b, d_out, rows, first_row, st)
            assert e.timer_end(st)[1] == 1, "one launch writes the whole object"
            got = gk.read_guarded(d_out, rows * (n + 1))
            want = R.tlwe_seeded_expand(e.p, seed, b, first_row=first_row)
            assert np.array_equal(got, want.reshape(-1)), (rows, first_row)
            assert np.array_equal(gk.words_of(d_b), b), "d_b stays as it is"


@pytest.mark.parametrize("n", [634, 635])
def test_expansion_into_rows_of_a_wire_table(worlds, n):
    """rows 3 .. 7 of a 12-row table that starts one word into its allocation: no row starts at a multiple of 4 words; its neighbours stay"""
    import torch
    R = _R()
    e = worlds(n)
    rng = np.random.default_rng(n)
    w = n + 1
    seed, b = random_words(rng, 8), random_words(rng, 5)
    before = random_words(rng, 1 + 12 * w)
    d_table = gk.guarded_out(1 + 12 * w, init=before)
    d_b = gk.to_device(b, np.uint32)
    at = 1 + 3 * w
    assert at % 4 and (at + w) % 4
    e.tlwe_seeded_expand_dev(seed, d_b, d_table.data_ptr() + 4 * at, 5, (1 << 32) - 3)
    torch.cuda.synchronize()
    got = gk.read_guarded(d_table, 1 + 12 * w)
    want = before.copy()
    want[at:at + 5 * w] = R.tlwe_seeded_expand(e.p, seed, b, first_row=(1 << 32) - 3).reshape(-1)
    assert np.array_equal(got, want)


def test_refusals_come_before_any_launch(worlds):
    R = _R()
    n = 635
    e = worlds(n)
    seed = np.arange(8, dtype=np.uint32)
    d_b = gk.to_device(np.zeros(6, np.uint32), np.uint32)
    d_out = gk.guarded_out(6 * (n + 1))
    d_both = gk.to_device(np.full(6 + 6 * (n + 1), gk.FILL, np.uint32), np.uint32)      # b and the output in one allocation
    b, out, both = d_b.data_ptr(), d_out.data_ptr(), d_both.data_ptr()
    e.timer_begin()

    def dev(h=e.h, sd=seed.ctypes.data, first_row=0, b=b, out=out, rows=6):
        return e.L.rtfhe_tlwe_seeded_expand_dev(h, sd, first_row, b, out, rows, None)

    for kw, word in (({"sd": None}, "null"), ({"b": None}, "null"), ({"out": None}, "null"), ({"rows": 0}, "rows = 0"),
                     ({"rows": 0x7fffffff // 40 + 1}, "too large"), ({"first_row": M64 - 5}, "pass 2^64"),
                     ({"b": both, "out": both + 20}, "overlaps"), ({"b": both + 6 * (n + 1) * 4 - 4, "out": both}, "overlaps"),
                     ({"b": b + 2}, "aligned"), ({"out": out + 1}, "aligned"), ({"b": seed.ctypes.data & ~3}, "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(dev(**kw))
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (word, str(ei.value))
    assert dev(h=None) == R._ffi.ERR_INVALID
    assert e.timer_end()[1] == 0, "a refused call launched something"
    e.timer_begin()
    assert dev(b=both, out=both + 24, first_row=M64 - 6) == 0, "out right behind b, 4-byte aligned only, the last six rows: accepted"
    assert e.timer_end()[1] == 1
    e.sync()
    assert (gk.read_guarded(d_out, 6 * (n + 1)) == gk.FILL).all()


@pytest.mark.parametrize("n", [17, 635])
def test_capture_first_thing_on_a_fresh_engine_and_stream(n):
    """no eager call before the capture, on a stream nothing has run on; the seed is baked into the graph"""
    import torch
    R = _R()
    rng = np.random.default_rng(7 + n)
    seed, b = random_words(rng, 8), random_words(rng, 12)
    e = R.Engine(R.Params(n=n), 0)
    try:
        want = R.tlwe_seeded_expand(e.p, seed, b, first_row=(1 << 32) - 5)
        s = torch.cuda.Stream()
        d_b, d_out = gk.to_device(b, np.uint32), gk.guarded_out(12 * (n + 1))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                e.tlwe_seeded_expand_dev(seed.copy(), d_b, d_out, 12, (1 << 32) - 5, s.cuda_stream)
            for _ in range(2):
                d_out.copy_(gk.guarded_out(12 * (n + 1)))
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.read_guarded(d_out, 12 * (n + 1)), want.reshape(-1))
        e.sync(s.cuda_stream)
        d_out.copy_(gk.guarded_out(12 * (n + 1)))
        e.tlwe_seeded_expand_dev(seed, d_b, d_out, 12, (1 << 32) - 5)
        torch.cuda.synchronize()
        assert np.array_equal(gk.read_guarded(d_out, 12 * (n + 1)), want.reshape(-1)), "the replay equals the eager result"
        del g
    finally:
        e.close()


def test_gates_on_seeded_inputs(engine, keys):
    """N = 1024, n = 635, the golden key set: 8 pairs of seeded bits, uploaded and expanded on the device, through gate_batch_dev"""
    import torch
    R = _R()
    p = engine.p
    rng = np.random.default_rng(635)
    x, y = rng.integers(0, 2, 8).astype(np.uint8), rng.integers(0, 2, 8).astype(np.uint8)
    sx, bx = R.encrypt_bits_seeded(p, keys.key0, x)
    sy, by = R.encrypt_bits_seeded(p, keys.key0, y, noise_seed=3, seed=random_words(rng, 8), first_row=(1 << 32) - 4)
    d_x, d_y = engine.upload_tlwe_seeded(sx, bx), engine.upload_tlwe_seeded(sy, by, first_row=(1 << 32) - 4)
    assert d_x.shape == (8, p.n + 1) and d_x.dtype == torch.int32
    hx, hy = R.tlwe_seeded_expand(p, sx, bx), R.tlwe_seeded_expand(p, sy, by, first_row=(1 << 32) - 4)
    torch.cuda.synchronize()
    assert np.array_equal(gk.words_of(d_x), hx) and np.array_equal(gk.words_of(d_y), hy)
    d_out = gk.guarded_out(8 * (p.n + 1))
    engine.gate_batch_dev(R.NAND, d_x, d_y, d_out, 8, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = gk.read_guarded(d_out, 8 * (p.n + 1)).reshape(8, p.n + 1)
    assert np.array_equal(got, engine.gate_batch(R.NAND, hx, hy))
    assert np.array_equal(R.decrypt_bits(p, keys.key0, got), 1 - (x & y))


@pytest.mark.parametrize("route", [None, {"RTFHE_KS_MM_MIN": "0"}], ids=gk.env_id)
@pytest.mark.parametrize("N,n,devices", [(1024, 635, None), (1024, 635, [0, 0]), (1024, 1, None), (1024, 767, [0, 0]), (2048, 635, None)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_seeded_key_switching_key_is_the_unseeded_load_of_its_expansion(monkeypatch, N, n, devices, route):
    """... over a key loaded before.  key_switch_batch reads the pre-summed rows; trlwe_extract_batch the i8 matrix form on the default route
    (k_key_switch_mm) and the rows again under RTFHE_KS_MM_MIN=0 (k_key_switch_ext)"""
    R = _R()
    p = R.Params(n=n, N=N)
    key0, key1, _, old = R.keygen(p, 0x5EED + n, want_bk=False, want_ksk=True)
    first_row = (1 << 32) - 20
    seed, b = R.ksk_keygen_seeded(p, key0, key1, noise_seed=6, seed=np.arange(8, dtype=np.uint32) * 0x01010101, first_row=first_row)
    full = R.tlwe_seeded_expand(p, seed, b, first_row=first_row)
    rng = np.random.default_rng(N + n)
    t1 = random_words(rng, (9, N + 1))
    t1[1, :N] = 0
    t1[2, :N] = 0xFFFFFFFF
    rows = random_words(rng, (2, 2, N))
    kw = {} if devices is None else {"devices": devices}

    def words(e):
        return e.key_switch_batch(t1), e.trlwe_extract_batch(rows, 3, [0, 1, N - 1])

    if route:
        for k, v in route.items():
            monkeypatch.setenv(k, v)
    s_eng, u_eng = (R.Engine(p, 0, **kw) if devices is None else R.Engine(p, **kw) for _ in range(2))
    if route:
        for k in route:
            monkeypatch.delenv(k)
    try:
        s_eng.load_ksk(old)
        u_eng.load_ksk(old)
        before = words(s_eng)
        s_eng.load_ksk_seeded(seed, b, first_row)
        u_eng.load_ksk(full)
        for g, w, o in zip(words(s_eng), words(u_eng), before):
            assert np.array_equal(g, w) and not np.array_equal(g, o)
        assert s_eng.memory_bytes() >= u_eng.memory_bytes()
        with pytest.raises(R.RtfheError) as ei:
            s_eng.load_ksk_seeded(seed, b, M64 - b.size + 1)
        assert ei.value.code == R._ffi.ERR_INVALID and "pass 2^64" in str(ei.value)
        assert np.array_equal(words(s_eng)[0], words(u_eng)[0]), "a refused load leaves the key as it was"
    finally:
        s_eng.close()
        u_eng.close()


def test_seeded_gates_example():
    """examples/seeded_gates.py on a small context (n = 8): two replicas of the 8-bit adder on seeded inputs under seeded keys"""
    R = _R()
    ex = load_example("seeded_gates")
    got, want = ex.run(R.Params(n=8), 2, seed=0x6A7E5)
    assert np.array_equal(got, want)
    full, seeded = ex.shipped_bytes(R.Params(), 4)
    assert full == (64 + 24576) * 636 * 4 + R.Params().bk_words * 4 and seeded == (64 + 24576) * 4 + R.Params().bk_words * 2 + 96
