"""GPU: seeded ciphertexts (rtfhe_seeded_expand_dev and the *_seeded upload calls; k_seeded_expand).  The device expansion word for word against
the host expansion, itself held to its numpy restatement by tests/test_seeded_host.py (tests/seeded_oracle.py), at both rings, every group and the
edge row numbers, behind a canary; refusals before any launch; capture first thing on a fresh stream; and every seeded upload call against its
unseeded twin fed the host expansion of the same object: selector sets (tree words in both leveled modes, update of a middle range), encrypted
tables (rows read back, one PBS), the bootstrapping key (spectra, bootstraps on the mirror and an exact backend, a two-entry context), the
packing key (pack words); handle lifetimes; the example.  Contexts are small: n = 8."""
import numpy as np
import pytest

import gpu_kit as gk
from kit import load_example, random_words

pytestmark = pytest.mark.gpu

M64 = 1 << 64
SMALL = 8
SHAPES = [(1, 1), (1, 5), (1, 7), (6, 6), (6, 18)]       # (group, rows): a partial last workgroup, a row that straddles a workgroup


def _R():
    import rustfhe_amd as R
    return R


@pytest.fixture(scope="module")
def worlds():
    """one keyless context per ring"""
    R = _R()
    w = gk.Worlds(lambda N: R.Engine(R.Params(n=SMALL, N=N), 0))
    yield w
    w.close()


def _first_rows(rows):
    return (0, (1 << 32) - 2, M64 - rows)        # the low word carries between rows; the last rows there are


@pytest.mark.parametrize("N", [1024, 2048])      # a wave per row, two waves per row
def test_device_expansion_equals_the_host_expansion_word_for_word(worlds, N):
    import torch
    R = _R()
    e = worlds(N)
    rng = np.random.default_rng(N)
    st = torch.cuda.current_stream().cuda_stream
    for group, rows in SHAPES:
        b = random_words(rng, (rows, N))
        d_b = gk.to_device(b, np.uint32)
        for first_row in _first_rows(rows):
            seed = random_words(rng, 8)
            d_out = gk.guarded_out(2 * rows * N)
            e.timer_begin(st)
            e.seeded_expand_dev(seed, d_b, group, d_out, rows, first_row, st)
            assert e.timer_end(st)[1] == 1, "one launch writes the whole object"
            got = gk.read_guarded(d_out, 2 * rows * N)
            want = R.seeded_expand(e.p, seed, b, group, first_row=first_row)
            assert np.array_equal(got, want.reshape(-1)), (group, rows, first_row)
            assert np.array_equal(gk.words_of(d_b).reshape(rows, N), b), "d_b stays as it is"


def test_refusals_come_before_any_launch(worlds):
    import torch
    R = _R()
    N = 1024
    e = worlds(N)
    seed = np.arange(8, dtype=np.uint32)
    d_b = gk.to_device(np.zeros((6, N), np.uint32), np.uint32)
    d_out = gk.guarded_out(12 * N)
    d_both = gk.to_device(np.full(18 * N, gk.FILL, np.uint32), np.uint32)      # b and the output in one allocation
    b, out = d_b.data_ptr(), d_out.data_ptr()
    e.timer_begin()

    def dev(h=e.h, sd=seed.ctypes.data, first_row=0, b=b, group=6, out=out, rows=6):
        return e.L.rtfhe_seeded_expand_dev(h, sd, first_row, b, group, out, rows, None)

    both = d_both.data_ptr()
    for kw, word in (({"first_row": M64 - 5}, "pass 2^64"), ({"rows": 5}, "not a multiple"), ({"group": 4}, "not a multiple"), ({"group": 0}, "group = 0"),
                     ({"sd": None}, "null"), ({"b": None}, "null"), ({"out": None}, "null"), ({"b": b + 4}, "aligned"),
                     ({"b": both, "out": both + 6 * N * 4 - 16}, "overlaps"), ({"b": both + 64, "out": both}, "overlaps"),
                     ({"b": seed.ctypes.data & ~15}, "device pointers")):
        with pytest.raises(R.RtfheError) as ei:
            e._ck(dev(**kw))
        assert ei.value.code == R._ffi.ERR_INVALID and word in str(ei.value), (word, str(ei.value))
    assert dev(h=None) == R._ffi.ERR_INVALID
    assert dev(rows=0) == 0
    assert dev(b=d_both.data_ptr(), out=d_both.data_ptr() + 6 * N * 4, first_row=M64 - 6) == 0, "out right behind b, the last six rows: accepted"
    assert e.timer_end()[1] == 1, "the refused calls and the empty one launched nothing"
    e.sync()
    assert (gk.read_guarded(d_out, 12 * N) == gk.FILL).all()


@pytest.mark.parametrize("N", [1024, 2048])
def test_capture_first_thing_on_a_fresh_engine_and_stream(N):
    """no eager call before the capture, on a stream nothing has run on; the seed is baked into the graph"""
    import torch
    R = _R()
    rng = np.random.default_rng(7 + N)
    seed, b = random_words(rng, 8), random_words(rng, (12, N))
    e = R.Engine(R.Params(n=SMALL, N=N), 0)
    try:
        want = R.seeded_expand(e.p, seed, b, 6, first_row=(1 << 32) - 5)
        s = torch.cuda.Stream()
        d_b, d_out = gk.to_device(b, np.uint32), gk.guarded_out(24 * N)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                e.seeded_expand_dev(seed.copy(), d_b, 6, d_out, 12, (1 << 32) - 5, s.cuda_stream)
            for _ in range(2):
                d_out.copy_(gk.guarded_out(24 * N))
                g.replay()
                torch.cuda.synchronize()
                assert np.array_equal(gk.read_guarded(d_out, 24 * N), want.reshape(-1))
        e.sync(s.cuda_stream)
        del g
    finally:
        e.close()


@pytest.mark.parametrize("N", [1024, 2048])
def test_seeded_selectors_give_the_unseeded_sets_tree_words(worlds, N):
    """depth 2, 2 lookups, both leveled modes; then selectors [1, 3) rewritten on both sets"""
    R = _R()
    e = worlds(N)
    p = e.p
    rng = np.random.default_rng(N + 1)
    key1 = rng.integers(0, 2, N).astype(np.int32)
    rows = R.encrypt_lut(p, key1, R.encode_msgs(rng.integers(0, 4, (4, N)), 2), seed=3)
    seed, b = R.encrypt_selectors_seeded(p, key1, [1, 0, 0, 1], noise_seed=4, seed=random_words(rng, 8), first_row=(1 << 32) - 7)
    seed2, b2 = R.encrypt_selectors_seeded(p, key1, [0, 1], noise_seed=5, seed=random_words(rng, 8), first_row=M64 - 12)
    full = R.seeded_expand(p, seed, b, 2 * p.l, first_row=(1 << 32) - 7)
    full2 = R.seeded_expand(p, seed2, b2, 2 * p.l, first_row=M64 - 12)
    with e.lut_encrypted(rows) as table, e.selectors_seeded(seed, b, (1 << 32) - 7) as s_sel, e.selectors(full) as u_sel:
        assert s_sel.n_sel == u_sel.n_sel == 4
        try:
            for stage in ("created", "updated"):
                for mode in (R._ffi.DECOMP_REFERENCE, R._ffi.DECOMP_ROUNDED):
                    e.set_leveled_decomposition(mode)
                    got, want = e.cmux_tree_batch(s_sel, table, 2, 2), e.cmux_tree_batch(u_sel, table, 2, 2)
                    assert np.array_equal(got, want), (stage, mode)
                if stage == "created":
                    first = e.cmux_tree_batch(u_sel, table, 2, 2)
                    s_sel.update_seeded(seed2, b2, first=1, first_row=M64 - 12)
                    u_sel.update(full2, first=1)
                    assert not np.array_equal(e.cmux_tree_batch(u_sel, table, 2, 2), first), "the update changed lookup words"
        finally:
            e.set_leveled_decomposition(R._ffi.DECOMP_REFERENCE)
        with pytest.raises(R.RtfheError) as ei:
            s_sel.update_seeded(seed2, b2, first=3)
        assert ei.value.code == R._ffi.ERR_INVALID and "outside the set" in str(ei.value)
        with pytest.raises(R.RtfheError) as ei:
            s_sel.update_seeded(seed2, b2, first=1, first_row=M64 - 11)
        assert ei.value.code == R._ffi.ERR_INVALID and "pass 2^64" in str(ei.value)


@pytest.fixture(scope="module")
def keyed():
    """n = 8 at N = 1024: the keys, a seeded bootstrapping key and its host expansion, shared and read-only"""
    R = _R()
    p = R.Params(n=SMALL)
    key0, key1, bk, ksk = R.keygen(p, 0x5EED)
    seed, b = R.encrypt_selectors_seeded(p, key1, key0, noise_seed=6, seed=np.arange(8, dtype=np.uint32) * 0x01010101, first_row=(1 << 32) - 20)
    full = R.seeded_expand(p, seed, b, 2 * p.l, first_row=(1 << 32) - 20)
    for a in (key0, key1, bk, ksk, seed, b, full):
        a.setflags(write=False)
    return p, key0, key1, bk, ksk, seed, b, full


def test_seeded_table_reads_back_as_the_host_expansion_and_bootstraps_alike(keyed):
    import torch
    R = _R()
    p, key0, key1, bk, ksk, _, _, _ = keyed
    tv = np.stack([R.lut_polynomial(lambda m: (m + 1) % 4, p.N, 2), R.lut_polynomial(lambda m: 3 - m, p.N, 2), R.lut_polynomial(lambda m: m, p.N, 2)])
    seed, b = R.encrypt_lut_seeded(p, key1, tv, noise_seed=8, seed=np.arange(8) + 100, first_row=M64 - 3)
    full = R.seeded_expand(p, seed, b, 1, first_row=M64 - 3).reshape(3, 2, p.N)
    cts = R.encrypt_torus(p, key0, R.encode_msgs([0, 1, 2, 3], 2), seed=9)
    e = R.Engine(p, 0)
    try:
        e.load_bk_torus(bk)
        e.load_ksk(ksk)
        with e.lut_encrypted_seeded(seed, b, M64 - 3) as s_lut, e.lut_encrypted(full) as u_lut:
            assert s_lut.encrypted and s_lut.n_lut == 3
            d_rows = gk.guarded_out(3 * 2 * p.N)
            s_lut.read_dev(d_rows, 0, 3)
            torch.cuda.synchronize()
            assert np.array_equal(gk.read_guarded(d_rows, 3 * 2 * p.N), full.reshape(-1))
            idx = [2, 0, 1, 1]
            got, want = e.pbs_batch(s_lut, cts, idx), e.pbs_batch(u_lut, cts, idx)
            assert np.array_equal(got, want)
    finally:
        e.close()


def _bootstraps(R, e, cts):
    """the four words a key is compared by: bootstraps on the mirror backend, gates on an exact one, the mirror restored"""
    out = [e.bootstrap_batch(cts)]
    e.set_backend(R._ffi.BACKEND_NTT_EXACT)
    out.append(e.gate_batch(R.NAND, cts, cts[::-1]))
    e.set_backend(R._ffi.BACKEND_FFT64_MIRROR)
    return out


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one entry", "two entries"])
def test_seeded_bootstrapping_key_is_the_unseeded_load_of_its_expansion(keyed, devices):
    """... also over a key loaded before, whose derived exact-backend key must follow"""
    R = _R()
    p, key0, _, bk, ksk, seed, b, full = keyed
    cts = R.encrypt_bits(p, key0, [0, 1, 1, 0], 10)
    kw = {} if devices is None else {"devices": devices}
    s_eng, u_eng = gk.engine(R, p, bk, ksk, **kw), gk.engine(R, p, bk, ksk, **kw)
    try:
        before = _bootstraps(R, s_eng, cts)               # the exact backend's key form exists now
        s_eng.load_bk_seeded(seed, b, (1 << 32) - 20)
        u_eng.load_bk_torus(full)
        assert s_eng.export_bk_fft().tobytes() == u_eng.export_bk_fft().tobytes()
        got, want = _bootstraps(R, s_eng, cts), _bootstraps(R, u_eng, cts)
        for g, w, old in zip(got, want, before):
            assert np.array_equal(g, w) and not np.array_equal(g, old)
        assert list(R.decrypt_bits(p, key0, got[1])) == [1, 0, 0, 1], "the seeded key is a bootstrapping key of key0"
        assert s_eng.memory_bytes() >= u_eng.memory_bytes()
        with pytest.raises(R.RtfheError) as ei:
            s_eng.load_bk_seeded(seed, b, M64 - 6 * SMALL + 1)
        assert ei.value.code == R._ffi.ERR_INVALID and "pass 2^64" in str(ei.value)
    finally:
        s_eng.close()
        u_eng.close()


def test_seeded_packing_key_gives_the_unseeded_keys_pack_words():
    R = _R()
    p = R.Params(n=4)
    key0, key1, _, _ = R.keygen(p, 0xA11, want_bk=False, want_ksk=False)
    seed, b = R.packing_keygen_seeded(p, key0, key1, noise_seed=11, seed=np.arange(8) + 7, first_row=(1 << 32) - 50)
    full = R.seeded_expand(p, seed, b, 1, first_row=(1 << 32) - 50)
    msgs = [0, 1, 2, 3]
    tlwe = R.encrypt_torus(p, key0, R.encode_msgs(msgs, 2), seed=12)
    e = R.Engine(p, 0)
    try:
        with e.packing_key_seeded(seed, b, (1 << 32) - 50) as s_pk, e.packing_key(full) as u_pk:
            got, want = e.pack_batch(s_pk, tlwe, 4), e.pack_batch(u_pk, tlwe, 4)
            assert got.shape == (1, 2, p.N) and np.array_equal(got, want)
    finally:
        e.close()


def test_seeded_handles_follow_the_twins_lifetime_rules():
    """a seeded handle of another context, of a destroyed one and closed early, through one _dev call per kind (tests/test_gpu_handle_lifetimes.py)"""
    import torch
    R = _R()
    N = 1024
    p = R.Params(n=4, N=N)
    rng = np.random.default_rng(5)
    seed = random_words(rng, 8)
    mine, other = R.Engine(p, 0), R.Engine(p, 0)
    try:
        L = mine.L
        make = {"table": lambda eng: eng.lut_encrypted_seeded(seed, random_words(rng, (2, N))),
                "selector set": lambda eng: eng.selectors_seeded(seed, random_words(rng, (1, 2 * p.l, N))),
                "packing key": lambda eng: eng.packing_key_seeded(seed, random_words(rng, R.engine.packing_key_words(p) // 2))}
        d_tlwe = torch.zeros((1, p.n + 1), dtype=torch.int32, device="cuda")
        d_row = torch.zeros((1, 2, N), dtype=torch.int32, device="cuda")
        d_out = gk.guarded_out(2 * N)
        tlwe, row, out = d_tlwe.data_ptr(), d_row.data_ptr(), d_out.data_ptr()
        call = {"table": lambda h: L.rtfhe_pbs_batch_dev(mine.h, h, None, tlwe, out, 1, None),
                "selector set": lambda h: L.rtfhe_trgsw_rotate_batch_dev(mine.h, h, None, 1, None, row, out, 1, None),
                "packing key": lambda h: L.rtfhe_pack_batch_dev(mine.h, h, tlwe, 1, None, 1, out, 1, None)}
        late = {kind: make[kind](other) for kind in make}
        mine.timer_begin()
        for kind in make:
            with pytest.raises(R.RtfheError) as ei:
                mine._ck(call[kind](late[kind].h))
            assert ei.value.code == R._ffi.ERR_INVALID and "another context" in str(ei.value), kind
        other.close()
        for kind in make:
            with pytest.raises(R.RtfheError) as ei:
                mine._ck(call[kind](late[kind].h))
            assert ei.value.code == R._ffi.ERR_STATE and "destroyed" in str(ei.value), kind
        with pytest.raises(R.RtfheError) as ei:
            late["selector set"].update_seeded(seed, np.zeros((1, 2 * p.l, N), np.uint32))
        assert ei.value.code == R._ffi.ERR_STATE
        assert mine.timer_end()[1] == 0, "a refused call launched something"
        mine.sync()
        assert (gk.read_guarded(d_out, 2 * N) == gk.FILL).all()
        for kind in make:
            late[kind].close()
            late[kind].close()
            first = make[kind](mine)          # closed before its context: the context goes on
            first.close()
            make[kind](mine).close()
        mine.sync()
    finally:
        other.close()
        mine.close()


def test_seeded_leveled_lut_example(keyed):
    """examples/seeded_leveled_lut.py on a small context (n = 8) that holds the key-switching key only: 6 twelve-bit lookups, all right, and half
    the bytes shipped"""
    R = _R()
    p, key0, key1, _, ksk, _, _, _ = keyed
    ex = load_example("seeded_leveled_lut")
    e = R.Engine(p, 0)
    try:
        e.load_ksk(ksk)
        addr, got, want = ex.run(e, key0, key1, 6, seed=0x1E7E1)
        assert len(addr) == 6 and np.array_equal(got, want)
        full, seeded = ex.shipped_bytes(p, 6)
        assert seeded == full // 2 + 64
    finally:
        e.close()
