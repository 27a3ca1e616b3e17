"""CPU: the host-only plan units at sizes past 2^32 and 2^33 bytes ("Address arithmetic"), and the arithmetic half of
tests/large_kit.py.  A plan function never dereferences its buffer arguments (rows_overlap compares addresses), so it is driven through ctypes
with made-up addresses: for every family that compares its buffers -- extract, compress (both forms), plain, trgsw_mac, dense, seeded,
tlwe_seeded -- an output directly behind (and directly before) an input or output of 4.3 GB and of the largest size the family's 2^31-item
rule admits up to 17 GB is accepted, an output that shares only the other buffer's last word is refused with the family's "overlaps" message,
a buffer that starts inside the last row of a far larger one is refused, and the 2^31-item rule holds exactly at its limit, where the byte
sizes are terabytes.  pack and cmux_net compare no addresses: their item rules alone.  The same cases run under UndefinedBehaviorSanitizer in
the stand-alone walks of tests/c/ (sanitize_kit.h: large_cases, large_limit)."""
import ctypes as C

import numpy as np
import pytest

import large_kit as lk

INV = -1
BASE = 0x7F0000000000            # where the made-up buffers start: 127 TiB, far below 2^63
FAR = 0x100000000000             # 16 TiB on


@pytest.fixture(scope="module")
def L():
    import rustfhe_amd as R
    lib = R.load()
    vp, i32, sz, cp = C.c_void_p, C.c_int32, C.c_size_t, C.c_char_p
    for name, args in {
        "rtfhe_extract_plan": [i32, i32, vp, i32, sz, vp, vp, sz, vp, cp, sz],
        "rtfhe_pack_plan": [i32, i32, vp, i32, sz, vp, vp, vp, cp, sz],
        "rtfhe_tlwe_compress_plan": [i32, i32, i32, sz, vp, vp, cp, sz],
        "rtfhe_trlwe_compress_plan": [i32, i32, i32, i32, vp, i32, sz, vp, vp, vp, cp, sz],
        "rtfhe_plain_plan": [i32, i32, C.c_int64, i32, i32, vp, i32, i32, vp, sz, vp, vp, cp, sz],
        "rtfhe_trgsw_mac_plan": [i32, i32, i32, i32, vp, i32, i32, vp, sz, vp, vp, cp, sz],
        "rtfhe_dense_plan": [i32, i32, i32, sz, vp, vp, cp, sz],
        "rtfhe_seeded_plan": [i32, i32, vp, C.c_uint64, vp, i32, vp, sz, cp, sz],
        "rtfhe_tlwe_seeded_plan": [i32, i32, vp, C.c_uint64, vp, vp, sz, cp, sz],
    }.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, args
    return lib


class Family:
    """A plan function over (items, in, out): call(L, items, a, b) -> rc with the message left in self.msg; in_bytes / out_bytes of `items`;
    sizes: the item counts that make the large side 4.3 GB and the largest the item rule admits up to 17 GB; limit: the largest accepted
    item count and the word its refusal one above carries; large_out: the OUTPUT is the side that grows (the input cannot reach 2^32)."""

    def __init__(self, name, call, in_bytes, out_bytes, sizes, limit, limit_word, overlap_word, last=4, large_out=False):
        self.name, self._call, self.in_bytes, self.out_bytes = name, call, in_bytes, out_bytes
        self.sizes, self.limit, self.limit_word, self.overlap_word, self.last, self.large_out = sizes, limit, limit_word, overlap_word, last, large_out
        self.msg = ""

    def __call__(self, L, items, a, b):
        err = C.create_string_buffer(b"x" * 255, 256)
        rc = self._call(L, items, a, b, err, len(err))
        self.msg = err.value.decode()
        return rc


_idx = (C.c_int32 * 1)()
_seed = (C.c_uint32 * 8)()
N2, n767 = 2048, 767
FAMILIES = [
    Family("extract", lambda L, c, a, b, e, n: L.rtfhe_extract_plan(N2, 1, None, 1, c, a, b, N2 + 1, _idx, e, n),
           lambda c: c * 8 * N2, lambda c: c * 4 * (N2 + 1), [(1 << 18) + 3, (1 << 20) + 3], (1 << 31) - 1, "count * P", "overlaps the TRLWE rows"),
    Family("trlwe_compress", lambda L, c, a, b, e, n: L.rtfhe_trlwe_compress_plan(0, N2, 10, 1, None, 1, c, a, b, _idx, e, n),
           lambda c: c * 8 * N2, lambda c: c * 4 * lk_words(N2 + 1, 10), [(1 << 18) + 3, ((1 << 31) - 1) // (N2 + 1)], ((1 << 31) - 1) // (N2 + 1), "count * L",
           "overlaps the input rows"),
    Family("tlwe_compress", lambda L, c, a, b, e, n: L.rtfhe_tlwe_compress_plan(0, n767, 10, c, a, b, e, n),
           lambda c: c * 4 * (n767 + 1), lambda c: c * 4 * lk_words(n767 + 1, 10), [1398102 + 3, ((1 << 31) - 1) // (n767 + 1)], ((1 << 31) - 1) // (n767 + 1),
           "count * L", "overlaps the input rows"),
    # the two sums of products: x has `items` rows (x_idx given, on the device: NULL here), 64 samples of K = 1
    Family("plain", lambda L, c, a, b, e, n: L.rtfhe_plain_plan(N2, 1, 0, 1, 0, None, c, 1, None, 64, a, b, e, n),
           lambda c: c * 8 * N2, lambda c: 64 * 8 * N2, [(1 << 18) + 3, (1 << 20) + 4], None, None, "overlaps the TRLWE rows x"),
    Family("trgsw_mac", lambda L, c, a, b, e, n: L.rtfhe_trgsw_mac_plan(N2, 1, 1, 1, None, c, 1, None, 64, a, b, e, n),
           lambda c: c * 8 * N2, lambda c: 64 * 8 * N2, [(1 << 18) + 3, (1 << 20) + 4], None, None, "overlaps the TRLWE rows x"),
    # ... and with 64 rows of x and `items` samples: the output is the far array, and count * K the item rule
    Family("plain (far output)", lambda L, c, a, b, e, n: L.rtfhe_plain_plan(N2, 1, 0, 1, 0, None, 64, 1, None, c, a, b, e, n),
           lambda c: 64 * 8 * N2, lambda c: c * 8 * N2, [(1 << 18) + 3, (1 << 20) + 3], (1 << 31) - 1, "count * K", "overlaps the TRLWE rows x", large_out=True),
    Family("trgsw_mac (far output)", lambda L, c, a, b, e, n: L.rtfhe_trgsw_mac_plan(N2, 1, 1, 1, None, 64, 1, None, c, a, b, e, n),
           lambda c: 64 * 8 * N2, lambda c: c * 8 * N2, [(1 << 18) + 3, (1 << 20) + 3], (1 << 31) - 1, "count * K", "overlaps the TRLWE rows x", large_out=True),
    Family("dense", lambda L, c, a, b, e, n: L.rtfhe_dense_plan(n767, 16, 64, c, a, b, e, n),
           lambda c: c * 64 * 4 * (n767 + 1), lambda c: c * 16 * 4 * (n767 + 1), [21900, ((1 << 31) - 1) // (64 * (n767 + 1))], ((1 << 31) - 1) // (64 * (n767 + 1)),
           "count * max(I, O)", "overlaps the input rows x"),
    # RTFHE_SEEDED_DEVICE asks for 16-byte alignment first: the output that shares the b rows' last 16 bytes
    Family("seeded", lambda L, c, a, b, e, n: L.rtfhe_seeded_plan(1, N2, _seed, 5, a, 1, b, c, e, n),
           lambda c: c * 4 * N2, lambda c: c * 8 * N2, [(1 << 19) + 3, (1 << 21) + 3], ((1 << 31) - 1) // (N2 // 16), "rows * N / 16", "overlaps the b rows", last=16),
    # b is one word per row and cannot reach 2^32 bytes below the item rule: the output does
    Family("tlwe_seeded", lambda L, c, a, b, e, n: L.rtfhe_tlwe_seeded_plan(1, n767, _seed, 5, a, b, c, e, n),
           lambda c: c * 4, lambda c: c * 4 * (n767 + 1), [1398102 + 3, 5592405 + 3], ((1 << 31) - 1) // 48, "rows * ceil(n / 16)", "overlaps the b words", large_out=True),
]


def lk_words(L_, k):
    return -(-L_ * k // 32)


@pytest.mark.parametrize("f", FAMILIES, ids=lambda f: f.name)
def test_buffers_past_4_and_16_gib(L, f):
    for items in f.sizes:
        ib, ob = f.in_bytes(items), f.out_bytes(items)
        assert (ob if f.large_out else ib) > 1 << 32, (f.name, items)
        a = BASE
        # directly behind, directly before: accepted
        assert f(L, items, a, a + ib) == 0 and f.msg == "", (f.name, items, f.msg)
        assert f(L, items, a, a - ob) == 0 and f.msg == "", (f.name, items, f.msg)
        # sharing only the input's last word (or 16 bytes), only the output's last word: refused
        for b in (a + ib - f.last, a - ob + f.last):
            assert f(L, items, a, b) == INV and f.overlap_word in f.msg, (f.name, items, hex(b), f.msg)
        # one buffer starting inside the last row of the other, the large one: the output inside the input's, or the input inside the output's
        half = (ob if f.large_out else ib) // items // 2 // 16 * 16
        assert f(L, items, a, a - ob + half if f.large_out else a + ib - half) == INV and f.overlap_word in f.msg, (f.name, items, f.msg)
        # a difference of exactly 2^32 or 2^33 bytes between the two starts is an overlap only if the buffers reach that far
        for d in (1 << 32, 1 << 33):
            assert (f(L, items, a, a + d) == INV) == (d < ib), (f.name, items, d, f.msg)
            assert (f(L, items, a, a - d) == INV) == (d < ob), (f.name, items, d, f.msg)


@pytest.mark.parametrize("f", [f for f in FAMILIES if f.limit], ids=lambda f: f.name)
def test_item_rules_hold_exactly_where_the_bytes_are_terabytes(L, f):
    assert max(f.in_bytes(f.limit), f.out_bytes(f.limit)) > 1 << 32
    far = lambda items: BASE + f.in_bytes(items) + FAR  # noqa: E731
    assert f(L, f.limit, BASE, far(f.limit)) == 0 and f.msg == "", (f.name, f.msg)
    assert f(L, f.limit, BASE, BASE + f.in_bytes(f.limit)) == 0, (f.name, "directly behind, at the limit", f.msg)
    assert f(L, f.limit, BASE, BASE + f.in_bytes(f.limit) - f.last) == INV and f.overlap_word in f.msg, (f.name, f.msg)
    assert f(L, f.limit + 1, BASE, far(f.limit + 1)) == INV and f.limit_word in f.msg, (f.name, f.msg)
    assert f(L, 1 << 32, BASE, far(1 << 32)) == INV and f.limit_word in f.msg, (f.name, "a count whose low 32 bits are zero", f.msg)
    assert f(L, (1 << 32) + 1, BASE, far((1 << 32) + 1)) == INV and f.limit_word in f.msg, (f.name, "a count whose low 32 bits are 1", f.msg)


def test_pack_and_cmux_net_item_rules(L):
    """the two plans that compare no addresses: count * P and count * max(n_nodes, n_out) at the limit"""
    shift = (C.c_int32 * 1024)()
    err = C.create_string_buffer(256)
    most = ((1 << 31) - 1) // 1024
    assert most * 1024 * 4 * 9 > 1 << 32
    assert L.rtfhe_pack_plan(1024, 1024, None, 1, most, BASE, BASE + 4, shift, err, len(err)) == 0
    assert L.rtfhe_pack_plan(1024, 1024, None, 1, most + 1, BASE, BASE + FAR, shift, err, len(err)) == INV and b"count * P" in err.value
    assert L.rtfhe_pack_plan(1024, 1, None, 1, (1 << 32) + 1, BASE, BASE + FAR, shift, err, len(err)) == INV and b"count * P" in err.value

    class World(C.Structure):
        _fields_ = [("N", C.c_int32), ("n_lut", C.c_int32), ("n_sel", C.c_int32), ("has_row0", C.c_int32), ("has_sel_idx", C.c_int32), ("count", C.c_size_t)]
    f = L.rtfhe_cmux_net_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 5 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5 + [C.c_char_p, C.c_size_t]
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    var, hi, lo, out_ref = i32(0), i32(-1), i32(-2), i32(0)
    order, level_off, n_levels, span = i32(0), i32(0, 0), i32(0), i32(0, 0)
    node_bytes = C.c_size_t()

    def plan(count):
        w = World(1024, 2, 1, 1, 1, count)
        return f(C.byref(w), var.ctypes.data, hi.ctypes.data, lo.ctypes.data, None, 1, 1, out_ref.ctypes.data, None, 1, order.ctypes.data,
                 level_off.ctypes.data, n_levels.ctypes.data, span.ctypes.data, C.byref(node_bytes), err, len(err))
    for count in ((1 << 19) + 3, (1 << 21) + 3, (1 << 31) - 1):
        assert plan(count) == 0 and node_bytes.value == count * 8192 > 1 << 32, (count, err.value)
    for count in (1 << 31, 1 << 32, (1 << 32) + 1):
        assert plan(count) == INV and b"count * max(n_nodes, n_out)" in err.value, (count, err.value)


# ---- the arithmetic half of tests/large_kit.py ---------------------------------------------------------------------------------------------
def test_large_kit_boundaries_segments_and_probes():
    assert lk.ks_segment(1024) == 523776 and lk.ks_segment(2048) == 261632
    for N in (1024, 2048):
        assert lk.ks_segment(N) % 512 == 0 and lk.ks_segment(N) * (N + 1) * 4 <= 1 << 31 < (lk.ks_segment(N) + 512) * (N + 1) * 4
    b = lk.boundaries(8192)
    assert b == {"B31": 1 << 18, "B32": 1 << 19, "W31": 1 << 20, "W32": 1 << 21}
    b = lk.boundaries(4100)
    assert b["B31"] * 4100 <= 1 << 31 < (b["B31"] + 1) * 4100 and b["B31"] == 523776
    assert lk.crossed(1 << 19, 8192) == ["B31"] and lk.crossed((1 << 19) + 1, 8192) == ["B31", "B32"]
    assert lk.crossed((1 << 20) + 3, 16384) == list(lk.NAMES)
    count = 1047552 + 2048 + 37
    p = lk.probe_items(count, 4100, lk.ks_segment(1024))
    assert p.dtype == np.int64 and (np.diff(p) > 0).all() and p[0] == 0 and p[-1] == count - 1
    for m in (0, lk.ks_segment(1024), 2 * lk.ks_segment(1024), 1047552, count):
        want = np.arange(max(m - 32, 0), min(m + 32, count))
        assert np.isin(want, p).all(), m
    assert 4 * 64 + 32 + 32 <= p.size <= 4 * 64 + 64 + lk.RANDOM_PROBES
    assert np.array_equal(p, lk.probe_items(count, 4100, lk.ks_segment(1024))), "a fixed seed"
    small = lk.probe_items(40, 4100)
    assert np.array_equal(small, np.arange(40))
