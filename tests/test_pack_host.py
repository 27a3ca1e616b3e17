"""CPU: the packing key switch without a device -- the numpy oracle (tests/pack_oracle.py) pins the table convention against lut_polynomial,
rtfhe_packing_keygen's rows decrypt to their messages, and the noise of a packed row stays inside the bound derived in DESIGN.md 5.11."""
import numpy as np
import pytest

import pack_oracle as O
from pack_helpers import ALPHA, noise_bound, pack_noise, sdist

@pytest.mark.parametrize("N,p", [(1024, 1), (1024, 2), (1024, 3), (2048, 2)])
def test_table_layout_gives_lut_polynomial(N, p):
    """All-zero key, trivial samples (a = 0, b = enc_out(f(e))): with lut_pack_layout the packed row is (lut_polynomial(f), 0) word for word."""
    import rustfhe_amd as R
    rp = R.Params(n=12, N=N)
    rng = np.random.default_rng(100 * p + N)
    f = rng.integers(0, 1 << p, 1 << p)
    pk = np.zeros((rp.n, rp.ks_t, 3, 2, N), np.uint32)
    tlwe = np.zeros((1 << p, rp.n + 1), np.uint32)
    tlwe[:, rp.n] = R.encode_msgs(f, p)
    pos, rep = R.lut_pack_layout(N, p)
    assert rep == N >> p and pos.dtype == np.int32 and pos[0] == 2 * N - rep // 2 and pos[1] == rep - rep // 2
    out = O.pack(rp, pk, tlwe[None], 1 << p, pos, rep)
    assert out.shape == (1, 2, N)
    assert np.array_equal(out[0, 0], R.lut_polynomial(list(f), N, p)) and not out[0, 1].any()


def test_keygen_rows_decrypt_to_their_messages():
    import rustfhe_amd as R
    rp = R.Params(n=24)
    key0, key1, _, _ = R.keygen(rp, 21, want_bk=False, want_ksk=False)
    pk = R.packing_keygen(rp, key0, key1, 5)
    assert pk.shape == (rp.n, 8, 3, 2, rp.N) and pk.dtype == np.uint32
    assert np.array_equal(pk, R.packing_keygen(rp, key0, key1, 5))            # reproducible from the seed
    assert not np.array_equal(pk, R.packing_keygen(rp, key0, key1, 6))        # another seed: other words
    coefs = list(np.flatnonzero(key0 == 1)[:4]) + list(np.flatnonzero(key0 == 0)[:4])       # 8 coefficients i, both key bits
    assert len(coefs) == 8
    worst = 0
    for i in coefs:
        ph = R.trlwe_phase(rp, key1, pk[i].reshape(-1, 2, rp.N)).reshape(8, 3, rp.N)
        for j in range(8):
            for d in range(3):
                want = np.zeros(rp.N, np.int64)
                want[0] = (d + 1) * int(key0[i]) * (1 << (32 - 2 * (j + 1))) % 2 ** 32
                worst = max(worst, int(sdist(ph[j, d], want).max()))
    print("largest row noise: %.2f * 2^-25" % (worst / 2.0 ** 32 / ALPHA))
    assert worst <= 8 * ALPHA * 2 ** 32
    # production form: fresh words every call, rows still valid
    a, b = R.packing_keygen(rp, key0, key1), R.packing_keygen(rp, key0, key1)
    assert not np.array_equal(a, b)
    ph = R.trlwe_phase(rp, key1, a[3, 2, 1][None])[0]
    want = np.zeros(rp.N, np.int64)
    want[0] = 2 * int(key0[3]) << (32 - 6)
    assert sdist(ph, want).max() <= 8 * ALPHA * 2 ** 32
    # non-binary keys and other ks parameters are refused
    bad = key0.copy()
    bad[3] = 2
    for k0, k1, prm in ((bad, key1, rp), (key0, key1 * 3, rp), (key0, key1, R.Params(n=24, ks_t=4, ks_basebit=4))):
        with pytest.raises(R.RtfheError) as ei:
            R.packing_keygen(prm, k0, k1, 5)
        assert ei.value.code == R._ffi.ERR_INVALID


@pytest.fixture(scope="module")
def real():
    """default parameters: keys, a packing key, 1,024 fresh encryptions of +-1/8 and their key-switched rows from the oracle (shared, read-only)"""
    import types
    import rustfhe_amd as R
    w = types.SimpleNamespace(R=R, rp=R.Params())
    w.key0, w.key1, _, _ = R.keygen(w.rp, 7, want_bk=False, want_ksk=False)
    w.pk = R.packing_keygen(w.rp, w.key0, w.key1, 11)
    w.mu = np.where(np.random.default_rng(3).integers(0, 2, 1024) == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    w.ct = R.encrypt_torus(w.rp, w.key0, w.mu, 5)
    w.S = O.key_switch(w.rp, w.pk, w.ct)
    return w


@pytest.mark.parametrize("case", ["P1024_rep1", "table_P4_rep256"])
def test_noise_through_the_oracle(real, case):
    """measured on this key (h = 335): P = 1024, rep = 1: 3.5e-4; P = 4, rep = 256 (256 outputs): 4.2e-4; bound 8.4e-4"""
    w = real
    if case == "P1024_rep1":
        P, pos, rep = 1024, None, 1
    else:
        pos, rep = w.R.lut_pack_layout(w.rp.N, 2)
        P = 4
    out = O.combine(w.S, P, pos, rep)
    inside, outside = pack_noise(w.R, w.rp, w.key0, w.key1, w.ct, out, P, pos, rep)
    bound = noise_bound(w.rp, w.key0, P, rep)
    print("%s: h = %d, max distance on runs %.3e, outside runs %.3e, bound %.3e" % (case, int(w.key0.sum()), inside, outside, bound))
    assert inside <= bound and outside <= bound
    # every packed coefficient still decodes to its +-1/8
    ph = w.R.trlwe_phase(w.rp, w.key1, out)
    if case == "P1024_rep1":
        assert np.array_equal(ph[0] >> 31, w.mu >> 31)


def _pack_plan(N, P, pos, rep, count, tlwe=0x10000000, out=0x40000000):
    """(rc, message, shift) of rtfhe_pack_plan (rustfhe_amd/csrc/rtfhe_extract_plan.cpp) through ctypes; the two buffers are addresses only"""
    import ctypes as C
    import rustfhe_amd as R
    f = R.load().rtfhe_pack_plan
    f.restype = C.c_int
    f.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    pos = None if pos is None else np.ascontiguousarray(pos, np.int32)
    shift = np.full(P if 1 <= P <= N else 1, -7, np.int32)
    err = C.create_string_buffer(256)
    rc = f(N, P, None if pos is None else pos.ctypes.data, rep, count, tlwe, out, shift.ctypes.data, err, len(err))
    return rc, err.value.decode(), shift


def test_the_pack_plan_fills_the_positions():
    import rustfhe_amd as R
    rc, msg, shift = _pack_plan(1024, 1024, None, 2, 3)
    assert (rc, msg) == (0, "") and np.array_equal(shift, 2 * np.arange(1024))
    pos, rep = R.lut_pack_layout(1024, 2)
    rc, msg, shift = _pack_plan(1024, 4, pos, rep, 1)
    assert (rc, msg) == (0, "") and np.array_equal(shift, pos)
    assert _pack_plan(2048, 2048, None, 2, 0)[0] == 0 and _pack_plan(1024, 1, None, 1024, (1 << 31) - 1)[0] == 0
    assert _pack_plan(1024, 1, None, 1, 1, out=0x10000000)[0] == 0          # the buffers' addresses are not compared


@pytest.mark.parametrize("args,message", [
    ((1024, 0, None, 1, 1), "P = 0 is outside [1, 1024]"),
    ((1024, 1025, None, 1, 1), "P = 1025 is outside [1, 1024]"),
    ((1024, 1, None, 0, 1), "rep = 0 is outside [1, 1024]"),
    ((2048, 1, None, 2049, 1), "rep = 2049 is outside [1, 2048]"),
    ((1024, 1, None, 1, 1 << 31), "count * P too large"),
    ((1024, 3, None, 1, (1 << 31) // 3 + 1), "count * P too large"),
    ((1024, 3, [0, -1, 5], 1, 1), "sample 1: pos = -1 is outside [0, 2048)"),
    ((1024, 3, [0, 2047, 2048], 1, 1), "sample 2: pos = 2048 is outside [0, 2048)"),
    ((16, 3, None, 16, 1), "sample 2: pos = 32 is outside [0, 32) (pos NULL: p * rep)"),
    ((1024, 1, None, 1, 1, 0), "null argument"),
    ((1024, 1, None, 1, 1, 0x10000000, 0), "null argument"),
])
def test_the_pack_plan_refuses_with_the_entry_points_messages(args, message):
    """the whole message: what rtfhe_pack_batch[_dev] reported before the checks moved into the plan"""
    import rustfhe_amd as R
    rc, msg, shift = _pack_plan(*args)
    assert rc == R._ffi.ERR_INVALID and msg == message
    if not message.startswith("sample"):
        assert (shift == -7).all(), "nothing is written on a refusal that comes before the list"


def test_the_pack_plan_needs_room_for_the_positions():
    import rustfhe_amd as R
    import ctypes as C
    assert _pack_plan(1024, 1, None, 1, 1)[0] == 0          # (sets the argument types)
    f = R.load().rtfhe_pack_plan
    err = C.create_string_buffer(64)
    assert f(1024, 1, None, 1, 1, 0x10000000, 0x40000000, None, err, len(err)) == R._ffi.ERR_INVALID and b"null" in err.value
