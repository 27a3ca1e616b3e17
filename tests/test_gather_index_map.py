"""CPU: the index and sign map of the pair kernels' coarse/fine rotated gather (rotated_gather, rustfhe_amd/csrc/rtfhe_device.hpp), restated
in numpy formula for formula and held to the definition of the negacyclic rotated read (rotated_coef: e = (c - r) & (2N - 1), index
e & (N - 1), negated when e >> 10) for every rotation amount, lane and register: 2048 x 64 x 16 cases, equality, no tolerance."""
import numpy as np

N, LANES, REGS = 1024, 64, 16


def gather_map():
    """(byte offset into the polynomial, sign as 0 / 1) of register mm of lane ln at rotation r, as rotated_gather computes them: [2048][64][16]"""
    r = np.arange(2 * N, dtype=np.int64)[:, None, None]
    ln = np.arange(LANES, dtype=np.int64)[None, :, None]
    mm = np.arange(REGS, dtype=np.int64)[None, None, :]
    q, d = r >> 6, ln - (r & 63)
    neg = d < 0
    base = 4 * (d & 63) - np.where(neg, 256, 0)
    base2 = base + np.where(neg, 4096, 0)
    s = q >> 4                                      # the uniform sign; the kernel holds it as 0 / ~0
    sx = s ^ neg                                    # ... and the sign of the one word that can wrap
    Q = q & 15                                      # the case of the dispatch
    blk, flip = (mm - Q) & 15, mm < Q
    addr = np.where(blk == 0, base2, base + 256 * blk)
    sign = np.where(blk == 0, sx, s ^ flip)
    return np.broadcast_to(addr, (2 * N, LANES, REGS)), np.broadcast_to(sign, (2 * N, LANES, REGS))


def test_every_rotation_lane_and_register_reads_the_definitions_word_and_sign():
    addr, sign = gather_map()
    r = np.arange(2 * N, dtype=np.int64)[:, None, None]
    c = np.arange(LANES, dtype=np.int64)[None, :, None] + 64 * np.arange(REGS, dtype=np.int64)[None, None, :]
    e = (c - r) & (2 * N - 1)
    assert addr.shape == e.shape == (2 * N, LANES, REGS)
    assert (addr % 4 == 0).all() and (addr >= 0).all() and (addr < 4 * N).all()
    assert np.array_equal(addr // 4, e & (N - 1))
    assert np.array_equal(sign, e >> 10)


def test_the_base_of_the_immediate_offsets_stays_within_one_block_of_the_polynomial():
    """base is the only address that can be negative (d < 0): never below -252 bytes, so base + 256 blk, blk >= 1, is inside the polynomial"""
    ln = np.arange(LANES)[None, :]
    d = ln - np.arange(64)[:, None]
    base = 4 * (d & 63) - np.where(d < 0, 256, 0)
    assert base.min() == -252 and base.max() == 252
    assert ((base + 256 >= 0) & (base + 256 * 15 + 4 <= 4 * N)).all()


def test_the_signed_word_form_is_the_kernels_pre_decomposition_word():
    """u = ((v ^ sign) + ((MA - sign) - own)) ^ MX with sign 0 / ~0 is (((sign ? -v : v) - own) + MA) ^ MX in 32-bit arithmetic, for both
    decompositions' constants (rtfhe_device.hpp: decomp_add / decomp_xor at l = 3, bgbit = 6)"""
    rng = np.random.default_rng(7)
    v = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    own = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    v[:4], own[:4] = (0, 0xFFFFFFFF, 0x80000000, 1), (0, 0, 0x80000000, 0xFFFFFFFF)
    for ma, mx in ((0x02084000, 0x02084000), (0x82082000, 0x82080000)):
        ma, mx = np.full(1, ma, np.uint32), np.full(1, mx, np.uint32)      # (arrays: modular arithmetic without numpy's scalar overflow warning)
        for sign in (np.zeros(1, np.uint32), np.full(1, 0xFFFFFFFF, np.uint32)):
            got = ((v ^ sign) + ((ma - sign) - own)) ^ mx
            want = (((np.uint32(0) - v if sign[0] else v) - own) + ma) ^ mx
            assert np.array_equal(got, want)
