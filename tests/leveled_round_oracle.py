"""TEST INFRASTRUCTURE: the leveled entry points with a choice of gadget decomposition (include/rtfhe.h: rtfhe_set_leveled_decomposition).
The CMUX tree, the TRGSW rotation and the CMUX netlist restated word for word as oracle_cmux_tree, oracle_trgsw_rotate and
oracle_cmux_net (tests/leveled_oracle.py) state them, with
round_oracle.cmux(.., ma, mx) in the place of orc_cmux.  With the reference constants they are those three functions
(tests/test_leveled_round_host.py); with the rounded constants they are what the ROUNDED = true twins of k_cmux_tree, k_trgsw_rotate and
k_cmux_net compute (tests/test_gpu_leveled_round.py)."""
import ctypes as C

import numpy as np

import orc
import round_oracle as ro
from round_oracle import REFERENCE, ROUNDED  # noqa: F401
from kit import torus_err  # noqa: F401
from leveled_oracle import as_trlwe, default_rot

U32P = C.POINTER(C.c_uint32)


def _selector(p, sel_f, k):
    trgsw = 2 * 2 * p.l * p.N
    return np.ascontiguousarray(sel_f[int(k) * trgsw:(int(k) + 1) * trgsw])


def _rotated(N, words, r):
    """orc_rotate_u32 by r on both polynomials of u32[2N]"""
    words = np.ascontiguousarray(words, np.uint32)
    out = np.empty(2 * N, np.uint32)
    for h in range(2):
        orc.lib().orc_rotate_u32(N, words[h * N:].ctypes.data_as(U32P), int(r), out[h * N:].ctypes.data_as(U32P))
    return out


def cmux_tree(p, plan, sel_f, sel_idx, rows, coef=None, ksk=None, mode=ROUNDED):
    """oracle_cmux_tree in the given decomposition mode: level k is r'_j = cmux(S_k, r_{2j+1}, r_{2j})."""
    N = p.N
    ma, mx = ro.constants(p.l, p.bgbit, mode)
    nodes = [np.ascontiguousarray(r, np.uint32).reshape(2 * N) for r in rows]
    assert len(nodes) == 1 << len(sel_idx)
    for k in sel_idx:
        S = _selector(p, sel_f, k)
        nodes = [ro.cmux(p, plan, S, nodes[2 * j + 1], nodes[2 * j], ma, mx) for j in range(len(nodes) // 2)]
    if coef is None:
        return nodes[0].reshape(2, N)
    return orc.key_switch(p, ksk, orc.sample_extract(p, nodes[0], int(coef)))


def trgsw_rotate(p, plan, sel_f, sel_idx, rot, trlwe, extract=False, ksk=None, mode=ROUNDED):
    """oracle_trgsw_rotate in the given decomposition mode: step k is acc = cmux(S_k, X^rot[k] * acc, acc)."""
    N = p.N
    ma, mx = ro.constants(p.l, p.bgbit, mode)
    if rot is None:
        rot = default_rot(N, len(sel_idx))
    assert len(rot) == len(sel_idx)
    acc = np.ascontiguousarray(trlwe, np.uint32).reshape(2 * N).copy()
    for k, r in zip(sel_idx, rot):
        acc = ro.cmux(p, plan, _selector(p, sel_f, k), _rotated(N, acc, r), acc, ma, mx)
    if not extract:
        return acc.reshape(2, N)
    return orc.key_switch(p, ksk, orc.sample_extract(p, acc, 0))


def cmux_net(p, plan, sel_f, sel_idx, rows, netlist, ksk=None, mode=ROUNDED):
    """oracle_cmux_net in the given decomposition mode: node i is cmux(S_var[i], X^rot[i] * value(hi[i]), value(lo[i])), in index order."""
    N = p.N
    ma, mx = ro.constants(p.l, p.bgbit, mode)
    a = netlist.arrays(N)
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 2 * N)
    val = []
    value = lambda r: val[r] if r >= 0 else rows[-1 - r]  # noqa: E731
    for var, hi, lo, rot in zip(a["var"], a["hi"], a["lo"], a["rot"]):
        val.append(ro.cmux(p, plan, _selector(p, sel_f, sel_idx[var]), _rotated(N, value(hi), rot), value(lo), ma, mx))
    if a["out_coef"] is None:
        return np.stack([val[r].reshape(2, N) for r in a["out_ref"]])
    return np.stack([orc.key_switch(p, ksk, orc.sample_extract(p, val[r], int(c))) for r, c in zip(a["out_ref"], a["out_coef"])])


# ---- the 6-bit setup of DESIGN.md 5.13, shared by the host test, the GPU meaning tests and the seeds' check ----
MSG_BITS = 6


def noise_bound(depth, N, l=3):
    """r(d, N) = sqrt(d (2 l N 18.5^2 2^-50 + (N/2 + 1) 2^-38 / 3)): per level whose selector bit is 1, the selector rows' 2^-25 noise through
    2 l N balanced 6-bit digits (rms 18.5) plus the rounding error, uniform in +-2^-19, times the binary key ((N/2 + 1) terms on average)."""
    return float(np.sqrt(depth * (2 * l * N * 18.5 ** 2 * 2.0 ** -50 + (N / 2 + 1) * 2.0 ** -38 / 3)))


def meaning_setup(R, rp, key1, n_rows, seed):
    """n_rows rows of N random 6-bit messages: (msgs [n_rows][N], their torus words, {"plain": trivial TRLWEs, "encrypted": encrypt_lut's})."""
    msgs = np.random.default_rng(seed).integers(0, 1 << MSG_BITS, (n_rows, rp.N))
    plain = R.encode_msgs(msgs, MSG_BITS)
    return msgs, plain, {"plain": as_trlwe(plain, rp.N), "encrypted": R.encrypt_lut(rp, key1, plain, seed=seed + 1)}


def address_selectors(R, rp, key1, depth, addr, seed):
    """TRGSW encryptions of the depth bits of addr, least significant first: u32[depth][2][2l][N]."""
    return R.encrypt_selectors(rp, key1, [(addr >> k) & 1 for k in range(depth)], seed=seed + addr)


def gpu_meaning_world(R):
    """The inputs of the GPU meaning tests (tests/test_gpu_leveled_round.py), which tests/test_leveled_round_host.py runs through the
    restatement first: n = 40, N = 1024, 256 rows of N random 6-bit messages, plain and encrypted, and the selectors of three addresses of
    the depth-8 tree and of the 10-step rotation (which rotates row ROT_ROW)."""
    import types
    m = types.SimpleNamespace(ROT_ROW=3, TREE_ADDRS=(0, 255, 0xA5), ROT_ADDRS=(0, 1023, 0x2B5))
    m.rp = R.Params(n=40, N=1024)
    _, m.key1, _, _ = R.keygen(m.rp, 0x6B17, want_bk=False, want_ksk=False)
    m.msgs, m.plain, m.rows = meaning_setup(R, m.rp, m.key1, 256, 0x6B18)
    m.tree_sel = {a: address_selectors(R, m.rp, m.key1, 8, a, 0x5E3) for a in m.TREE_ADDRS}
    m.rot_sel = {a: address_selectors(R, m.rp, m.key1, 10, a, 0x5E4) for a in m.ROT_ADDRS}
    return m
