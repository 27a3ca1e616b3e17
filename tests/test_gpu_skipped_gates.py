"""GPU: skipped gates and netlist waves in every kernel family.

Every *_dev entry point checks its indices on the device: a gate with a bad wire index, opcode, table index or selector index is skipped and
the next rtfhe_sync reports RTFHE_ERR_INVALID once.  Each kernel body states that rule itself (an early return, a `live` flag around every
store, a second gate_io in an epilogue, k_key_switch_mm's own copy of the rule), so it is checked here family by family -- on buffers that are
filled with a nonzero, row-dependent sentinel, so that "wrote nothing" and "wrote zeros" differ, with guard rows outside the batch.  Netlist
waves (per-gate opcodes, gathered inputs, scattered outputs) are compared word for word with the same engine's plain batches as well.

One key set per ring at n = 64 (n + 1 = 65 is odd: misaligned rows; 64 steps: more than every prefetch depth), one engine per launch shape,
and the session engine (N = 1024, n = 635) for one pass of the default shape.  Batch sizes [1, 4] + gk.forced_sizes(N, C), C = the device's CUs.
What each (shape, batch size) launches, from rtfhe_dispatch_fft.hip / _ntt.hip / _xfft.hip (wg_max = C; a MODE_GATE batch of the default
shapes takes the split path: the family's kernel in MODE_EXTRACT, then k_key_switch_mm):

  N = 1024 mirror       1, 4            C + C/6             2C + C/3            4C                  5C
  default               wg              pair4<2>            pair4<3>            pair<4>             pair_rr (one launch)       + ks_mm
  RTFHE_FORCE_WAVES=1   wg, fused epilogue, at every size      =2: pair<4>, fused      =4 / =8: k_bootstrap<10, .., 4 / 8> (one wave per gate)
  RTFHE_PAIR_RR=0       as default                                                                  pair<4> + wg (C)           + ks_mm
  RTFHE_PAIR4=0         wg              pair<2>             pair<3>             pair<4>             pair_rr                    + ks_mm
  RTFHE_KS_MM_MIN=0     wg              pair<2>             pair<3>             pair<4>             pair_rr        fused epilogues, no ks_mm
  N = 2048 mirror       1, 4, 37        2C + 1              4C + 76
  default               eo4<1>          eo<3>               eo<4> + eo4<1>                                                     + ks_mm
  RTFHE_FORCE_WAVES=4   k_bootstrap<11, .., 4> (one wave per gate), fused, at every size
  RTFHE_N2048_EO4=0     eo<1>           eo<3>               eo<4> + eo<1>                                                      + ks_mm
  NTT exact, N = 1024   ntt_wg          ntt_pair<2>         ntt_pair<3>         ntt_pair<4>         ntt_pair<4> + ntt_wg       + ks_mm
    RTFHE_FORCE_WAVES=4 k_bootstrap_ntt<.., 4> (one wave per gate) at every size
  NTT exact, N = 2048   ntt_halves<1>   ntt_halves<3>       ntt_halves<4> + ntt_halves<1>  (RTFHE_FORCE_WAVES=4 changes nothing here)    + ks_mm
  split-FFT, N = 1024   xpair<1>        xpair<2>            xpair<3>            xpair<4>            xpair_rr (one launch)      + ks_mm
  split-FFT, N = 2048   xquad<1>        xquad<2> + xquad<1> xquad<2> + xquad<1>                                                + ks_mm

A programmable bootstrap takes the same ladder on the k_pbs_* twins (pbs_batch_dev: MODE_GATE, so the split path), a many-LUT PBS and an
encrypted table the k_pbs_many_* / k_pbs_enc_* twins in MODE_EXTRACT followed by one k_key_switch_mm over count * n_out rows (one wave per
sample under RTFHE_KS_MM_MIN=0); the CMUX tree has one kernel, k_cmux_tree<LOGN, .., 4> (four lookups of the last level per workgroup).

Bad positions in a batch of G: gates 0 and G - 1, the last gate before and the first after every multiple of 4C (N = 2048: also of 3C), one
aligned run of 4 (a whole 4-gate workgroup skipped), one aligned run of 16 (a whole key-switch tile), 4 random gates; at G = 1 and 4 also
every gate.  The oracle runs on gates 0, G - 1 and the valid neighbours of every bad gate, once per (ring, batch size) -- the cases do not
depend on the launch shape, so every shape is held to the same oracle rows.  Every comparison is np.array_equal on uint32 words: there is no
tolerance in this file.

Wall time, measured on an MI355X (256 CUs; profiles/r11/README.md): 13.3 s for this file against 235.5 s for the rest of the GPU suite."""
import types

import numpy as np
import pytest

import gpu_kit as gk
from kit import random_words
from leveled_kit import tree_oracle
from leveled_oracle import as_trlwe
from pbs_oracle import bk_fft, oracle_pbs, oracle_pbs_enc, oracle_pbs_many

pytestmark = pytest.mark.gpu

N_MASK = 64
IN_ROWS, GUARD = 64, 8
OP_LAST = 6                                     # OP_ANDNY: the last opcode a netlist accepts
SHAPES = {1024: gk.CONFIGS_1024, 2048: gk.CONFIGS_2048}
MIRROR = [(N, env) for N in (1024, 2048) for env in SHAPES[N]]
EXACT = [(N, b, env) for N in (1024, 2048) for b, env in (("ntt", None), ("ntt", {"RTFHE_FORCE_WAVES": "4"}), ("xfft", None))]


def _sentinel(rows, width, salt=0):
    """nonzero words that differ from row to row and from word to word"""
    r = np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(salt + 1)
    c = np.arange(width, dtype=np.uint64)[None, :]
    return ((r * np.uint64(0x9E3779B1) + c * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)).astype(np.uint32) | np.uint32(1)


def _sizes(N, C):
    return sorted(set([1, 4] + gk.forced_sizes(N, C)))


def _bad_positions(G, N, C, rng):
    """the positions the module docstring lists (G = 1: gate 0; G = 4: gates 0 and 3, the rest stay valid)"""
    s = {0, G - 1}
    for per in ((4,) if N == 1024 else (3, 4)):
        for b in range(per * C, G, per * C):
            s |= {b - 1, b}
    if G >= 8:
        a = 4 * int(rng.integers(1, G // 4))
        s |= set(range(a, a + 4))
    if G >= 32:
        a = 16 * int(rng.integers(1, G // 16))
        s |= set(range(a, a + 16))
    rest = np.setdiff1d(np.arange(G), sorted(s))
    if G >= 8:
        s |= set(rng.choice(rest, min(4, rest.size), replace=False).tolist())
    return np.array(sorted(s), np.int64)


def _picks(G, bad):
    """gates 0 and G - 1 and both neighbours of every bad gate"""
    s = {0, G - 1}
    for g in bad.tolist():
        s |= {g - 1, g + 1}
    return sorted(g for g in s if 0 <= g < G)


def _expect_invalid_once(e, st):
    import rustfhe_amd as R
    with pytest.raises(R.RtfheError) as ei:
        e.sync(st)
    assert ei.value.code == R._ffi.ERR_INVALID
    e.sync(st)                                  # reported once


class Ring:
    """One key set of the oracle's keygen at n = 64, the inputs every netlist wave of this ring gathers from, three plain and three
    encrypted tables, and the oracle rows computed so far (shared between the launch shapes, read-only)."""

    def __init__(self, orc, N, n=N_MASK, keys=None, P=None):
        import rustfhe_amd as R
        self.orc, self.N, self.n = orc, N, n
        self.P = P or orc.Params(n=n, N=N)
        self.K = keys or orc.Keys(self.P, 6400 + N)
        self.p = R.Params(n=n, N=N)
        self.C = gk.cus()
        rng = np.random.default_rng(N + n)
        self.inputs = random_words(rng, (IN_ROWS, n + 1))
        self.tv = random_words(rng, (3, N))
        self.trl = R.encrypt_lut(self.p, self.K.key1, self.tv, seed=N + n)
        self.memo = {}

    def engine(self, monkeypatch=None, env=None):
        import rustfhe_amd as R
        return gk.engine(R, self.p, self.K.bk_t, self.K.ksk, monkeypatch, env)

    def oracle_gates(self, exact, ops, i0, i1):
        """orc.gate of (op, input row, input row) triples, on the mirror or on the exact-integer backend"""
        orc, K = self.orc, self.K
        backend = orc.BACKEND_EXACT if exact else orc.BACKEND_MIRROR
        todo = sorted({(exact, int(o), int(a), int(b)) for o, a, b in zip(ops, i0, i1)} - set(self.memo))
        rows = gk.pmap(lambda k: orc.gate(self.P, gk.oracle_plan(orc, self.N, backend), k[1], None if exact else K.bk_f, K.bk_t if exact else None, K.ksk,
                                        self.inputs[k[2]], self.inputs[k[3]]), todo)
        self.memo.update(zip(todo, rows))
        return np.stack([self.memo[exact, int(o), int(a), int(b)] for o, a, b in zip(ops, i0, i1)])

    def oracle_pbs(self, key, fn, picks):
        """fn(g) for the picks, memoised under (key, g)"""
        todo = [g for g in picks if (key, g) not in self.memo]
        self.memo.update(zip([(key, g) for g in todo], gk.pmap(fn, todo)))
        return np.stack([self.memo[key, g] for g in picks])


@pytest.fixture(scope="module")
def rings(orc):
    return gk.Worlds(lambda N: Ring(orc, N))


# ---- 1. netlist waves ----------------------------------------------------------------------------------------------------------------------
def _wave_case(ring, G, all_bad=False):
    """A wave of G gates over a table of 64 input rows, G output rows reached through a random permutation and 8 guard rows; every row but the
    inputs holds the sentinel.  The same case for every launch shape of the ring."""
    rng = np.random.default_rng([ring.N, ring.n, G, int(all_bad)])
    W = IN_ROWS + G + GUARD
    c = types.SimpleNamespace(G=G, W=W)
    c.table = _sentinel(W, ring.n + 1)
    c.table[:IN_ROWS] = ring.inputs
    c.ops = rng.integers(0, OP_LAST + 1, G).astype(np.int32)
    c.i0, c.i1 = rng.integers(0, IN_ROWS, G).astype(np.int32), rng.integers(0, IN_ROWS, G).astype(np.int32)
    c.io = (IN_ROWS + rng.permutation(G)).astype(np.int32)
    c.bad = np.arange(G) if all_bad else _bad_positions(G, ring.N, ring.C, rng)
    kinds = [("i0", -1), ("i0", W), ("i0", 10 ** 7), ("i1", W), ("io", -1), ("io", W), ("ops", -1), ("ops", OP_LAST + 1), ("ops", 99)]
    c.b = {k: getattr(c, k).copy() for k in ("ops", "i0", "i1", "io")}
    for k, g in enumerate(c.bad.tolist()):        # one bad field per bad gate: its idx_out stays valid unless idx_out is the bad field
        field, v = kinds[k % len(kinds)]
        c.b[field][g] = v
    c.valid = np.ones(G, bool)
    c.valid[c.bad] = False
    return c


def _launch_wave(e, c, ops, i0, i1, io):
    import torch
    wires = torch.from_numpy(c.table.view(np.int32).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    e.circuit_wave_dev(gk.to_device(ops), gk.to_device(i0), gk.to_device(i1), gk.to_device(io), wires, c.W, c.G, st)
    return wires, st


def _table_diff(got, exp, c):
    rows = np.flatnonzero((got != exp).any(axis=1))
    if rows.size == 0:
        return None
    gate_of = {int(r): g for g, r in enumerate(c.io.tolist())}
    return [("input" if r < IN_ROWS else "guard" if r >= IN_ROWS + c.G else "gate %d%s" % (gate_of[r], "" if c.valid[gate_of[r]] else " (bad)"), int(r))
            for r in rows[:12].tolist()]


def _check_waves(ring, e, exact, label):
    """every batch size: the wave with bad gates, then the clean wave of the same size; at G = 1 and 4 also the wave whose gates are all bad"""
    for G in _sizes(ring.N, ring.C):
        for all_bad in ((False, True) if G <= 4 else (False,)):
            c = _wave_case(ring, G, all_bad)
            ref = np.empty((G, ring.n + 1), np.uint32)              # the same engine's plain batches, opcode by opcode, over the whole wave
            for op in range(OP_LAST + 1):
                sel = np.flatnonzero(c.ops == op)
                if sel.size:
                    ref[sel] = e.gate_batch(op, ring.inputs[c.i0[sel]], ring.inputs[c.i1[sel]])
            pick = _picks(G, c.bad)
            assert np.array_equal(ref[pick], ring.oracle_gates(exact, c.ops[pick], c.i0[pick], c.i1[pick])), (label, G, "gate_batch against the oracle")
            wires, st = _launch_wave(e, c, c.b["ops"], c.b["i0"], c.b["i1"], c.b["io"])
            _expect_invalid_once(e, st)
            exp = c.table.copy()
            exp[c.io[c.valid]] = ref[c.valid]
            assert _table_diff(gk.words_of(wires), exp, c) is None, (label, G, all_bad, _table_diff(gk.words_of(wires), exp, c))
            wires, st = _launch_wave(e, c, c.ops, c.i0, c.i1, c.io)
            e.sync(st)
            exp = c.table.copy()
            exp[c.io] = ref
            assert _table_diff(gk.words_of(wires), exp, c) is None, (label, G, all_bad, "clean wave", _table_diff(gk.words_of(wires), exp, c))


@pytest.mark.parametrize("N,env", MIRROR, ids=lambda v: str(v) if isinstance(v, int) else gk.env_id(v))
def test_netlist_wave_skips_bad_gates_mirror(rings, monkeypatch, N, env):
    """Valid gates' rows equal gate_batch(op) of the same engine on the gathered inputs (and the oracle on the picks); every other row of the
    table -- inputs, the target rows of bad gates, guard rows -- is unchanged; sync raises ERR_INVALID once; a clean wave follows."""
    ring = rings(N)
    e = ring.engine(monkeypatch, env)
    try:
        _check_waves(ring, e, False, (N, gk.env_id(env)))
    finally:
        e.close()


@pytest.mark.parametrize("N,backend,env", EXACT, ids=lambda v: str(v) if not isinstance(v, (dict, type(None))) else gk.env_id(v))
def test_netlist_wave_skips_bad_gates_exact_backends(rings, monkeypatch, N, backend, env):
    """The same on the NTT backend (default shape and RTFHE_FORCE_WAVES=4) and on the split-FFT backend, against the exact-integer oracle."""
    import rustfhe_amd as R
    ring = rings(N)
    e = ring.engine(monkeypatch, env)
    try:
        e.set_backend(R._ffi.BACKEND_NTT_EXACT if backend == "ntt" else R._ffi.BACKEND_FFT_SPLIT_EXACT)
        _check_waves(ring, e, True, (N, backend, gk.env_id(env)))
    finally:
        e.close()


def test_netlist_wave_skips_bad_gates_session_engine(orc, params, keys, engine):
    """One pass of the default shape at the full parameter set (N = 1024, n = 635)."""
    ring = Ring(orc, params.N, params.n, keys, params)
    _check_waves(ring, engine, False, "session engine")


# ---- 2. device-indexed tables ---------------------------------------------------------------------------------------------------------------
BAD_LUT_IDX = (-1, 3, 2 ** 31 - 1, -2 ** 31)
VARIANTS = [("pbs", False, 1), ("many", False, 1), ("many", False, 4), ("pbs", True, 1), ("many", True, 1), ("many", True, 4)]


def _pbs_dev(e, lut, call, n_out, ct, idx, salt):
    """the _dev call into the middle of a sentinel-filled tensor with 8 guard rows on each side; (output rows, guards intact, stream)"""
    import torch
    G, n1 = ct.shape
    fill = _sentinel(G * n_out + 2 * GUARD, n1, salt)
    big = torch.from_numpy(fill.view(np.int32).copy()).cuda()
    out = big[GUARD:GUARD + G * n_out]
    st = torch.cuda.current_stream().cuda_stream
    if call == "pbs":
        e.pbs_batch_dev(lut, gk.to_device(ct.view(np.int32)), out, G, gk.to_device(idx), st)
    else:
        e.pbs_many_batch_dev(lut, gk.to_device(ct.view(np.int32)), out, G, n_out, gk.to_device(idx), st)
    return big, fill, st


def _guards_intact(big, fill, rows):
    got = gk.words_of(big)
    return np.array_equal(got[:GUARD], fill[:GUARD]) and np.array_equal(got[GUARD + rows:], fill[GUARD + rows:])


@pytest.mark.parametrize("N,env", MIRROR, ids=lambda v: str(v) if isinstance(v, int) else gk.env_id(v))
def test_device_indexed_tables_skip_bad_gates(rings, monkeypatch, N, env):
    """pbs_batch_dev, pbs_many_batch_dev (n_out 1 and 4) and both with an encrypted table, lut_idx = -1, 3, 2^31 - 1, -2^31 at the bad
    positions: valid gates' rows equal a clean run of the same engine (and the oracle on the picks), the guard rows around the output are
    unchanged, the error is reported once.  A skipped gate's own rows are left open by the header and are not looked at."""
    ring = rings(N)
    orc, P, K = ring.orc, ring.P, ring.K
    e = ring.engine(monkeypatch, env)
    try:
        with e.lut(ring.tv) as plain, e.lut_encrypted(ring.trl) as enc:
            for G in _sizes(N, ring.C):
                rng = np.random.default_rng([N, G, 2])
                ct = random_words(rng, (G, ring.n + 1))
                idx = rng.integers(0, 3, G).astype(np.int32)
                bad = _bad_positions(G, N, ring.C, rng)
                bad_idx = idx.astype(np.int64)
                bad_idx[bad] = [BAD_LUT_IDX[k % 4] for k in range(bad.size)]
                bad_idx = bad_idx.astype(np.int32)
                valid = np.ones(G, bool)
                valid[bad] = False
                pick = [g for g in _picks(G, bad)]
                for vi, (call, encrypted, n_out) in enumerate(VARIANTS):
                    label = (N, gk.env_id(env), call, "encrypted" if encrypted else "plain", n_out, G)
                    lut = enc if encrypted else plain
                    big, fill, st = _pbs_dev(e, lut, call, n_out, ct, idx, vi)
                    e.sync(st)
                    assert _guards_intact(big, fill, G * n_out), (label, "clean run: guard rows")
                    clean = gk.words_of(big)[GUARD:GUARD + G * n_out].reshape(G, n_out, -1).copy()
                    if encrypted:
                        fn = lambda g: oracle_pbs_enc(orc, P, gk.oracle_plan(orc, N), K.bk_f, K.ksk, ring.trl[idx[g]], ct[g], n_out)  # noqa: E731
                    elif call == "pbs":
                        fn = lambda g: oracle_pbs(orc, P, gk.oracle_plan(orc, N), K.bk_f, K.ksk, ring.tv[idx[g]], ct[g])[None]  # noqa: E731
                    else:
                        fn = lambda g: oracle_pbs_many(orc, P, gk.oracle_plan(orc, N), K.bk_f, K.ksk, ring.tv[idx[g]], ct[g], n_out)  # noqa: E731
                    want = ring.oracle_pbs(("pbs", G, encrypted, "pbs" if call == "pbs" and not encrypted else n_out), fn, pick)
                    assert np.array_equal(clean[pick], want.reshape(len(pick), n_out, -1)), (label, "clean run against the oracle")
                    big, fill, st = _pbs_dev(e, lut, call, n_out, ct, bad_idx, vi + 8)
                    _expect_invalid_once(e, st)
                    got = gk.words_of(big)[GUARD:GUARD + G * n_out].reshape(G, n_out, -1)
                    assert np.array_equal(got[valid], clean[valid]), (label, np.flatnonzero((got != clean).any(axis=(1, 2)) & valid)[:12])
                    assert _guards_intact(big, fill, G * n_out), (label, "guard rows")
    finally:
        e.close()


# ---- 3. CMUX tree ---------------------------------------------------------------------------------------------------------------------------
N_SEL, N_ROWS = 8, 8 + 3


@pytest.fixture(scope="module", params=[1024, 2048], ids=lambda N: "N%d" % N)
def tree_world(request, rings, orc):
    """the ring's key set with eight selectors of known bits and an 11-row plain and encrypted table, in the shape leveled_kit.tree_oracle reads"""
    import rustfhe_amd as R
    ring = rings(request.param)
    w = types.SimpleNamespace(R=R, N=ring.N, rp=ring.p, P=ring.P, plan=orc.Plan(ring.N), ksk=ring.K.ksk, C=ring.C, oracle_memo={})
    rng = np.random.default_rng(ring.N + 3)
    sel_t = R.encrypt_selectors(ring.p, ring.K.key1, rng.integers(0, 2, N_SEL).astype(np.uint8), seed=0x5E1 + ring.N)
    w.sel_f = bk_fft(orc, w.P, w.plan, sel_t.reshape(-1))
    w.rows = {"plain": random_words(rng, (N_ROWS, ring.N)), "encrypted": R.encrypt_lut(ring.p, ring.K.key1, random_words(rng, (N_ROWS, ring.N)), seed=0x7AB + ring.N)}
    assert as_trlwe(w.rows["plain"], ring.N).shape == (N_ROWS, 2, ring.N)
    w.eng = ring.engine()
    w.sel = w.eng.selectors(sel_t)
    w.lut = {"plain": w.eng.lut(w.rows["plain"]), "encrypted": w.eng.lut_encrypted(w.rows["encrypted"])}
    yield w
    for h in (w.sel, w.lut["plain"], w.lut["encrypted"]):
        h.close()
    w.eng.close()


def _tree_dev(w, kind, depth, count, sel_idx, row0, coef, extract, salt):
    import torch
    width = w.rp.n + 1 if extract else 2 * w.N
    fill = _sentinel(count + 2 * GUARD, width, salt)
    big = torch.from_numpy(fill.view(np.int32).copy()).cuda()
    out = big[GUARD:GUARD + count]
    st = torch.cuda.current_stream().cuda_stream
    if extract:
        w.eng.cmux_tree_extract_batch_dev(w.sel, w.lut[kind], depth, out, count, gk.to_device(sel_idx), gk.to_device(row0), gk.to_device(coef), st)
    else:
        w.eng.cmux_tree_batch_dev(w.sel, w.lut[kind], depth, out, count, gk.to_device(sel_idx), gk.to_device(row0), st)
    return big, fill, st


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_cmux_tree_skips_bad_lookups(orc, tree_world, depth):
    """cmux_tree_batch_dev and the extract form, plain and encrypted tables, counts 1, 5, 37 and 4C + 1: bad sel_idx, row0 and coef values at
    the first and the last lookup, then at an aligned run of 4 lookups (one workgroup of the last level).  Valid lookups equal the clean run
    (and leveled_kit.tree_oracle on the picks), the guard rows are unchanged, the error is reported once."""
    w = tree_world
    for count in (1, 5, 37, 4 * w.C + 1):
        rng = np.random.default_rng([w.N, depth, count])
        sel_idx = rng.integers(0, N_SEL, (count, depth)).astype(np.int32)
        row0 = rng.integers(0, N_ROWS - (1 << depth) + 1, count).astype(np.int32)
        coef = rng.integers(0, w.N, count).astype(np.int32)
        coef[0], coef[-1] = w.N - 1, 0
        run = 4 * ((count // 4) // 2)
        places = [np.array(sorted({0, count - 1}))] + ([np.arange(run, run + 4)] if count >= 4 else [])
        for extract in (False, True):
            kinds = [("sel", -1), ("sel", N_SEL), ("row0", -1), ("row0", N_ROWS - (1 << depth) + 1)] + ([("coef", -1), ("coef", w.N)] if extract else [])
            for ki, kind in enumerate(("plain", "encrypted")):
                label = (w.N, depth, count, "extract" if extract else "tree", kind)
                big, fill, st = _tree_dev(w, kind, depth, count, sel_idx, row0, coef, extract, 0)
                w.eng.sync(st)
                assert _guards_intact(big, fill, count), (label, "clean run: guard rows")
                clean = gk.words_of(big)[GUARD:GUARD + count].copy()
                for pi, bad in enumerate(places):
                    b_sel, b_row, b_coef = sel_idx.copy(), row0.copy(), coef.copy()
                    for k, g in enumerate(bad.tolist()):
                        field, v = kinds[(k + pi + ki) % len(kinds)]
                        if field == "sel":
                            b_sel[g, (g + k) % depth] = v
                        elif field == "row0":
                            b_row[g] = v
                        else:
                            b_coef[g] = v
                    valid = np.ones(count, bool)
                    valid[bad] = False
                    pick = np.array(_picks(count, bad))
                    want = tree_oracle(orc, w, kind, depth, sel_idx[pick], row0[pick], coef[pick] if extract else None)
                    assert np.array_equal(clean[pick], want.reshape(len(pick), -1)), (label, "clean run against the oracle")
                    big, fill, st = _tree_dev(w, kind, depth, count, b_sel, b_row, b_coef, extract, 1 + pi)
                    _expect_invalid_once(w.eng, st)
                    got = gk.words_of(big)[GUARD:GUARD + count]
                    assert np.array_equal(got[valid], clean[valid]), (label, pi, np.flatnonzero((got != clean).any(axis=1) & valid)[:12])
                    assert _guards_intact(big, fill, count), (label, pi, "guard rows")
