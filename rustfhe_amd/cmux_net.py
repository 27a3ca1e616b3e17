"""CMUX netlists: decision diagrams over TRGSW-encrypted inputs, levelised on the host, recorded once into a HIP graph and replayed as one
submission (include/rtfhe.h: rtfhe_cmux_circuit_create).  The leveled-mode counterpart of the gate netlists of
rustfhe_amd.circuit and the LUT netlists of rustfhe_amd.lut_circuit.

A node is cmux(S_var, X^rot * hi, lo) on TRLWEs: the encrypted bit of variable `var` selects X^rot * hi (bit 1) or lo (bit 0).  hi and lo are
earlier nodes or table rows.  The CMUX tree (Engine.cmux_tree_batch) and the TRGSW rotation (Engine.trgsw_rotate_batch) are the two degenerate
shapes, cmux_tree_netlist and trgsw_rotate_netlist; bdd_netlist builds the shapes between from a function of the bits.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .engine import _Handle


class CmuxNetlist:
    """References are integers: r >= 0 is node r (in the order the nodes were added), r < 0 is table row -1 - r (CmuxNetlist.row)."""

    def __init__(self, n_vars):
        if int(n_vars) < 1:
            raise ValueError("a netlist has at least one variable")
        self.n_vars = int(n_vars)
        self.nodes = []           # (var, hi, lo, rot)
        self.outputs = []         # (ref, coef or None)

    # ---- construction ----
    @staticmethod
    def row(k):
        """The reference of table row k (counted from the replica's row0)."""
        if int(k) < 0:
            raise ValueError("table rows count from 0")
        return -1 - int(k)

    def _ref(self, r, what):
        r = int(r)
        if r >= len(self.nodes):
            raise ValueError("%s = %d: node %d does not exist yet" % (what, r, r))
        return r

    def node(self, var, hi, lo, rot=0):
        """cmux(S_var, X^rot * hi, lo); returns the new node's reference.  rot < 0 means X^rot: it becomes rot + 2N once N is known (arrays)."""
        var = int(var)
        if not 0 <= var < self.n_vars:
            raise ValueError("var = %d is outside [0, %d)" % (var, self.n_vars))
        self.nodes.append((var, self._ref(hi, "hi"), self._ref(lo, "lo"), int(rot)))
        return len(self.nodes) - 1

    def output(self, ref, coef=None):
        """Names node `ref` an output: the TRLWE itself, or with coef the lvl0 ciphertext of its coefficient coef (all outputs of a netlist take
        one form)."""
        ref = self._ref(ref, "output")
        if ref < 0:
            raise ValueError("an output is a node, not a table row")
        if self.outputs and (self.outputs[0][1] is None) != (coef is None):
            raise ValueError("all outputs of a netlist take one form: every one with a coefficient, or none")
        if coef is not None and int(coef) < 0:
            raise ValueError("coef = %d is negative" % coef)
        self.outputs.append((ref, None if coef is None else int(coef)))
        return ref

    @property
    def n_nodes(self):
        return len(self.nodes)

    # ---- scheduling ----
    def levels(self):
        """Node level = 1 + the highest level among its node children, 0 for a node with only table rows below it.  A list of levels, each a list
        of node numbers in ascending order -- the launches of a replay."""
        lvl, levels = [], []
        for i, (_, hi, lo, _) in enumerate(self.nodes):
            l = max([lvl[r] + 1 for r in (hi, lo) if r >= 0], default=0)
            lvl.append(l)
            while len(levels) <= l:
                levels.append([])
            levels[l].append(i)
        return levels

    def arrays(self, N=None):
        """The description arrays of rtfhe_cmux_circuit_create.  N (the ring degree) resolves negative exponents: rot < 0 becomes rot + 2N."""
        if not self.nodes or not self.outputs:
            raise ValueError("a netlist needs at least one node and one output")
        var, hi, lo, rot = (np.array(c, np.int64) for c in zip(*self.nodes))
        if (rot < 0).any():
            if N is None:
                raise ValueError("negative exponents need N")
            rot = np.where(rot < 0, rot + 2 * int(N), rot)
        extract = self.outputs[0][1] is not None
        return {"n_vars": self.n_vars, "n_nodes": len(self.nodes), "n_out": len(self.outputs), "var": var.astype(np.int32), "hi": hi.astype(np.int32),
                "lo": lo.astype(np.int32), "rot": rot.astype(np.int32), "out_ref": np.array([r for r, _ in self.outputs], np.int32),
                "out_coef": np.array([c for _, c in self.outputs], np.int32) if extract else None}

    def evaluate_plain(self, bits, rows):
        """The clear meaning: bits[v] the value of variable v, rows u32[n][N] the table rows from row0 on.  Returns u32[n_out][N], the selected
        and rotated polynomial of every output (an output with a coefficient means that coefficient of it)."""
        rows = np.ascontiguousarray(rows, np.uint32)
        N = rows.shape[-1]
        rows = rows.reshape(-1, N)
        assert len(bits) == self.n_vars, "one bit per variable"
        val = []
        value = lambda r: val[r] if r >= 0 else rows[-1 - r]  # noqa: E731
        for var, hi, lo, rot in self.nodes:
            val.append(_rotate(value(hi), rot) if int(bits[var]) else value(lo))
        return np.stack([val[r] for r, _ in self.outputs])


def _rotate(p, r):
    """X^r * p, negacyclic, on torus words (r any integer)"""
    N = p.size
    e = (np.arange(N) - int(r)) % (2 * N)
    v = p[e % N]
    return np.where(e >= N, (0 - v.astype(np.int64)) & 0xFFFFFFFF, v).astype(np.uint32)


# ---- builders ----
def cmux_tree_netlist(depth):
    """Engine.cmux_tree_batch as a netlist: level k, node j is cmux(S_k, r_{2j+1}, r_{2j}) over the previous level (level 0: table rows 2j + 1
    and 2j); variable k is address bit k.  2^depth - 1 nodes, one output (TRLWE form)."""
    if int(depth) < 1:
        raise ValueError("depth must be at least 1")
    net = CmuxNetlist(depth)
    prev = [net.row(k) for k in range(1 << depth)]
    for k in range(depth):
        prev = [net.node(k, prev[2 * j + 1], prev[2 * j]) for j in range(len(prev) // 2)]
    net.output(prev[0])
    return net


def trgsw_rotate_netlist(depth, rot=None):
    """Engine.trgsw_rotate_batch as a netlist: step k is cmux(S_k, X^rot[k] * acc, acc) on the previous step (step 0: table row 0).  rot None:
    X^-2^k, stored as -2^k and resolved to 2N - 2^k by arrays(N).  depth nodes, one output (TRLWE form)."""
    if int(depth) < 1:
        raise ValueError("depth must be at least 1")
    rot = [-(1 << k) for k in range(depth)] if rot is None else [int(r) for r in rot]
    if len(rot) != depth:
        raise ValueError("one exponent per step")
    net = CmuxNetlist(depth)
    acc = net.row(0)
    for k in range(depth):
        acc = net.node(k, acc, acc, rot[k])
    net.output(acc)
    return net


def bdd_netlist(n_vars, fn_or_truth_tables, order=None, true_row=0, false_row=1):
    """The reduced ordered multi-output decision diagram of boolean functions of n_vars <= 16 bits, by truth-table reduction: equal sub-diagrams
    are merged (also between outputs) and a node whose two children are equal is dropped.  fn_or_truth_tables: a callable of the tuple of bits
    giving one value or a sequence of them, or the tables [n_out][2^n_vars] indexed by sum(bit_v << v).  order: the variables from the root
    down (default 0, 1, ...).  An output that is 1 selects table row true_row, else false_row.  Outputs in TRLWE form, in the functions' order;
    a constant function has no node to name and is refused."""
    n_vars = int(n_vars)
    if not 1 <= n_vars <= 16:
        raise ValueError("n_vars = %d is outside [1, 16]" % n_vars)
    order = list(range(n_vars)) if order is None else [int(v) for v in order]
    if sorted(order) != list(range(n_vars)):
        raise ValueError("order must name every variable once")
    size = 1 << n_vars
    if callable(fn_or_truth_tables):
        vals = [fn_or_truth_tables(tuple((x >> v) & 1 for v in range(n_vars))) for x in range(size)]
        if not isinstance(vals[0], (tuple, list, np.ndarray)):
            vals = [(v,) for v in vals]
        tt = np.array(vals, np.int64).T
    else:
        tt = np.atleast_2d(np.asarray(fn_or_truth_tables, np.int64))
    if tt.ndim != 2 or tt.shape[1] != size:
        raise ValueError("a truth table has 2^n_vars entries")
    tt = (tt != 0).astype(np.uint8)
    # index the tables by the order: the root's variable is the most significant bit, so a node's lo / hi children are the halves of its table
    x = np.arange(size)
    src = np.zeros(size, np.int64)
    for p, v in enumerate(order):
        src |= ((x >> (n_vars - 1 - p)) & 1) << v
    tt = tt[:, src]
    net = CmuxNetlist(n_vars)
    memo = {}

    def build(t):
        if t.min() == t.max():
            return net.row(true_row if t[0] else false_row)
        half = t.size // 2
        lo_t, hi_t = t[:half], t[half:]
        if np.array_equal(lo_t, hi_t):
            return build(lo_t)
        key = t.tobytes()           # its length says which variable the table starts at
        if key not in memo:
            lo, hi = build(lo_t), build(hi_t)
            memo[key] = net.node(order[n_vars - (t.size.bit_length() - 1)], hi, lo)
        return memo[key]

    for o in range(tt.shape[0]):
        ref = build(tt[o])
        if ref < 0:
            raise ValueError("output %d is constant: it has no node to name" % o)
        net.output(ref)
    return net


class CmuxCircuit(_Handle):
    """A recorded CMUX netlist on an Engine (Engine.cmux_circuit): launch(stream) replays it, close() frees it.  It keeps the device arrays it
    was recorded on alive.  rounded: None records the engine's leveled decomposition in force (Engine.set_leveled_decomposition); True / False
    set it around the recording and restore it after.  The circuit replays in the mode it was recorded in."""

    def __init__(self, engine, netlist, sel, lut, d_out, count, d_sel_idx=None, d_row0=None, rounded=None):
        a = netlist.arrays(engine.p.N)
        self.engine, self.netlist, self.count = engine, netlist, int(count)
        self._destroy = engine.circuit_destroy
        self._keep = (sel, d_out, d_sel_idx, d_row0)
        ptr =lambda v: None if v is None else C.c_void_p(v.ctypes.data)  # noqa: E731
        h = C.c_void_p()
        self.h = None
        before = engine.leveled_decomposition()
        if rounded is not None:
            engine.set_leveled_decomposition(_ffi.DECOMP_ROUNDED if rounded else _ffi.DECOMP_REFERENCE)
        try:
            engine._ck(engine.L.rtfhe_cmux_circuit_create(engine.h, sel.h, lut.h, ptr(a["var"]), ptr(a["hi"]), ptr(a["lo"]), ptr(a["rot"]), a["n_nodes"],
                                                          a["n_vars"], ptr(a["out_ref"]), ptr(a["out_coef"]), a["n_out"], engine._dev(d_sel_idx),
                                                          engine._dev(d_row0), engine._dev(d_out), self.count, C.byref(h)))
        finally:
            if rounded is not None:
                engine.set_leveled_decomposition(before)
        self.rounded = before == _ffi.DECOMP_ROUNDED if rounded is None else bool(rounded)
        self.h = h
        self.levels = len(netlist.levels())      # kernel launches of one replay: levels + 2, and the key switch in the extract form

    def launch(self, stream=None):
        """One replay, asynchronous on `stream`; a replica with a bad device-resident index is skipped and the next Engine.sync raises."""
        self.engine.circuit_launch(self.h, stream)
