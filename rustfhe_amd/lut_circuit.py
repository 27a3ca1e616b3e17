"""LUT circuits: netlists whose nodes are "weighted sum of wires, then a many-LUT bootstrap", levelled into waves, recorded once into a HIP graph
and replayed as one submission (include/rtfhe.h: rtfhe_lut_circuit_create).  The programmable-bootstrapping counterpart of the
gate netlists of rustfhe_amd.circuit.

Every wire carries a message of one width p (rustfhe_amd.pbs: m in [0, 2^p) is the torus word m * 2^(32-p-1)).  A node computes
s = sum_k w_k * m_k + const, which must stay in [0, 2^p) (the padding bit), and its table's theta functions of s, each a new p-bit wire.
"""
import numpy as np

from .engine import _Handle
from .pbs import many_lut_polynomial


def _value(f, m):
    return f(m) if callable(f) else int(f[m])


class LutNetlist:
    """Wires are integers: the inputs first (0 .. num_inputs - 1), then the outputs of every node in the order the nodes were added."""

    def __init__(self, msg_bits):
        self.p = msg_bits
        self.num_inputs = 0
        self.tables = []          # lists of theta functions (callables or 2^p values)
        self.nodes = []           # (terms [(wire, weight)], const, table, first output wire)
        self.outputs = []
        self._num_wires = 0

    # ---- construction ----
    def input(self):
        assert not self.nodes, "declare all inputs before the first node"
        self.num_inputs += 1
        self._num_wires += 1
        return self.num_inputs - 1

    def inputs(self, k):
        return [self.input() for _ in range(k)]

    def table(self, fs):
        """theta = len(fs) (1, 2, 4 or 8) functions of a p-bit message, p-bit results; returns the table's index."""
        fs = list(fs)
        if len(fs) not in (1, 2, 4, 8):
            raise ValueError("a table holds 1, 2, 4 or 8 functions (got %d)" % len(fs))
        self.tables.append(fs)
        return len(self.tables) - 1

    def node(self, terms, const=0, table=0):
        """s = sum(weight * wire for wire, weight in terms) + const (const in message units, added to the b word only), then table `table`:
        returns its theta new wires."""
        terms = [(int(w), int(k)) for w, k in terms]
        if len(terms) > 8:
            raise ValueError("a node sums at most 8 wires")
        if not 0 <= table < len(self.tables):
            raise ValueError("no table %d" % table)
        for w, _ in terms:
            if not 0 <= w < self._num_wires:
                raise ValueError("wire %d does not exist yet" % w)
        first = self._num_wires
        th = len(self.tables[table])
        self.nodes.append((terms, int(const), table, first))
        self._num_wires += th
        return tuple(range(first, first + th))

    def output(self, w):
        self.outputs.append(w)
        return w

    @property
    def num_wires(self):
        return self._num_wires

    def n_out(self, g):
        return len(self.tables[self.nodes[g][2]])

    # ---- scheduling ----
    def levels(self):
        """Node level = 1 + the highest level among its input wires (inputs: level 0).  A list of levels, each a list of node indices."""
        lvl = np.zeros(self._num_wires, np.int64)
        levels = []
        for g, (terms, _, table, first) in enumerate(self.nodes):
            l = 1 + max([int(lvl[w]) for w, _ in terms], default=0)
            lvl[first:first + len(self.tables[table])] = l
            while len(levels) < l:
                levels.append([])
            levels[l - 1].append(g)
        return levels

    def waves(self):
        """The levels, each split into consecutive sub-waves of one theta (ascending): a list of (theta, [node indices])."""
        out = []
        for level in self.levels():
            for th in (1, 2, 4, 8):
                nodes = [g for g in level if self.n_out(g) == th]
                if nodes:
                    out.append((th, nodes))
        return out

    def evaluate_plain(self, msgs):
        """Reference semantics on plain integers: the input messages in, the output wires' messages out.  Raises ValueError when a node's sum
        leaves [0, 2^p) -- the padding-bit condition (a range check only: it says nothing about noise)."""
        assert len(msgs) == self.num_inputs
        v = [int(m) for m in msgs] + [0] * (self._num_wires - self.num_inputs)
        for m in v[:self.num_inputs]:
            if not 0 <= m < (1 << self.p):
                raise ValueError("input message %d outside [0, 2^%d)" % (m, self.p))
        for g, (terms, const, table, first) in enumerate(self.nodes):
            s = sum(k * v[w] for w, k in terms) + const
            if not 0 <= s < (1 << self.p):
                raise ValueError("node %d: sum %d leaves [0, 2^%d)" % (g, s, self.p))
            for j, f in enumerate(self.tables[table]):
                v[first + j] = _value(f, s)
        return [v[w] for w in self.outputs]

    def polynomials(self, N):
        """The test polynomials of every table, u32[num_tables][N] (many_lut_polynomial with p-bit outputs)."""
        return np.stack([many_lut_polynomial(fs, N, self.p, out_bits=self.p) for fs in self.tables])

    def arrays(self, replicas=1):
        """The description arrays of rtfhe_lut_circuit_create for `replicas` independent instances side by side in one wire table: replica r's
        wire w is row r * num_wires + w.  Every wave holds its nodes for all replicas, replica by replica."""
        W = self._num_wires
        fan_in = max([len(t) for t, _, _, _ in self.nodes], default=1) or 1
        sh = 32 - self.p - 1
        in_idx, weights, cst, lut_idx, out_idx, offs, n_out = [], [], [], [], [], [0], []
        for th, nodes in self.waves():
            for r in range(replicas):
                base = r * W
                for g in nodes:
                    terms, const, table, first = self.nodes[g]
                    pad = fan_in - len(terms)
                    in_idx.append([base + w for w, _ in terms] + [-1] * pad)
                    weights.append([k for _, k in terms] + [0] * pad)
                    cst.append((const << sh) & 0xFFFFFFFF)
                    lut_idx.append(table)
                    out_idx.extend(base + first + j for j in range(th))
            offs.append(offs[-1] + replicas * len(nodes))
            n_out.append(th)
        return {"fan_in": fan_in, "in_idx": np.array(in_idx, np.int32).reshape(-1, fan_in), "weights": np.array(weights, np.int32).reshape(-1, fan_in),
                "cst": np.array(cst, np.uint32), "lut_idx": np.array(lut_idx, np.int32), "wave_offsets": np.array(offs, np.int32),
                "wave_n_out": np.array(n_out, np.int32), "out_idx": np.array(out_idx, np.int32), "num_wires": replicas * W}


class LutCircuitRunner(_Handle):
    """Runs `replicas` independent instances of a LutNetlist on one Engine as ONE recorded circuit.  Wire table: int32[replicas * num_wires][n+1]
    in HBM; the inputs of replica r are rows r * num_wires + 0 .. num_inputs - 1.  Given the lvl1 key key1, the tables are encrypted under it
    (rustfhe_amd.encrypt_lut; seed: TEST-ONLY deterministic encryption) and the circuit holds them only as ciphertexts (Engine.lut_encrypted).
    rounded=True records the circuit with the rounded gadget decomposition (Engine.set_decomposition): the engine's mode is set around the
    recording and restored after it; the circuit replays in the mode it was recorded in."""
    _slot = "_circuit"      # the recorded circuit, once launch() has made it

    def __init__(self, engine, net, replicas=1, key1=None, seed=None, rounded=False):
        import torch
        self.e, self.net, self.R = engine, net, replicas
        self._destroy = engine.circuit_destroy
        self.key1, self.seed = key1, seed
        self.rounded = bool(rounded)
        self.n1 = engine.p.n + 1
        self.wires = torch.zeros((replicas * net.num_wires, self.n1), dtype=torch.int32, device="cuda")
        self.desc = net.arrays(replicas)
        self._circuit = None

    def set_inputs(self, cts):
        """cts: uint32[replicas][num_inputs][n+1] (numpy)."""
        import torch
        cts = np.ascontiguousarray(cts, np.uint32).reshape(self.R, self.net.num_inputs, self.n1)
        view = self.wires.view(self.R, self.net.num_wires, self.n1)
        view[:, :self.net.num_inputs] = torch.from_numpy(cts.view(np.int32)).cuda()

    def launch(self, stream=None):
        """One replay, asynchronous on `stream`.  The first call records the circuit; the tables are uploaded for the recording only (the
        circuit keeps its own copy)."""
        if self._circuit is None and self.net.nodes:
            d = self.desc
            tv = self.net.polynomials(self.e.p.N)
            if self.key1 is not None:
                from .client import encrypt_lut
                lut = self.e.lut_encrypted(encrypt_lut(self.e.p, self.key1, tv, self.seed))
            else:
                lut = self.e.lut(tv)
            from . import _ffi
            before = self.e.decomposition()
            with lut:
                self.e.set_decomposition(_ffi.DECOMP_ROUNDED if self.rounded else _ffi.DECOMP_REFERENCE)
                try:
                    self._circuit = self.e.lut_circuit_create(lut, d["fan_in"], d["in_idx"], d["weights"], d["cst"], d["lut_idx"], d["wave_offsets"],
                                                              d["wave_n_out"], d["out_idx"], self.wires, d["num_wires"])
                finally:
                    self.e.set_decomposition(before)
        if self._circuit is not None:
            self.e.circuit_launch(self._circuit, stream)

    def run(self):
        """Replays the circuit on the current stream and waits for it."""
        import torch
        st = torch.cuda.current_stream().cuda_stream
        self.launch(st)
        self.e.sync(st)
        return self

    def outputs(self):
        """uint32[replicas][num_outputs][n+1]."""
        import torch
        view = self.wires.view(self.R, self.net.num_wires, self.n1)
        idx = torch.tensor(self.net.outputs, device="cuda", dtype=torch.long)
        return view[:, idx].cpu().numpy().view(np.uint32)

    def wire(self, w):
        return self.wires.view(self.R, self.net.num_wires, self.n1)[:, w].cpu().numpy().view(np.uint32)


def lut_ripple_adder(bits=8):
    """The adder of examples/pbs_adder.py as a LutNetlist: 2-bit messages, inputs a_0 .. a_{bits-1}, b_0 .. b_{bits-1} (LSB first, each 0 or 1);
    level i sums a_i + b_i + c_i (at most 3) and one theta = 2 node gives the sum bit s & 1 and the carry s >> 1.  Outputs: the sum bits, then the
    carry out.  bits nodes, bits levels."""
    net = LutNetlist(2)
    a = net.inputs(bits)
    b = net.inputs(bits)
    t = net.table([lambda s: s & 1, lambda s: s >> 1])
    carry = None
    for i in range(bits):
        terms = [(a[i], 1), (b[i], 1)] + ([(carry, 1)] if carry is not None else [])
        s, carry = net.node(terms, 0, t)
        net.output(s)
    net.output(carry)
    return net
