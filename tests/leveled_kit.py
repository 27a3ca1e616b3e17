"""TEST INFRASTRUCTURE: the drivers of the leveled entry points that more than one GPU test module uses -- the CMUX tree's lookups, oracle
memo and _dev form (tests/test_gpu_cmux_tree.py, tests/test_gpu_leveled_round.py, tests/test_gpu_skipped_gates.py), the TRGSW rotation's
_dev form and one replay of a CMUX netlist (their own modules and tests/test_gpu_leveled_round.py).  A `w` is the world of the calling
module's fixture: an engine, its selector set and tables, the oracle's parameters and spectra."""
import types

import numpy as np

from gpu_kit import memo, to_device, words_of
from kit import SMALL_N
from leveled_oracle import as_trlwe, oracle_cmux_tree
from pbs_oracle import bk_fft

TREE_N_SEL = 37 * 4          # sel_idx = NULL at depth 4 and 37 lookups reads selectors 0 .. 147
TREE_N_ROWS = 16 + 7         # row0 up to 7 at depth 4


def selector_world(orc, N, key_seed, rng_seed, n_sel, sel_seed, known=(0, 1), n=None):
    """What every leveled world starts with: keys from the product's keygen at the stage tests' n (or at `n`), the oracle's parameters and plan, n_sel
    selectors of random bits (the first ones `known`) as torus words and as the oracle's spectra of them.  Returns (w, rng): the module's
    fixture draws its tables and rows from rng next, then creates its engine and handles."""
    import rustfhe_amd as R
    rp = R.Params(n=n or SMALL_N[N], N=N)
    key0, key1, bk, ksk = R.keygen(rp, key_seed)
    w = types.SimpleNamespace(R=R, N=N, logn=N.bit_length() - 1, rp=rp, key0=key0, key1=key1, bk=bk, ksk=ksk)
    w.P = orc.Params(n=rp.n, N=N)
    w.plan = orc.Plan(N)
    rng = np.random.default_rng(rng_seed)
    w.bits = rng.integers(0, 2, n_sel).astype(np.uint8)
    w.bits[:len(known)] = known
    w.sel_t = R.encrypt_selectors(rp, key1, w.bits, seed=sel_seed)
    w.sel_f = bk_fft(orc, w.P, w.plan, w.sel_t.reshape(-1))
    return w, rng


def tree_oracle(orc, w, kind, depth, sel_idx, row0, coef=None):
    """the oracle's tree of every lookup: sel_idx [count][depth], row0 [count], coef [count] or None; computed once per world and arguments,
    shared by the tests that ask for the same lookups, and read-only"""
    def compute():
        rows = as_trlwe(w.rows[kind], w.N)
        return np.stack([oracle_cmux_tree(orc, w.P, w.plan, w.sel_f, sel_idx[g], rows[row0[g]:row0[g] + (1 << depth)],
                                          None if coef is None else coef[g], w.ksk) for g in range(len(row0))])
    return memo(w.oracle_memo, (kind, depth, sel_idx, row0, coef), compute)


def tree_dev(w, kind, depth, count, sel_idx, row0, coef=None, extract=False, on=None):
    """the _dev form on the world's engine, selectors and tables, or on=(engine, selectors, table)"""
    import torch
    eng, sel, lut = on or (w.eng, w.sel, w.lut[kind])
    st = torch.cuda.current_stream().cuda_stream
    if extract:
        d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
        eng.cmux_tree_extract_batch_dev(sel, lut, depth, d_out, count, to_device(sel_idx), to_device(row0), to_device(coef), st)
    else:
        d_out = torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
        eng.cmux_tree_batch_dev(sel, lut, depth, d_out, count, to_device(sel_idx), to_device(row0), st)
    eng.sync(st)
    return words_of(d_out)


def tree_lookups(depth, count):
    """(sel_idx, row0, and what they mean to the oracle) twice: six selectors shared between the lookups with row0 non-zero and differing per
    lookup; then sel_idx = NULL and row0 = NULL"""
    rng = np.random.default_rng(100 * depth + count)
    shared = rng.integers(0, 6, (count, depth)).astype(np.int32)             # six selectors serve every lookup
    rows0 = rng.integers(1, TREE_N_ROWS - (1 << depth) + 1, count).astype(np.int32)
    if count > 1:
        rows0[0], rows0[1] = 1, TREE_N_ROWS - (1 << depth)                   # they differ, and one lookup ends on the table's last row
    default_idx = np.arange(count * depth, dtype=np.int32).reshape(count, depth)
    return (shared, rows0, shared, rows0), (None, None, default_idx, np.zeros(count, np.int32))


def rotate_dev(w, rows, depth, sel_idx, rot, extract=False, on=None, in_place=False):
    """the _dev form on the world's engine and selectors, or on=(engine, selectors)"""
    import torch
    eng, sel = on or (w.eng, w.sel)
    st = torch.cuda.current_stream().cuda_stream
    count = len(rows)
    d_in = to_device(rows, np.uint32)
    if extract:
        d_out = torch.zeros((count, w.rp.n + 1), dtype=torch.int32, device="cuda")
        eng.trgsw_rotate_extract_batch_dev(sel, d_in, depth, d_out, count, to_device(sel_idx), rot, st)
    else:
        d_out = d_in if in_place else torch.zeros((count, 2, w.N), dtype=torch.int32, device="cuda")
        eng.trgsw_rotate_batch_dev(sel, d_in, depth, d_out, count, to_device(sel_idx), rot, st)
    eng.sync(st)
    return words_of(d_out)


def net_run(w, net, lut, count, sel_idx=None, row0=None, on=None, sel=None):
    """records the netlist on the world's engine (or `on`), replays it once and returns d_out's words"""
    import torch
    eng = on or w.eng
    n_out = len(net.outputs)
    shape = (count, n_out, 2, w.N) if net.outputs[0][1] is None else (count, n_out, w.rp.n + 1)
    d_out = torch.zeros(shape, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with eng.cmux_circuit(net, sel or w.sel, lut, d_out, count, to_device(sel_idx), to_device(row0)) as c:
        c.launch(st)
        eng.sync(st)
    return words_of(d_out)
