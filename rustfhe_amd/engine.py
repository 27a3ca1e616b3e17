"""Engine: one rtfhe_ctx (one GPU) behind numpy / torch-device-pointer calls.

Every compute method runs the HIP kernels of librtfhe_hip.so through the C ABI; errors surface as
RtfheError with the library's message.  No CPU path exists in this package.  The key holder's side (key generation, encryption, decryption,
the file formats), which needs no GPU, is client.py.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import AND, ANDNY, COPY, ERR_INVALID, NAND, NOT, OR, XOR, Params  # noqa: F401
from .client import RtfheError, _np, _ptr, _seed


def _stream(stream):
    return C.c_void_p(stream) if stream else None


class _Handle:
    """Owns one handle of the library, kept in the attribute named by _slot, and the function that destroys it (self._destroy, set before the
    handle is): close() frees it once, and so do a with block and garbage collection."""
    _slot = "h"

    def close(self):
        h = getattr(self, self._slot, None)
        if h:
            self._destroy(h)
            setattr(self, self._slot, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def packed_rows(words, L, k):
    """The host side of the upload_*_compressed helpers, checked before any device is touched: compressed rows of L values at k bits as a
    contiguous u32[count][W(L, k)] -- what read_compressed returns goes through as it is, a flat array is cut into rows.  RtfheError for k
    outside 2 .. 32 or a size that is no whole number of rows."""
    k, L = int(k), int(L)
    W = (L * k + 31) // 32
    if not 2 <= k <= 32 or L < 1:
        raise RtfheError(ERR_INVALID, "k = %d is outside 2 .. 32 (or the row is empty)" % k)
    words = _np(words, np.uint32)
    if words.size % W or (words.ndim > 1 and words.shape[-1] != W):
        raise RtfheError(ERR_INVALID, "compressed rows of %d values at k = %d are %d words each; got an array of shape %s" % (L, k, W, words.shape))
    return words.reshape(-1, W)


ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")


def reference_twiddle_file(N):
    """The shipped twiddle tables of the reference build the golden vectors were made with (rustfhe_amd/assets/), or None."""
    path = os.path.join(ASSETS, "twiddles_N%d.bin" % N)
    return path if os.path.exists(path) else None


class Engine(_Handle):
    def __init__(self, params=None, device=0, devices=None, reference_twiddles=True):
        """device: one GPU (rtfhe_ctx_create).  devices=[d0, d1, ...]: one context over several GPUs of the node
        (rtfhe_ctx_create_multi): keys are loaded once and replicated device-to-device, the host-buffer batch calls shard
        contiguous gate ranges over them, the *_dev batch calls shard a batch resident on devices[0]; netlists and stage-level calls stay on devices[0].
        reference_twiddles: the context builds its twiddle tables with this host's libm; when that libm disagrees with the shipped
        tables of the reference build (a few entries may be an ulp apart between libms) the shipped tables are installed
        instead (rtfhe_twiddles_load) and self.twiddle_entries_replaced says how many entries differed.  False: this host's libm as it is."""
        self.L = _ffi.load()
        self._destroy = self.L.rtfhe_ctx_destroy
        self.p = params or Params()
        h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int * len(devices))(*devices)
            rc = self.L.rtfhe_ctx_create_multi(C.byref(self.p), ids, len(devices), C.byref(h))
            device = devices[0] if len(devices) else 0
        else:
            rc = self.L.rtfhe_ctx_create(C.byref(self.p), device, C.byref(h))
        if rc != 0:
            raise RtfheError(rc, (self.L.rtfhe_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self.twiddle_entries_replaced = 0
        path = reference_twiddle_file(self.p.N) if reference_twiddles else None
        if path:
            self.twiddle_entries_replaced = self.twiddles_load(path)

    def twiddles_load(self, path):
        """rtfhe_twiddles_load: installs the file's tables if they differ from the context's; returns the number of differing entries."""
        n = C.c_int32(0)
        self._ck(self.L.rtfhe_twiddles_load(self.h, os.fsencode(path), C.byref(n)))
        return n.value

    def twiddles_write(self, path):
        self._ck(self.L.rtfhe_twiddles_write(self.h, os.fsencode(path)))

    def device_count(self):
        return self.L.rtfhe_ctx_device_count(self.h)

    def _ck(self, rc):
        """Raises RtfheError with the context's message -- or, once the engine is closed (a call made through a handle that outlived it), with
        the calling thread's last one."""
        if rc != 0:
            raise RtfheError(rc, (self.L.rtfhe_last_error(self.h) or b"").decode())

    # ---- keys -------------------------------------------------------------------------------
    def load_bk_torus(self, bk):
        bk = _np(bk, np.uint32).reshape(-1)
        assert bk.size == self.p.bk_words, "bk must be u32[n][2][2l][N]"
        self._ck(self.L.rtfhe_load_bk_torus(self.h, _ptr(bk)))

    def load_bk_seeded(self, seed, b, first_row=0):
        """load_bk_torus from the key's seeded form (rtfhe_load_bk_seeded): b u32[n][2l][N], e.g. encrypt_selectors_seeded(params, key1, key0) --
        half the bytes go up, the masks are made on the device."""
        b = _np(b, np.uint32).reshape(-1)
        assert b.size == self.p.bk_words // 2, "b must be u32[n][2l][N]"
        self._ck(self.L.rtfhe_load_bk_seeded(self.h, _ptr(_seed(seed)), int(first_row), _ptr(b)))

    def load_bk_fft(self, bk_f):
        bk_f = _np(bk_f, np.float64).reshape(-1)
        assert bk_f.size == self.p.bk_words, "bk_f must be f64[n][2][2l][N]"
        self._ck(self.L.rtfhe_load_bk_fft(self.h, _ptr(bk_f)))

    def export_bk_fft(self):
        out = np.empty(self.p.bk_words, np.float64)
        self._ck(self.L.rtfhe_export_bk_fft(self.h, _ptr(out)))
        return out

    def load_ksk(self, ksk):
        ksk = _np(ksk, np.uint32).reshape(-1)
        assert ksk.size == self.p.ksk_words, "ksk must be u32[N][t][base-1][n+1]"
        self._ck(self.L.rtfhe_load_ksk(self.h, _ptr(ksk)))

    def load_ksk_seeded(self, seed, b, first_row=0):
        """load_ksk from the key's seeded form (rtfhe_load_ksk_seeded): b u32[N][t][base-1], one word per row, and the public seed
        (rustfhe_amd.ksk_keygen_seeded) -- 98 KB go up where load_ksk ships 62.5 MB; the masks are made on the device."""
        b = _np(b, np.uint32).reshape(-1)
        assert b.size == self.p.ksk_words // (self.p.n + 1), "b must be u32[N][t][base-1]"
        self._ck(self.L.rtfhe_load_ksk_seeded(self.h, _ptr(_seed(seed)), int(first_row), _ptr(b)))

    def load_ksk_ref(self, ksk_ref):
        """The reference's own shape, KeySwitchingKey(Vec<[[TLWERep; 4]; 8]>) flattened to u32[N][t][base][n+1]
        (hom_nand/src/tlwe.rs:243-245); the never-read entry t = base of every level is dropped by the library."""
        ksk_ref = _np(ksk_ref, np.uint32).reshape(-1)
        base = 1 << self.p.ks_basebit
        assert ksk_ref.size == self.p.ksk_words // (base - 1) * base, "ksk_ref must be u32[N][t][base][n+1]"
        self._ck(self.L.rtfhe_load_ksk_ref(self.h, _ptr(ksk_ref)))

    def set_backend(self, backend):
        self._ck(self.L.rtfhe_set_backend(self.h, backend))

    def backend(self):
        return self.L.rtfhe_get_backend(self.h)

    def set_decomposition(self, mode):
        """The gadget decomposition of the PBS family (pbs_batch*, pbs_many_batch*, LUT circuits at creation): _ffi.DECOMP_REFERENCE (the
        default, the reference's words) or _ffi.DECOMP_ROUNDED (round to nearest, balanced digits: about a fifth of the output noise at
        N = 1024, 4-bit messages).  Gates and every other call always use the reference decomposition."""
        self._ck(self.L.rtfhe_set_decomposition(self.h, mode))

    def decomposition(self):
        return self.L.rtfhe_get_decomposition(self.h)

    def set_leveled_decomposition(self, mode):
        """The gadget decomposition of the leveled calls (cmux_tree_*, trgsw_rotate_*, external_product_batch on the mirror backend, CMUX
        netlists at creation): _ffi.DECOMP_REFERENCE (the default, the reference's words) or _ffi.DECOMP_ROUNDED (round to nearest, balanced
        digits: no systematic error under selector bits that are 1, 6-bit rows through a depth-8 tree and a 10-step rotation).  A second mode,
        independent of set_decomposition's; gates, the PBS family and packing never read it."""
        self._ck(self.L.rtfhe_set_leveled_decomposition(self.h, mode))

    def leveled_decomposition(self):
        return self.L.rtfhe_get_leveled_decomposition(self.h)

    def twiddles(self):
        a = np.zeros(2 * self.p.N, np.float64)
        b = np.zeros(2 * self.p.N, np.float64)
        self._ck(self.L.rtfhe_get_twiddles(self.h, _ptr(a), _ptr(b)))
        return a, b

    def set_twiddles(self, ifft_table, fft_table):
        a, b = _np(ifft_table, np.float64), _np(fft_table, np.float64)
        assert a.size == 2 * self.p.N and b.size == 2 * self.p.N
        self._ck(self.L.rtfhe_set_twiddles(self.h, _ptr(a), _ptr(b)))

    # ---- hot path, host buffers -------------------------------------------------------------
    def gate_batch(self, op, in0, in1=None):
        in0 = _np(in0, np.uint32).reshape(-1, self.p.n + 1)
        if in1 is not None:
            in1 = _np(in1, np.uint32).reshape(-1, self.p.n + 1)
            assert in1.shape == in0.shape
        out = np.empty_like(in0)
        self._ck(self.L.rtfhe_gate_batch(self.h, op, _ptr(in0), _ptr(in1), _ptr(out), in0.shape[0]))
        return out

    def mux_batch(self, c, in0, in1):
        c = _np(c, np.uint32).reshape(-1, self.p.n + 1)
        in0 = _np(in0, np.uint32).reshape(c.shape)
        in1 = _np(in1, np.uint32).reshape(c.shape)
        out = np.empty_like(c)
        self._ck(self.L.rtfhe_mux_batch(self.h, _ptr(c), _ptr(in0), _ptr(in1), _ptr(out), c.shape[0]))
        return out

    def bootstrap_batch(self, tlwe):
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        out = np.empty_like(tlwe)
        self._ck(self.L.rtfhe_bootstrap_batch(self.h, _ptr(tlwe), _ptr(out), tlwe.shape[0]))
        return out

    # ---- hot path, device buffers (torch tensors or raw pointers) ---------------------------
    @staticmethod
    def _dev(t):
        if t is None:
            return None
        if isinstance(t, int):
            return C.c_void_p(t)
        return C.c_void_p(t.data_ptr())

    def gate_batch_dev(self, op, d_in0, d_in1, d_out, count, stream=None):
        self._ck(self.L.rtfhe_gate_batch_dev(self.h, op, self._dev(d_in0), self._dev(d_in1), self._dev(d_out),
                                             count, _stream(stream)))

    def mux_batch_dev(self, d_c, d_in0, d_in1, d_out, count, stream=None):
        self._ck(self.L.rtfhe_mux_batch_dev(self.h, self._dev(d_c), self._dev(d_in0), self._dev(d_in1), self._dev(d_out),
                                            count, _stream(stream)))

    def bootstrap_batch_dev(self, d_tlwe, d_out, count, stream=None):
        self._ck(self.L.rtfhe_bootstrap_batch_dev(self.h, self._dev(d_tlwe), self._dev(d_out), count, _stream(stream)))

    def memory_bytes(self, d=0):
        """Device memory entry d of the context holds right now: keys in every form built so far, staging and scratch (not the twiddle tables, not
        live circuits' sample buffers)."""
        b = C.c_size_t()
        self._ck(self.L.rtfhe_ctx_memory_bytes(self.h, d, C.byref(b)))
        return b.value

    def peer_info(self, d):
        """What the runtime reported about entry d >= 1 of a multi-device context against the primary (peer access both ways, whether enabling it
        worked, link type and hops) and the phases of that entry's share of the last device-resident sharded batch; a dict (rtfhe_peer_info)."""
        info = _ffi.PeerInfo()
        self._ck(self.L.rtfhe_ctx_peer_info(self.h, d, C.byref(info)))
        return info.as_dict()

    def circuit_wave_dev(self, d_ops, d_idx0, d_idx1, d_idx_out, d_wires, num_wires, count, stream=None):
        """One dependency wave of a netlist; wire indices / opcodes are validated on the device against num_wires
        (rows of d_wires) and a violation surfaces as RtfheError at the next sync()."""
        self._ck(self.L.rtfhe_circuit_wave_dev(self.h, self._dev(d_ops), self._dev(d_idx0), self._dev(d_idx1),
                                               self._dev(d_idx_out), self._dev(d_wires), num_wires, count,
                                               _stream(stream)))

    def circuit_create(self, d_ops, d_idx0, d_idx1, d_idx_out, wave_offsets, d_wires, num_wires):
        """Records the waves [wave_offsets[w], wave_offsets[w+1]) of a levelised netlist into one HIP graph; returns a handle
        for circuit_launch / circuit_destroy.  The device arrays must stay alive while the handle exists."""
        offs = _np(wave_offsets, np.int32)
        h = C.c_void_p()
        self._ck(self.L.rtfhe_circuit_create(self.h, self._dev(d_ops), self._dev(d_idx0), self._dev(d_idx1), self._dev(d_idx_out),
                                             offs.ctypes.data_as(C.POINTER(C.c_int32)), offs.size - 1, self._dev(d_wires), num_wires,
                                             C.byref(h)))
        return h

    def lut_circuit_create(self, lut, fan_in, in_idx, weights, cst, lut_idx, wave_offsets, wave_n_out, out_idx, d_wires, num_wires):
        """Records a LUT circuit (include/rtfhe.h: rtfhe_lut_circuit_create): waves of many-LUT bootstraps of weighted wire sums over the wire
        table d_wires (num_wires rows of n+1 words).  The description arrays are host arrays (numpy), copied by the library, and so is the
        table: `lut` may be closed afterwards.  cst / lut_idx may be None.  Returns a handle for circuit_launch / circuit_destroy."""
        i32 = lambda a: None if a is None else _np(a, np.int32).reshape(-1)      # noqa: E731
        in_idx, weights, lut_idx, out_idx = i32(in_idx), i32(weights), i32(lut_idx), i32(out_idx)
        cst = None if cst is None else _np(np.asarray(cst, np.int64) & 0xFFFFFFFF, np.uint32).reshape(-1)
        offs, n_out = i32(wave_offsets), i32(wave_n_out)
        assert n_out.size == offs.size - 1, "one n_out per wave"
        h = C.c_void_p()
        self._ck(self.L.rtfhe_lut_circuit_create(self.h, lut.h, int(fan_in), _ptr(in_idx), _ptr(weights), _ptr(cst), _ptr(lut_idx),
                                                 offs.ctypes.data_as(C.POINTER(C.c_int32)), n_out.ctypes.data_as(C.POINTER(C.c_int32)), n_out.size,
                                                 _ptr(out_idx), self._dev(d_wires), num_wires, C.byref(h)))
        return h

    def circuit_launch(self, circuit, stream=None):
        self._ck(self.L.rtfhe_circuit_launch(circuit, _stream(stream)))

    def circuit_destroy(self, circuit):
        self.L.rtfhe_circuit_destroy(circuit)

    def sync(self, stream=None):
        self._ck(self.L.rtfhe_sync(self.h, _stream(stream)))

    def timer_begin(self, stream=None):
        self._ck(self.L.rtfhe_timer_begin(self.h, _stream(stream)))

    def timer_end(self, stream=None):
        ms, n = C.c_double(), C.c_int64()
        self._ck(self.L.rtfhe_timer_end(self.h, _stream(stream), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timer_end_detail(self, stream=None):
        """(total ms, ms of it inside the batch key switches of the split path, kernel launches)"""
        ms, ks, n = C.c_double(), C.c_double(), C.c_int64()
        self._ck(self.L.rtfhe_timer_end_detail(self.h, _stream(stream), C.byref(ms), C.byref(ks), C.byref(n)))
        return ms.value, ks.value, n.value

    # ---- programmable bootstrapping (include/rtfhe.h: rtfhe_lut_create, rtfhe_pbs_batch[_dev]) -------------------------------
    def lut(self, tv):
        """Uploads test polynomials u32[n_lut][N] (or one u32[N]) to every device of the context; a Lut, closed by Lut.close() or a with block.
        rustfhe_amd.lut_polynomial builds one for a function of a small integer."""
        return Lut(self, tv)

    def lut_encrypted(self, trlwe):
        """Uploads an encrypted table (include/rtfhe.h: rtfhe_lut_create_encrypted): u32[n_lut][2][N] (or one u32[2][N]) TRLWE rows under the
        lvl1 key, e.g. from rustfhe_amd.encrypt_lut.  Returns a Lut (lut.encrypted is True) usable wherever a Lut is."""
        return Lut(self, trlwe, encrypted=True)

    def lut_encrypted_seeded(self, seed, b, first_row=0):
        """lut_encrypted from the table's seeded form (rtfhe_lut_create_encrypted_seeded): b u32[n_lut][N] (or one u32[N]) and the public seed,
        e.g. from rustfhe_amd.encrypt_lut_seeded; row r's mask is row first_row + r of the seed, made on the device."""
        return Lut(self, b, encrypted=True, seeded=(_seed(seed), int(first_row)))

    def pbs_batch(self, lut, tlwe, lut_idx=None):
        """One programmable bootstrap per ciphertext: gate g evaluates table lut_idx[g] (None: table 0).  Indices are checked here:
        one outside [0, n_lut) raises RtfheError before anything runs."""
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        idx = None if lut_idx is None else _np(lut_idx, np.int32).reshape(-1)
        assert idx is None or idx.size == tlwe.shape[0], "one table index per ciphertext"
        out = np.empty_like(tlwe)
        self._ck(self.L.rtfhe_pbs_batch(self.h, lut.h, _ptr(idx), _ptr(tlwe), _ptr(out), tlwe.shape[0]))
        return out

    def pbs_batch_dev(self, lut, d_tlwe, d_out, count, d_lut_idx=None, stream=None):
        """... on device buffers (d_lut_idx: int32[count] on the device or None), asynchronous on `stream`.  Indices are checked on the device:
        a gate with a bad one is skipped and the next sync() raises RtfheError."""
        self._ck(self.L.rtfhe_pbs_batch_dev(self.h, lut.h, self._dev(d_lut_idx), self._dev(d_tlwe), self._dev(d_out), count,
                                            _stream(stream)))

    # ---- multi-bit blind rotation (include/rtfhe.h: rtfhe_mbk_create, rtfhe_pbs_mb_batch[_dev]) ----------------------------------------------
    def multibit_key(self, words, g):
        """Uploads a multi-bit bootstrapping key (rustfhe_amd.mbk_keygen at the same g) to the primary device as spectra; a MultibitKey handle,
        closed by close() or a with block."""
        return MultibitKey(self, words, g)

    def pbs_mb_batch(self, mbk, lut, tlwe, lut_idx=None):
        """pbs_batch through the multi-bit blind rotation: ceil(n / g) dependent steps instead of n, g the key's.  Plain tables only.  The outputs
        decrypt like pbs_batch's; their words differ.  Indices are checked here: a bad one raises RtfheError before anything runs."""
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        idx = None if lut_idx is None else _np(lut_idx, np.int32).reshape(-1)
        assert idx is None or idx.size == tlwe.shape[0], "one table index per ciphertext"
        out = np.empty_like(tlwe)
        self._ck(self.L.rtfhe_pbs_mb_batch(self.h, mbk.h, lut.h, _ptr(idx), _ptr(tlwe), _ptr(out), tlwe.shape[0]))
        return out

    def pbs_mb_batch_dev(self, mbk, lut, d_tlwe, d_out, count, d_lut_idx=None, stream=None):
        """... on device buffers (d_lut_idx: int32[count] on the device or None), asynchronous on `stream`; a gate with a bad index is skipped and
        the next sync() raises.  Inside a stream capture it allocates nothing and needs no earlier call on the stream."""
        self._ck(self.L.rtfhe_pbs_mb_batch_dev(self.h, mbk.h, lut.h, self._dev(d_lut_idx), self._dev(d_tlwe), self._dev(d_out), count, _stream(stream)))

    def pbs_many_batch(self, lut, tlwe, n_out, lut_idx=None):
        """Many-LUT PBS (include/rtfhe.h: rtfhe_pbs_many_batch): n_out (1, 2, 4 or 8) functions of each ciphertext from ONE blind rotation,
        u32[count][n_out][n+1].  Tables interleave the functions (rustfhe_amd.many_lut_polynomial); indices are checked as in pbs_batch."""
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        idx = None if lut_idx is None else _np(lut_idx, np.int32).reshape(-1)
        assert idx is None or idx.size == tlwe.shape[0], "one table index per ciphertext"
        out = np.empty((tlwe.shape[0], max(int(n_out), 0), self.p.n + 1), np.uint32)
        self._ck(self.L.rtfhe_pbs_many_batch(self.h, lut.h, int(n_out), _ptr(idx), _ptr(tlwe), _ptr(out), tlwe.shape[0]))
        return out

    def pbs_many_batch_dev(self, lut, d_tlwe, d_out, count, n_out, d_lut_idx=None, stream=None):
        """... on device buffers (d_out: [count][n_out][n+1] words), asynchronous on `stream`; bad indices are reported by the next sync().
        Inside a stream capture an eager call of at least `count` gates and this n_out must have run on the stream first."""
        self._ck(self.L.rtfhe_pbs_many_batch_dev(self.h, lut.h, int(n_out), self._dev(d_lut_idx), self._dev(d_tlwe), self._dev(d_out), count,
                                                 _stream(stream)))

    # ---- CMUX-tree table lookup (include/rtfhe.h: rtfhe_trgsw_create, rtfhe_cmux_tree_batch[_dev], rtfhe_cmux_tree_extract_batch[_dev]) ------
    def selectors(self, trgsw):
        """Uploads TRGSW samples u32[n_sel][2][2l][N] (or one u32[2][2l][N]) under the lvl1 key, e.g. from rustfhe_amd.encrypt_selectors, and
        converts them to spectra on the primary device; a Selectors handle, closed by close() or a with block."""
        return Selectors(self, trgsw)

    def selectors_seeded(self, seed, b, first_row=0):
        """selectors from the set's seeded form (rtfhe_trgsw_create_seeded): b u32[n_sel][2l][N] (or one u32[2l][N]) and the public seed, e.g. from
        rustfhe_amd.encrypt_selectors_seeded / encrypt_trgsw_polys_seeded -- half the bytes go up, the masks are made on the device."""
        return Selectors(self, b, seeded=(_seed(seed), int(first_row)))

    def seeded_expand_dev(self, seed, d_b, group, d_out, rows, first_row=0, stream=None):
        """One launch (rtfhe_seeded_expand_dev): d_out [rows / group][2][group][N] words = the b halves d_b [rows][N] and the masks of rows
        first_row .. first_row + rows - 1 of the seed; what rustfhe_amd.seeded_expand computes on the CPU.  Asynchronous on `stream`, nothing
        allocated: it may be captured first thing on a fresh stream.  The buffers must be 16-byte aligned and must not overlap."""
        self._ck(self.L.rtfhe_seeded_expand_dev(self.h, _ptr(_seed(seed)), int(first_row), self._dev(d_b), int(group), self._dev(d_out), int(rows),
                                                _stream(stream)))

    def _tree_args(self, sel_idx, depth, row0, coef, count):
        i32 = lambda a, shape: None if a is None else _np(a, np.int32).reshape(shape)      # noqa: E731
        return i32(sel_idx, (count, depth)), i32(row0, (count,)), i32(coef, (count,))

    def cmux_tree_batch(self, sel, lut, depth, count, sel_idx=None, row0=None):
        """`count` lookups of depth `depth`: lookup g selects row row0[g] + (address bits sel_idx[g][0 .. depth), least significant first) of
        `lut` (plain or encrypted) with 2^depth - 1 CMUXes; u32[count][2][N] TRLWE rows (b then a).  sel_idx None: lookup g uses selectors
        g * depth + k; row0 None: 0.  Indices are checked here: a bad one raises RtfheError before anything runs."""
        idx, r0, _ = self._tree_args(sel_idx, depth, row0, None, count)
        out = np.empty((count, 2, self.p.N), np.uint32)
        self._ck(self.L.rtfhe_cmux_tree_batch(self.h, sel.h, _ptr(idx), int(depth), lut.h, _ptr(r0), _ptr(out), count))
        return out

    def cmux_tree_batch_dev(self, sel, lut, depth, d_out, count, d_sel_idx=None, d_row0=None, stream=None):
        """... on device buffers (d_sel_idx: int32[count][depth], d_row0: int32[count], d_out: [count][2][N] words), asynchronous on `stream`;
        bad indices are reported by the next sync().  Inside a stream capture an eager call of at least this count and depth must have run
        on the stream first."""
        self._ck(self.L.rtfhe_cmux_tree_batch_dev(self.h, sel.h, self._dev(d_sel_idx), int(depth), lut.h, self._dev(d_row0), self._dev(d_out), count,
                                                  _stream(stream)))

    def cmux_tree_extract_batch(self, sel, lut, depth, count, sel_idx=None, row0=None, coef=None):
        """The same tree followed by sample extract at coefficient coef[g] (None: 0) and the key switch: u32[count][n+1] lvl0 ciphertexts of
        that coefficient of the selected row.  Needs the key-switching key, not the bootstrapping key."""
        idx, r0, cf = self._tree_args(sel_idx, depth, row0, coef, count)
        out = np.empty((count, self.p.n + 1), np.uint32)
        self._ck(self.L.rtfhe_cmux_tree_extract_batch(self.h, sel.h, _ptr(idx), int(depth), lut.h, _ptr(r0), _ptr(cf), _ptr(out), count))
        return out

    def cmux_tree_extract_batch_dev(self, sel, lut, depth, d_out, count, d_sel_idx=None, d_row0=None, d_coef=None, stream=None):
        """... on device buffers (d_out: [count][n+1] words), under cmux_tree_batch_dev's rules."""
        self._ck(self.L.rtfhe_cmux_tree_extract_batch_dev(self.h, sel.h, self._dev(d_sel_idx), int(depth), lut.h, self._dev(d_row0), self._dev(d_coef),
                                                          self._dev(d_out), count, _stream(stream)))

    # ---- TRGSW blind rotation (include/rtfhe.h: rtfhe_trgsw_rotate_batch[_dev], rtfhe_trgsw_rotate_extract_batch[_dev]) ------------------------
    def _rot_arg(self, rot, depth):
        if rot is None:
            return None
        rot = _np(rot, np.int32).reshape(-1)
        assert rot.size == int(depth), "one exponent per step"
        return rot

    def trgsw_rotate_batch(self, sel, trlwe, depth, sel_idx=None, rot=None):
        """One rotation per TRLWE of u32[count][2][N]: depth steps acc <- cmux(S_k, X^rot[k] * acc, acc) with S_k = selector sel_idx[g][k] (None:
        g * depth + k) and the exponents rot[0 .. depth) in [0, 2N) shared by the batch (None: 2N - 2^k, so that address bits in S_k give
        X^-addr * trlwe[g]); u32[count][2][N].  Indices and exponents are checked here: a bad one raises RtfheError before anything runs."""
        trlwe = _np(trlwe, np.uint32).reshape(-1, 2, self.p.N)
        count = trlwe.shape[0]
        idx = None if sel_idx is None else _np(sel_idx, np.int32).reshape(count, depth)
        r = self._rot_arg(rot, depth)
        out = np.empty_like(trlwe)
        self._ck(self.L.rtfhe_trgsw_rotate_batch(self.h, sel.h, _ptr(idx), int(depth), _ptr(r), _ptr(trlwe), _ptr(out), count))
        return out

    def trgsw_rotate_batch_dev(self, sel, d_trlwe, depth, d_out, count, d_sel_idx=None, rot=None, stream=None):
        """... on device buffers (d_trlwe, d_out: [count][2][N] words, d_out may be d_trlwe; d_sel_idx: int32[count][depth]; rot stays a host
        array, copied at enqueue time), asynchronous on `stream`; a lookup with a bad index is skipped, its output row untouched, and the next
        sync() raises.  Allocates nothing: it may be captured without a prior eager call."""
        r = self._rot_arg(rot, depth)
        self._ck(self.L.rtfhe_trgsw_rotate_batch_dev(self.h, sel.h, self._dev(d_sel_idx), int(depth), _ptr(r), self._dev(d_trlwe), self._dev(d_out), count,
                                                     _stream(stream)))

    def trgsw_rotate_extract_batch(self, sel, trlwe, depth, sel_idx=None, rot=None):
        """The same rotation followed by sample extract at coefficient 0 and the key switch: u32[count][n+1] lvl0 ciphertexts.  With rot None
        and address bits in the selectors that is coefficient addr of each row.  Needs the key-switching key, not the bootstrapping key."""
        trlwe = _np(trlwe, np.uint32).reshape(-1, 2, self.p.N)
        count = trlwe.shape[0]
        idx = None if sel_idx is None else _np(sel_idx, np.int32).reshape(count, depth)
        r = self._rot_arg(rot, depth)
        out = np.empty((count, self.p.n + 1), np.uint32)
        self._ck(self.L.rtfhe_trgsw_rotate_extract_batch(self.h, sel.h, _ptr(idx), int(depth), _ptr(r), _ptr(trlwe), _ptr(out), count))
        return out

    def trgsw_rotate_extract_batch_dev(self, sel, d_trlwe, depth, d_out, count, d_sel_idx=None, rot=None, stream=None):
        """... on device buffers (d_out: [count][n+1] words).  Inside a stream capture an eager call of at least this count must have run on the
        stream first."""
        r = self._rot_arg(rot, depth)
        self._ck(self.L.rtfhe_trgsw_rotate_extract_batch_dev(self.h, sel.h, self._dev(d_sel_idx), int(depth), _ptr(r), self._dev(d_trlwe), self._dev(d_out),
                                                             count, _stream(stream)))

    # ---- CMUX demultiplexer tree (include/rtfhe.h: rtfhe_demux_tree_batch[_dev], rtfhe_lut_accumulate_dev) --------------------------------------
    def demux_tree_batch(self, sel, x, depth, sel_idx=None):
        """One demultiplexer per TRLWE of u32[count][2][N] (a plain polynomial tv goes in as the trivial (tv, 0)): leaf (address bits
        sel_idx[g][0 .. depth), least significant first; None: selectors g * depth + k) of the 2^depth leaves is a TRLWE of x[g]'s message,
        every other leaf a TRLWE of 0; u32[count][2^depth][2][N].  Level t splits on selector demux_level_selector(depth, t) = depth - 1 - t,
        the one cmux_tree_batch's level depth - 1 - t joins on: cmux_tree_batch over the leaves with the same selectors gives x[g] back.
        Indices are checked here: a bad one raises RtfheError before anything runs."""
        x = _np(x, np.uint32).reshape(-1, 2, self.p.N)
        count = x.shape[0]
        idx = None if sel_idx is None else _np(sel_idx, np.int32).reshape(count, depth)
        out = np.empty((count, 1 << int(depth) if 1 <= int(depth) <= 16 else 1, 2, self.p.N), np.uint32)      # (a bad depth is refused by the library)
        self._ck(self.L.rtfhe_demux_tree_batch(self.h, sel.h, _ptr(idx), int(depth), _ptr(x), _ptr(out), count))
        return out

    def demux_tree_batch_dev(self, sel, d_x, depth, d_out, count, d_sel_idx=None, stream=None):
        """... on device buffers (d_x: [count][2][N] words, d_out: [count][2^depth][2][N] words, not overlapping; d_sel_idx:
        int32[count][depth]), asynchronous on `stream`; a lookup with a bad index is skipped, its 2^depth output rows untouched, and the next
        sync() raises.  Inside a stream capture an eager call of at least this count and depth must have run on the stream first (depth 1
        needs none)."""
        self._ck(self.L.rtfhe_demux_tree_batch_dev(self.h, sel.h, self._dev(d_sel_idx), int(depth), self._dev(d_x), self._dev(d_out), count,
                                                   _stream(stream)))

    # ---- CMUX netlists (include/rtfhe.h: rtfhe_cmux_circuit_create; rustfhe_amd.cmux_net) -----------------------------------------------------
    def cmux_circuit(self, netlist, sel, lut, d_out, count, d_sel_idx=None, d_row0=None, rounded=None):
        """Records `count` replicas of a CmuxNetlist over the selector set `sel` and the table `lut` into one graph.  d_out: device buffer
        [count][n_out][2][N] words, or [count][n_out][n+1] when the netlist's outputs carry coefficients; d_sel_idx: int32[count][n_vars] on
        the device (None: replica g uses selectors g * n_vars + v); d_row0: int32[count] (None: 0).  The description is checked here: a bad
        node or output raises RtfheError before anything is allocated.  rounded: None records the leveled decomposition in force
        (set_leveled_decomposition), True / False set it around the recording and restore it; the circuit replays in the mode it was recorded
        in.  Returns a CmuxCircuit: launch(stream), close()."""
        from .cmux_net import CmuxCircuit
        return CmuxCircuit(self, netlist, sel, lut, d_out, count, d_sel_idx, d_row0, rounded)

    # ---- packing key switch (include/rtfhe.h: rtfhe_packing_key_create, rtfhe_pack_batch[_dev], rtfhe_lut_update_dev) --------------------------
    def packing_key(self, pk):
        """Uploads a packing key u32[n][t][base-1][2][N] (rustfhe_amd.packing_keygen) to the primary device in the operand order of the matrix
        pipe; a PackingKey handle, closed by close() or a with block."""
        return PackingKey(self, pk)

    def tlwe_seeded_expand_dev(self, seed, d_b, d_out, rows, first_row=0, stream=None):
        """One launch (rtfhe_tlwe_seeded_expand_dev): d_out [rows][n+1] words = the masks of rows first_row .. first_row + rows - 1 of the seed in
        columns 0 .. n - 1 and d_b [rows] in column n; what rustfhe_amd.tlwe_seeded_expand computes on the CPU.  d_out needs 4-byte alignment only:
        it may be a range of rows of a larger wire table.  Asynchronous on `stream`, nothing allocated, capturable first thing on a fresh stream."""
        self._ck(self.L.rtfhe_tlwe_seeded_expand_dev(self.h, _ptr(_seed(seed)), int(first_row), self._dev(d_b), self._dev(d_out), int(rows),
                                                     _stream(stream)))

    def upload_tlwe_seeded(self, seed, b, first_row=0):
        """Seeded lvl0 inputs (rustfhe_amd.encrypt_bits_seeded / encrypt_torus_seeded) to the device: copies b u32[rows] up, expands it there and
        returns the int32 device tensor [rows][n+1] the *_dev batch calls read -- 4 bytes per row cross the bus, not 4 (n + 1).  Queued on torch's
        current stream."""
        import torch
        b = _np(b, np.uint32).reshape(-1)
        with torch.cuda.device(self.device):
            d_b = torch.from_numpy(b.view(np.int32)).cuda()
            d_out = torch.empty((b.size, self.p.n + 1), dtype=torch.int32, device="cuda")
            self.tlwe_seeded_expand_dev(seed, d_b, d_out, b.size, first_row, torch.cuda.current_stream().cuda_stream)
        return d_out

    def packing_key_seeded(self, seed, b, first_row=0):
        """packing_key from the key's seeded form (rtfhe_packing_key_create_seeded): b u32[n][t][base-1][N] and the public seed
        (rustfhe_amd.packing_keygen_seeded)."""
        return PackingKey(self, b, seeded=(_seed(seed), int(first_row)))

    def _pos_arg(self, pos, P):
        if pos is None:
            return None
        pos = _np(pos, np.int32).reshape(-1)
        assert pos.size == int(P), "one position per sample"
        return pos

    def pack_batch(self, pk, tlwe, P, rep=1, pos=None):
        """Packs lvl0 ciphertexts u32[count][P][n+1] into TRLWE rows u32[count][2][N] (b then a): output g is the sum over p of
        X^pos[p] * (1 + X + .. + X^(rep-1)) * key_switch(tlwe[g][p]), i.e. the phase of tlwe[g][p] on coefficients pos[p] .. pos[p] + rep - 1
        (negacyclic).  pos None: p * rep.  rustfhe_amd.lut_pack_layout gives the (pos, rep) of a PBS table.  Arguments are checked here: a bad
        one raises RtfheError before anything runs."""
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        P = int(P)
        count = tlwe.shape[0] // P if P > 0 else tlwe.shape[0]
        assert P <= 0 or tlwe.shape[0] == count * P, "P ciphertexts per output"
        out = np.empty((count, 2, self.p.N), np.uint32)
        self._ck(self.L.rtfhe_pack_batch(self.h, pk.h, _ptr(tlwe), P, _ptr(self._pos_arg(pos, P)), int(rep), _ptr(out), count))
        return out

    def pack_batch_dev(self, pk, d_tlwe, P, d_out, count, rep=1, pos=None, stream=None):
        """... on device buffers (d_tlwe: [count][P][n+1] words, d_out: [count][2][N] words; pos stays a host array, copied at enqueue time),
        asynchronous on `stream`.  Inside a stream capture an eager call of at least count * P samples must have run on the stream first."""
        self._ck(self.L.rtfhe_pack_batch_dev(self.h, pk.h, self._dev(d_tlwe), int(P), _ptr(self._pos_arg(pos, P)), int(rep), self._dev(d_out), count,
                                             _stream(stream)))

    # ---- TRLWE sample extraction (include/rtfhe.h: rtfhe_trlwe_extract_batch[_dev], rtfhe_trlwe_extract_lvl1_batch[_dev]) ----------------------
    def _coef_arg(self, coef, P):
        if coef is None:
            return None
        coef = _np(coef, np.int32).reshape(-1)
        assert coef.size == int(P), "one coefficient per sample"
        return coef

    def trlwe_extract_batch(self, trlwe, P, coef=None, stride=1):
        """Coefficients coef[0 .. P) (None: p * stride) of every TRLWE of u32[count][2][N] (b then a) as lvl0 ciphertexts u32[count][P][n+1]:
        sample extract at coef[p], then the key switch -- pack_batch the other way.  Needs the key-switching key, not the bootstrapping key.
        Arguments are checked here: a bad one raises RtfheError before anything runs."""
        trlwe = _np(trlwe, np.uint32).reshape(-1, 2, self.p.N)
        P = int(P)
        out = np.empty((trlwe.shape[0], max(P, 0), self.p.n + 1), np.uint32)
        self._ck(self.L.rtfhe_trlwe_extract_batch(self.h, _ptr(trlwe), P, _ptr(self._coef_arg(coef, P)), int(stride), _ptr(out), trlwe.shape[0]))
        return out

    def trlwe_extract_batch_dev(self, d_trlwe, P, d_out, count, coef=None, stride=1, stream=None):
        """... on device buffers (d_trlwe: [count][2][N] words, d_out: [count][P][n+1] words, not overlapping; coef stays a host array, copied at
        enqueue time), asynchronous on `stream`.  Inside a stream capture an eager call of at least count * P samples must have run on the
        stream first."""
        self._ck(self.L.rtfhe_trlwe_extract_batch_dev(self.h, self._dev(d_trlwe), int(P), _ptr(self._coef_arg(coef, P)), int(stride), self._dev(d_out), count,
                                                      _stream(stream)))

    def trlwe_extract_lvl1_batch(self, trlwe, P, coef=None, stride=1):
        """The same samples before the key switch: lvl1 samples u32[count][P][N+1] (a'[0..N), b'), the input layout of key_switch_batch.  Needs
        no key at all."""
        trlwe = _np(trlwe, np.uint32).reshape(-1, 2, self.p.N)
        P = int(P)
        out = np.empty((trlwe.shape[0], max(P, 0), self.p.N + 1), np.uint32)
        self._ck(self.L.rtfhe_trlwe_extract_lvl1_batch(self.h, _ptr(trlwe), P, _ptr(self._coef_arg(coef, P)), int(stride), _ptr(out), trlwe.shape[0]))
        return out

    def trlwe_extract_lvl1_batch_dev(self, d_trlwe, P, d_out, count, coef=None, stride=1, stream=None):
        """... on device buffers (d_out: [count][P][N+1] words).  Allocates nothing: it may be captured without a prior eager call."""
        self._ck(self.L.rtfhe_trlwe_extract_lvl1_batch_dev(self.h, self._dev(d_trlwe), int(P), _ptr(self._coef_arg(coef, P)), int(stride), self._dev(d_out),
                                                           count, _stream(stream)))

    # ---- compressed results (include/rtfhe.h: rtfhe_tlwe_compress_batch_dev, rtfhe_trlwe_compress_batch_dev) ---------------------------------------
    def tlwe_compress_dev(self, d_tlwe, k, d_out, count, stream=None):
        """lvl0 rows on the device ([count][n+1] words) -> d_out u32[count][W(n+1, k)], every word rounded to its top k bits and bit-packed
        (rustfhe_amd.compressed_words gives W, rustfhe_amd.tlwe_expand undoes it on the CPU).  One launch, asynchronous on `stream`, no key, every
        backend; allocates nothing: it may be captured first thing on a fresh stream.  d_out must not overlap d_tlwe."""
        self._ck(self.L.rtfhe_tlwe_compress_batch_dev(self.h, int(k), self._dev(d_tlwe), self._dev(d_out), count, _stream(stream)))

    def trlwe_compress_dev(self, d_trlwe, k, P, d_out, count, coef=None, stride=1, stream=None):
        """TRLWE rows on the device ([count][2][N] words, b then a) -> d_out u32[count][W(N+P, k)]: the a polynomial and b at the P kept
        coefficients coef (a host array, copied at enqueue time; None: p * stride), rounded and bit-packed; rustfhe_amd.trlwe_expand undoes it on
        the CPU.  Asynchronous on `stream`, no key, every backend, nothing allocated."""
        coef = self._coef_arg(coef, P)      # (kept in a name: _ptr holds an address, not the array)
        self._ck(self.L.rtfhe_trlwe_compress_batch_dev(self.h, int(k), self._dev(d_trlwe), int(P), _ptr(coef), int(stride), self._dev(d_out), count,
                                                       _stream(stream)))

    # ---- ... and back on the device (include/rtfhe.h: rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev) ------------------------------------
    def tlwe_expand_dev(self, d_words, k, d_out, count, stream=None):
        """Packed lvl0 rows on the device (u32[count][W(n+1, k)]) -> d_out [count][n+1] words, each value back at the top of its word: what
        rustfhe_amd.tlwe_expand computes on the CPU.  One launch, asynchronous on `stream`, no key, every backend, nothing allocated; writes
        exactly count * (n + 1) words, so d_out may be a range of rows of a larger wire table (4-byte alignment is all it needs)."""
        self._ck(self.L.rtfhe_tlwe_expand_batch_dev(self.h, int(k), self._dev(d_words), self._dev(d_out), count, _stream(stream)))

    def trlwe_expand_dev(self, d_words, k, P, d_out, count, coef=None, stride=1, stream=None):
        """Packed TRLWE rows on the device (u32[count][W(N+P, k)]) -> d_out [count][2][N] words (b then a): the a polynomial, b at the P kept
        coefficients coef (a host array, copied at enqueue time; None: p * stride; duplicates: the later entry wins) and zero everywhere else --
        rustfhe_amd.trlwe_expand on the GPU.  One launch (with a list at N = 2048: two), asynchronous on `stream`, nothing allocated."""
        coef = self._coef_arg(coef, P)      # (kept in a name: _ptr holds an address, not the array)
        self._ck(self.L.rtfhe_trlwe_expand_batch_dev(self.h, int(k), self._dev(d_words), int(P), _ptr(coef), int(stride), self._dev(d_out), count,
                                                     _stream(stream)))

    def _upload_compressed(self, words, row_words, expand):
        """what both upload helpers do with their checked rows: copy them up, expand(d_words, d_out, count, stream) on torch's current stream"""
        import torch
        with torch.cuda.device(self.device):
            d_words = torch.from_numpy(words.view(np.int32)).cuda()
            d_out = torch.empty((words.shape[0],) + tuple(row_words), dtype=torch.int32, device="cuda")
            if words.shape[0]:
                expand(d_words, d_out, words.shape[0], torch.cuda.current_stream().cuda_stream)
        return d_out

    def upload_tlwe_compressed(self, words, k):
        """Compressed lvl0 rows (tlwe_compress, Engine.tlwe_compress_dev, read_compressed) to the device: copies u32[count][W(n+1, k)] up,
        expands it there and returns the int32 device tensor [count][n+1] the *_dev batch calls read -- 796 bytes per row cross the bus at
        k = 10, not 2,544.  Queued on torch's current stream."""
        words = packed_rows(words, self.p.n + 1, k)
        return self._upload_compressed(words, (self.p.n + 1,), lambda d_w, d_out, count, st: self.tlwe_expand_dev(d_w, k, d_out, count, st))

    def upload_trlwe_compressed(self, words, k, P, coef=None, stride=1):
        """Compressed TRLWE rows to the device: copies u32[count][W(N+P, k)] up, expands it there and returns the int32 device tensor
        [count][2][N] that trlwe_extract_batch_dev, Lut.update_dev and the leveled calls read.  coef / stride as in trlwe_compress_dev --
        read_compressed's (words, k, _, N, coef) go in as upload_trlwe_compressed(words, k, len(coef), coef)."""
        P = int(P)
        if not 1 <= P <= self.p.N:
            raise RtfheError(ERR_INVALID, "P = %d is outside 1 .. N = %d" % (P, self.p.N))
        coef = self._coef_arg(coef, P)
        words = packed_rows(words, self.p.N + P, k)
        return self._upload_compressed(words, (2, self.p.N),
                                       lambda d_w, d_out, count, st: self.trlwe_expand_dev(d_w, k, P, d_out, count, coef, stride, st))

    # ---- exact TRLWE x plain-polynomial products (include/rtfhe.h: rtfhe_plain_create, rtfhe_trlwe_mul_plain_batch[_dev]) --------------------------
    def plain_polys(self, w):
        """Transforms integer polynomials int32[n_w][N] once and keeps them as spectra on the primary device; a PlainPolys handle (.n polynomials,
        .wmax = the largest l1 norm among them), closed by close() or a with block.  Needs no key."""
        return PlainPolys(self, w)

    def _term_idx(self, idx, count, K):
        return None if idx is None else _np(idx, np.int32).reshape(count, K)

    def trlwe_mul_plain_batch(self, pp, x, K=1, w_idx=None, x_idx=None, acc=None):
        """out[g] = (acc[g] if acc is given else 0) + sum_{k < K} pp[w_idx[g][k]] * x[x_idx[g][k]] in Z_2^32[X]/(X^N + 1), on both polynomials of
        every TRLWE row: u32[count][2][N], exact word for word.  x: u32[n_x][2][N].  w_idx None: polynomial k for every g; x_idx None: row
        g * K + k.  count comes from an index array or acc when one is given, else it is n_x // K.  A call is accepted iff
        K * pp.wmax <= 192 N and 1 <= K <= 8.  Arguments are checked here: a bad one raises RtfheError before anything runs."""
        x = _np(x, np.uint32).reshape(-1, 2, self.p.N)
        K = int(K)
        Kd = K if K > 0 else 1
        if w_idx is not None:
            count = np.asarray(w_idx).size // Kd
        elif x_idx is not None:
            count = np.asarray(x_idx).size // Kd
        elif acc is not None:
            count = np.asarray(acc).size // (2 * self.p.N)
        else:
            count = x.shape[0] // Kd
        wi, xi = self._term_idx(w_idx, count, Kd), self._term_idx(x_idx, count, Kd)
        out = np.array(_np(acc, np.uint32).reshape(count, 2, self.p.N)) if acc is not None else np.empty((count, 2, self.p.N), np.uint32)
        self._ck(self.L.rtfhe_trlwe_mul_plain_batch(self.h, pp.h, _ptr(wi), _ptr(x), x.shape[0], _ptr(xi), K, 1 if acc is not None else 0, _ptr(out), count))
        return out

    def trlwe_mul_plain_batch_dev(self, pp, d_x, n_x, d_out, count, K=1, d_w_idx=None, d_x_idx=None, accumulate=False, stream=None):
        """... on device buffers (d_x: [n_x][2][N] words, d_out: [count][2][N] words, not overlapping; d_w_idx / d_x_idx: int32[count][K] on the
        device), asynchronous on `stream`; accumulate adds into d_out.  A sample with a bad index is skipped, its output row untouched, and the
        next sync() raises.  One launch, nothing allocated: it may be captured first thing on a fresh stream."""
        self._ck(self.L.rtfhe_trlwe_mul_plain_batch_dev(self.h, pp.h, self._dev(d_w_idx), self._dev(d_x), int(n_x), self._dev(d_x_idx), int(K),
                                                        1 if accumulate else 0, self._dev(d_out), count, _stream(stream)))

    # ---- TRLWE x TRGSW multiply-accumulate (include/rtfhe.h: rtfhe_trlwe_mul_trgsw_batch[_dev]) -----------------------------------------------------
    def trlwe_mul_trgsw_batch(self, sel, x, K=1, s_idx=None, x_idx=None, acc=None):
        """out[g] = (acc[g] if acc is given else 0) + sum_{k < K} sel[s_idx[g][k]] (.) x[x_idx[g][k]], the external products summed in the
        frequency domain (one pair of inverse transforms, one truncation): u32[count][2][N].  x: u32[n_x][2][N].  s_idx None: selector
        g * K + k; x_idx None: row g * K + k.  count comes from an index array or acc when one is given, else it is n_x // K.  1 <= K <= 8;
        FP64 mirror backend, in the leveled decomposition in force now; needs no key.  Arguments are checked here: a bad one raises RtfheError
        before anything runs."""
        x = _np(x, np.uint32).reshape(-1, 2, self.p.N)
        K = int(K)
        Kd = K if K > 0 else 1
        if s_idx is not None:
            count = np.asarray(s_idx).size // Kd
        elif x_idx is not None:
            count = np.asarray(x_idx).size // Kd
        elif acc is not None:
            count = np.asarray(acc).size // (2 * self.p.N)
        else:
            count = x.shape[0] // Kd
        si, xi = self._term_idx(s_idx, count, Kd), self._term_idx(x_idx, count, Kd)
        out = np.array(_np(acc, np.uint32).reshape(count, 2, self.p.N)) if acc is not None else np.empty((count, 2, self.p.N), np.uint32)
        self._ck(self.L.rtfhe_trlwe_mul_trgsw_batch(self.h, sel.h, _ptr(si), _ptr(x), x.shape[0], _ptr(xi), K, 1 if acc is not None else 0, _ptr(out), count))
        return out

    def trlwe_mul_trgsw_batch_dev(self, sel, d_x, n_x, d_out, count, K=1, d_s_idx=None, d_x_idx=None, accumulate=False, stream=None):
        """... on device buffers (d_x: [n_x][2][N] words, d_out: [count][2][N] words, not overlapping; d_s_idx / d_x_idx: int32[count][K] on the
        device), asynchronous on `stream`; accumulate adds into d_out.  A sample with a bad index is skipped, its output row untouched, and the
        next sync() raises.  One launch, nothing allocated: it may be captured first thing on a fresh stream."""
        self._ck(self.L.rtfhe_trlwe_mul_trgsw_batch_dev(self.h, sel.h, self._dev(d_s_idx), self._dev(d_x), int(n_x), self._dev(d_x_idx), int(K),
                                                        1 if accumulate else 0, self._dev(d_out), count, _stream(stream)))

    # ---- TRLWE key switching (include/rtfhe.h: rtfhe_trlwe_ksk_create, rtfhe_trlwe_auto_batch[_dev]) ------------------------------------------------
    def trlwe_switch_key(self, words, t):
        """Keeps a TRLWE switching key (client.trlwe_ksk_keygen: u32[n_t][l][2][N]) for the exponents t as spectra on the primary device; a
        TrlweSwitchKey handle (.t, the exponents; .n entries), closed by close() or a with block.  Needs no key of the context."""
        return TrlweSwitchKey(self, words, t)

    @staticmethod
    def _program(entry, add):
        entry = _np(entry, np.int32).reshape(-1)
        add = None if add is None else _np(add, np.int32).reshape(-1)
        if add is not None and add.size != entry.size:
            raise RtfheError(ERR_INVALID, "add has %d flags for %d steps" % (add.size, entry.size))
        return entry, add

    def trlwe_auto_batch(self, key, x, entry, add=None):
        """Runs the program on every TRLWE row of x (u32[count][2][N]) and returns the rows: step k applies sigma_t and the key switch of entry
        entry[k] of `key` (t = key.t[entry[k]]) and replaces the row with the result, or adds the result into it where add[k] is 1 (add None:
        every step replaces).  1 .. 16 steps, shared by the batch.  A row that decrypts to mu under key_from then decrypts to sigma_t(mu) under
        key_to; t = 1 is a plain re-keying.  FP64 mirror backend, in the leveled decomposition in force now.  Arguments are checked here: a bad
        one raises RtfheError before anything runs."""
        x = _np(x, np.uint32).reshape(-1, 2, self.p.N)
        entry, add = self._program(entry, add)
        out = np.empty_like(x)
        self._ck(self.L.rtfhe_trlwe_auto_batch(self.h, key.h, _ptr(entry), _ptr(add), entry.size, _ptr(x), _ptr(out), x.shape[0]))
        return out

    def trlwe_auto_batch_dev(self, key, d_x, d_out, count, entry, add=None, stream=None):
        """... on device buffers (d_x, d_out: [count][2][N] words; d_out may be d_x itself, a partial overlap is refused), asynchronous on
        `stream`.  entry / add are host lists and are read before the call returns.  One launch, nothing allocated: it may be captured first
        thing on a fresh stream."""
        entry, add = self._program(entry, add)
        self._ck(self.L.rtfhe_trlwe_auto_batch_dev(self.h, key.h, _ptr(entry), _ptr(add), entry.size, self._dev(d_x), self._dev(d_out), count, _stream(stream)))

    # ---- lvl0 dense layers (include/rtfhe.h: rtfhe_dense_create, rtfhe_tlwe_dense_batch[_dev]) -------------------------------------------------------
    def dense(self, W):
        """Keeps an integer matrix int[O][I], every entry in [-128, 127], on the primary device in the matrix pipe's operand order; a Dense
        handle (.O, .I), closed by close() or a with block.  Needs no key."""
        return Dense(self, W)

    def tlwe_dense_batch(self, dense, x, bias=None, acc=None):
        """out[g][o] = (acc[g][o] if acc is given else 0) + bias[o] on word n + sum_i W[o][i] x[g][i] on all n + 1 words of the lvl0 rows,
        wrapping: u32[count][O][n+1], exact word for word.  x: u32[count][I][n+1]; bias: u32[O] torus words (linear.dense_bias) or None.
        Arguments are checked here: a bad one raises RtfheError before anything runs."""
        w = self.p.n + 1
        x = _np(x, np.uint32).reshape(-1, dense.I, w)
        count = x.shape[0]
        bias = None if bias is None else _np(bias, np.uint32).reshape(dense.O)
        out = np.array(_np(acc, np.uint32).reshape(count, dense.O, w)) if acc is not None else np.empty((count, dense.O, w), np.uint32)
        self._ck(self.L.rtfhe_tlwe_dense_batch(self.h, dense.h, _ptr(x), _ptr(bias), 1 if acc is not None else 0, _ptr(out), count))
        return out

    def tlwe_dense_batch_dev(self, dense, d_x, d_out, count, bias=None, accumulate=False, stream=None):
        """... on device buffers (d_x: [count][I][n+1] words, d_out: [count][O][n+1] words, not overlapping), asynchronous on `stream`; bias stays
        a HOST array u32[O] and is read before the call returns; accumulate adds into d_out.  Nothing allocated, one launch (with a bias: one per
        512 outputs): it may be captured first thing on a fresh stream."""
        bias = None if bias is None else _np(bias, np.uint32).reshape(dense.O)
        self._ck(self.L.rtfhe_tlwe_dense_batch_dev(self.h, dense.h, self._dev(d_x), _ptr(bias), 1 if accumulate else 0, self._dev(d_out), count,
                                                   _stream(stream)))

    # ---- stage level ------------------------------------------------------------------------
    def blind_rotate_batch(self, tlwe, steps=None):
        tlwe = _np(tlwe, np.uint32).reshape(-1, self.p.n + 1)
        acc = np.empty((tlwe.shape[0], 2, self.p.N), np.uint32)
        self._ck(self.L.rtfhe_blind_rotate_batch(self.h, _ptr(tlwe), self.p.n if steps is None else steps,
                                                 _ptr(acc), tlwe.shape[0]))
        return acc

    def external_product_batch(self, bk_index, trlwe):
        trlwe = _np(trlwe, np.uint32).reshape(-1, 2, self.p.N)
        idx = _np(bk_index, np.int32).reshape(-1)
        assert idx.size == trlwe.shape[0]
        out = np.empty_like(trlwe)
        self._ck(self.L.rtfhe_external_product_batch(self.h, _ptr(idx), _ptr(trlwe), _ptr(out), trlwe.shape[0]))
        return out

    def key_switch_batch(self, tlwe1):
        tlwe1 = _np(tlwe1, np.uint32).reshape(-1, self.p.N + 1)
        out = np.empty((tlwe1.shape[0], self.p.n + 1), np.uint32)
        self._ck(self.L.rtfhe_key_switch_batch(self.h, _ptr(tlwe1), _ptr(out), tlwe1.shape[0]))
        return out

    def ifft_i32_batch(self, src):
        src = _np(src, np.int32).reshape(-1, self.p.N)
        res = np.empty(src.shape, np.float64)
        self._ck(self.L.rtfhe_ifft_i32_batch(self.h, _ptr(src), _ptr(res), src.shape[0]))
        return res

    def ifft_f64_batch(self, src):
        """Spqlios_ifft: forward transform of double polynomials."""
        src = _np(src, np.float64).reshape(-1, self.p.N)
        res = np.empty(src.shape, np.float64)
        self._ck(self.L.rtfhe_ifft_f64_batch(self.h, _ptr(src), _ptr(res), src.shape[0]))
        return res

    def fft_f64_batch(self, src):
        """Spqlios_fft: inverse transform to doubles (scaled by 2/N, no truncation)."""
        src = _np(src, np.float64).reshape(-1, self.p.N)
        res = np.empty(src.shape, np.float64)
        self._ck(self.L.rtfhe_fft_f64_batch(self.h, _ptr(src), _ptr(res), src.shape[0]))
        return res

    def poly_mul_batch(self, a, b):
        """Spqlios_poly_mul: negacyclic product of torus polynomials through the FP64 transform."""
        a = _np(a, np.uint32).reshape(-1, self.p.N)
        b = _np(b, np.uint32).reshape(a.shape)
        res = np.empty_like(a)
        self._ck(self.L.rtfhe_poly_mul_batch(self.h, _ptr(a), _ptr(b), _ptr(res), a.shape[0]))
        return res

    def fft_u32_batch(self, src):
        src = _np(src, np.float64).reshape(-1, self.p.N)
        res = np.empty(src.shape, np.uint32)
        self._ck(self.L.rtfhe_fft_u32_batch(self.h, _ptr(src), _ptr(res), src.shape[0]))
        return res


class Lut(_Handle):
    """Test polynomials of a programmable bootstrap on an Engine's devices (rtfhe_lut), plain or encrypted (TRLWE rows, Engine.lut_encrypted).
    Closing it frees the device copies; a Lut whose Engine was closed first only frees its handle."""

    def __init__(self, engine, tv, encrypted=False, seeded=None):
        """seeded: (seed, first_row) -- tv then holds the b halves u32[n_lut][N] of an encrypted table (Engine.lut_encrypted_seeded)."""
        tv = _np(tv, np.uint32)
        tv = tv.reshape(-1, 2 * engine.p.N if encrypted and seeded is None else engine.p.N)
        self.engine, self._destroy = engine, engine.L.rtfhe_lut_destroy
        self.encrypted = bool(encrypted)
        self.n_lut = tv.shape[0]
        h = C.c_void_p()
        if seeded is not None:
            engine._ck(engine.L.rtfhe_lut_create_encrypted_seeded(engine.h, _ptr(seeded[0]), seeded[1], _ptr(tv), self.n_lut, C.byref(h)))
        else:
            create = engine.L.rtfhe_lut_create_encrypted if encrypted else engine.L.rtfhe_lut_create
            engine._ck(create(engine.h, _ptr(tv), self.n_lut, C.byref(h)))
        self.h = h

    def update_dev(self, d_trlwe, first=0, n=1, stream=None):
        """Rewrites rows [first, first + n) of an encrypted table in place from device memory u32[n][2][N] (rtfhe_lut_update_dev), e.g. the
        output of Engine.pack_batch_dev; a copy ordered on `stream`.  Refused for a plain table, a bad range and a multi-device Engine."""
        e = self.engine
        e._ck(e.L.rtfhe_lut_update_dev(self.h, e._dev(d_trlwe), int(first), int(n), _stream(stream)))

    def accumulate_dev(self, d_trlwe, first=0, n=1, count=1, stream=None):
        """Adds device TRLWEs u32[count][n][2][N] into rows [first, first + n) of an encrypted table in place (rtfhe_lut_accumulate_dev):
        row[first + r] += sum over g of d_trlwe[g][r], wrapping on every word, ordered on `stream` -- e.g. the leaves of
        Engine.demux_tree_batch_dev (n = 2^depth): an oblivious scatter-add.  Refused for a plain table, a bad range, count < 1 and a
        multi-device Engine."""
        e = self.engine
        e._ck(e.L.rtfhe_lut_accumulate_dev(self.h, e._dev(d_trlwe), int(first), int(n), int(count), _stream(stream)))

    def read_dev(self, d_out, first=0, n=1, stream=None):
        """Copies rows [first, first + n) of an encrypted table into device memory u32[n][2][N] (rtfhe_lut_read_dev), ordered on `stream`:
        update_dev the other way, under the same refusals."""
        e = self.engine
        e._ck(e.L.rtfhe_lut_read_dev(self.h, e._dev(d_out), int(first), int(n), _stream(stream)))


class Selectors(_Handle):
    """The TRGSW selectors of CMUX trees on an Engine's primary device (rtfhe_trgsw), kept as spectra.  Closing it frees the device copy; one
    whose Engine was closed first only frees its handle."""

    def __init__(self, engine, trgsw, seeded=None):
        """seeded: (seed, first_row) -- trgsw then holds the b halves u32[n_sel][2l][N] (Engine.selectors_seeded)."""
        p = engine.p
        trgsw = _np(trgsw, np.uint32).reshape(-1, (2 if seeded is None else 1) * 2 * p.l * p.N)
        self.engine, self._destroy = engine, engine.L.rtfhe_trgsw_destroy
        self.n_sel = trgsw.shape[0]
        h = C.c_void_p()
        if seeded is not None:
            engine._ck(engine.L.rtfhe_trgsw_create_seeded(engine.h, _ptr(seeded[0]), seeded[1], _ptr(trgsw), self.n_sel, C.byref(h)))
        else:
            engine._ck(engine.L.rtfhe_trgsw_create(engine.h, _ptr(trgsw), self.n_sel, C.byref(h)))
        self.h = h

    def update(self, words, first=0):
        """Rewrites selectors [first, first + n) with new TRGSW samples u32[n][2][2l][N] (rtfhe_trgsw_update; synchronous): the circuits
        recorded on this set (Engine.cmux_circuit) then run on the new ciphertexts."""
        p = self.engine.p
        words = _np(words, np.uint32).reshape(-1, 2 * 2 * p.l * p.N)
        self.engine._ck(self.engine.L.rtfhe_trgsw_update(self.h, _ptr(words), int(first), words.shape[0]))

    def update_seeded(self, seed, b, first=0, first_row=0):
        """update from the new samples' seeded form (rtfhe_trgsw_update_seeded): b u32[n][2l][N], sample i's rows masked by rows
        first_row + 2l i .. of the seed.  A (seed, row) pair masks one ciphertext only: new samples take a fresh seed or unused rows."""
        p = self.engine.p
        b = _np(b, np.uint32).reshape(-1, 2 * p.l * p.N)
        self.engine._ck(self.engine.L.rtfhe_trgsw_update_seeded(self.h, _ptr(_seed(seed)), int(first_row), _ptr(b), int(first), b.shape[0]))


class PackingKey(_Handle):
    """A packing key on an Engine's primary device (rtfhe_packing_key), kept as signed byte limbs in the matrix pipe's operand order.  Closing
    it frees the device copy; one whose Engine was closed first only frees its handle."""

    def __init__(self, engine, pk, seeded=None):
        """seeded: (seed, first_row) -- pk then holds the b halves u32[n][t][base-1][N] (Engine.packing_key_seeded)."""
        p = engine.p
        pk = _np(pk, np.uint32).reshape(-1)
        self.engine, self._destroy = engine, engine.L.rtfhe_packing_key_destroy
        h = C.c_void_p()
        if seeded is not None:
            assert pk.size == packing_key_words(p) // 2, "b must be u32[n][t][base-1][N]"
            engine._ck(engine.L.rtfhe_packing_key_create_seeded(engine.h, _ptr(seeded[0]), seeded[1], _ptr(pk), C.byref(h)))
        else:
            assert pk.size == packing_key_words(p), "pk must be u32[n][t][base-1][2][N]"
            engine._ck(engine.L.rtfhe_packing_key_create(engine.h, _ptr(pk), C.byref(h)))
        self.h = h


class MultibitKey(_Handle):
    """A multi-bit bootstrapping key on an Engine's primary device (rtfhe_mbk), kept as spectra.  Closing it frees the device copy; one whose
    Engine was closed first only frees its handle."""

    def __init__(self, engine, words, g):
        words = _np(words, np.uint32).reshape(-1)
        self.engine, self._destroy, self.g = engine, engine.L.rtfhe_mbk_destroy, int(g)
        need = engine.L.rtfhe_mbk_words(C.byref(engine.p), int(g))
        assert need == 0 or words.size == need, "words must be u32[n_trgsw][2][2l][N] of this g (rustfhe_amd.mbk_keygen)"
        h = C.c_void_p()
        engine._ck(engine.L.rtfhe_mbk_create(engine.h, _ptr(words), int(g), C.byref(h)))
        self.h = h


class TrlweSwitchKey(_Handle):
    """A TRLWE switching key on an Engine's primary device (rtfhe_trlwe_ksk), kept as spectra: the key of Engine.trlwe_auto_batch[_dev].
    Closing it frees the device copy; one whose Engine was closed first only frees its handle."""

    def __init__(self, engine, words, t):
        self.t = [int(v) for v in np.asarray(t).reshape(-1)]
        self.n = len(self.t)
        words = _np(words, np.uint32).reshape(-1)
        self.engine, self._destroy = engine, engine.L.rtfhe_trlwe_ksk_destroy
        assert words.size == self.n * engine.p.l * 2 * engine.p.N, "words must be u32[n_t][l][2][N] (rustfhe_amd.trlwe_ksk_keygen)"
        h = C.c_void_p()
        engine._ck(engine.L.rtfhe_trlwe_ksk_create(engine.h, _ptr(words), _ptr(_np(self.t, np.int32)), self.n, C.byref(h)))
        self.h = h


class PlainPolys(_Handle):
    """Integer polynomials on an Engine's primary device (rtfhe_plain), kept as spectra: the plain operand of Engine.trlwe_mul_plain_batch[_dev].
    Closing it frees the device copy; one whose Engine was closed first only frees its handle."""

    def __init__(self, engine, w):
        w = _np(w, np.int32).reshape(-1, engine.p.N)
        self.engine, self._destroy = engine, engine.L.rtfhe_plain_destroy
        self.n = w.shape[0]
        self.wmax = int(np.abs(w.astype(np.int64)).sum(axis=1).max()) if self.n else 0
        h = C.c_void_p()
        engine._ck(engine.L.rtfhe_plain_create(engine.h, _ptr(w), self.n, C.byref(h)))
        self.h = h


class Dense(_Handle):
    """An integer matrix on an Engine's primary device (rtfhe_dense), kept as signed bytes in the matrix pipe's operand order with one correction
    word per output: the small operand of Engine.tlwe_dense_batch[_dev].  Closing it frees the device copy; one whose Engine was closed first
    only frees its handle."""

    def __init__(self, engine, W):
        W = np.asarray(W)
        assert W.ndim == 2 and (W.size == 0 or np.issubdtype(W.dtype, np.integer)), "W must be an integer matrix [O][I]"
        assert W.size == 0 or np.abs(W.astype(np.int64)).max() < 1 << 31, "weights must fit int32 (the library then checks [-128, 127])"
        self.engine, self._destroy = engine, engine.L.rtfhe_dense_destroy
        self.O, self.I = int(W.shape[0]), int(W.shape[1])
        W = _np(W, np.int32)
        h = C.c_void_p()
        engine._ck(engine.L.rtfhe_dense_create(engine.h, _ptr(W), self.O, self.I, C.byref(h)))
        self.h = h


class FftPlan(_Handle):
    """rtfhe_fft_plan: the reference's two transforms (and Spqlios_poly_mul) at any power of two 16 <= N <= 2048 on the GPU
    (FFT_Processor_Spqlios(N), utils/src/spqlios/fft_processor_spqlios.cpp:7-14); numpy in / numpy out.  The gate path's N = 1024 /
    2048 have their own, fast kernels behind Engine; this serves every other size the reference's FFT FFI accepts."""

    def __init__(self, N, device=0):
        self.L = _ffi.load()
        self._destroy = self.L.rtfhe_fft_plan_destroy
        self.N = int(N)
        h = C.c_void_p()
        rc = self.L.rtfhe_fft_plan_create(self.N, device, C.byref(h))
        if rc != 0:
            raise RtfheError(rc, (self.L.rtfhe_last_error(None) or b"").decode())
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise RtfheError(rc, (self.L.rtfhe_last_error(None) or b"").decode())

    def _run(self, fn, src, in_dtype, out_dtype, src2=None):
        src = _np(src, in_dtype).reshape(-1, self.N)
        res = np.empty(src.shape, out_dtype)
        if src2 is None:
            self._ck(fn(self.h, _ptr(src), _ptr(res), src.shape[0]))
        else:
            src2 = _np(src2, in_dtype).reshape(src.shape)
            self._ck(fn(self.h, _ptr(src), _ptr(src2), _ptr(res), src.shape[0]))
        return res

    def ifft_i32(self, src):
        return self._run(self.L.rtfhe_fft_plan_ifft_i32, src, np.int32, np.float64)

    def ifft_f64(self, src):
        return self._run(self.L.rtfhe_fft_plan_ifft_f64, src, np.float64, np.float64)

    def fft_u32(self, src):
        return self._run(self.L.rtfhe_fft_plan_fft_u32, src, np.float64, np.uint32)

    def fft_f64(self, src):
        return self._run(self.L.rtfhe_fft_plan_fft_f64, src, np.float64, np.float64)

    def poly_mul(self, a, b):
        return self._run(self.L.rtfhe_fft_plan_poly_mul, a, np.uint32, np.uint32, b)

    def get_twiddles(self):
        ifft, fft = np.empty(2 * self.N, np.float64), np.empty(2 * self.N, np.float64)
        self._ck(self.L.rtfhe_fft_plan_get_twiddles(self.h, _ptr(ifft), _ptr(fft)))
        return ifft, fft

    def set_twiddles(self, ifft_table, fft_table):
        a, b = _np(ifft_table, np.float64).reshape(2 * self.N), _np(fft_table, np.float64).reshape(2 * self.N)
        self._ck(self.L.rtfhe_fft_plan_set_twiddles(self.h, _ptr(a), _ptr(b)))


def device_link(dev_a, dev_b):
    """What the runtime reports between two devices of the node (rtfhe_device_link): {"can_access", "link", "link_type", "hops"}."""
    L = _ffi.load()
    can, lt, hops = C.c_int32(), C.c_uint32(), C.c_uint32()
    rc = L.rtfhe_device_link(dev_a, dev_b, C.byref(can), C.byref(lt), C.byref(hops))
    if rc != 0:
        raise RtfheError(rc, (L.rtfhe_last_error(None) or b"").decode())
    return {"can_access": can.value, "link_type": lt.value, "link": _ffi.PeerInfo.LINK_NAMES.get(lt.value, "type %d" % lt.value), "hops": hops.value}


def pinned_empty(shape, dtype=np.uint32):
    """numpy array over pinned host memory (rtfhe_host_alloc): host-pointer calls DMA straight from / into it.  The memory
    is released when the array (and every view of it) is garbage-collected."""
    L = _ffi.load()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    ptr = L.rtfhe_host_alloc(n)
    if not ptr:
        raise RtfheError(_ffi.ERR_NOMEM, "rtfhe_host_alloc failed (needs a HIP device)")

    class _Owner:
        def __del__(self, _free=L.rtfhe_host_free, _p=ptr):
            _free(C.c_void_p(_p))
    buf = (C.c_char * n).from_address(ptr)
    arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
    buf._owner = _Owner()
    return arr


def demux_level_selector(depth, level):
    """The selector (address bit) that level `level` of a depth-`depth` demultiplexer (Engine.demux_tree_batch) splits on: depth - 1 - level,
    the most significant bit first.  Level k of cmux_tree_batch joins on selector k, so demux level t undoes tree level
    demux_level_selector(depth, t): the demultiplexer is the tree's inverse."""
    return int(depth) - 1 - int(level)


def packing_key_words(params):
    return params.n * params.ks_t * ((1 << params.ks_basebit) - 1) * 2 * params.N


def shard_range(count, d, n_dev):
    """[begin, end) of a count-gate host batch taken by entry d of an n_dev-device context (rtfhe_shard_range)."""
    L = _ffi.load()
    b, e = C.c_size_t(), C.c_size_t()
    rc = L.rtfhe_shard_range(count, d, n_dev, C.byref(b), C.byref(e))
    if rc != 0:
        raise RtfheError(rc, (L.rtfhe_last_error(None) or b"").decode())
    return b.value, e.value
