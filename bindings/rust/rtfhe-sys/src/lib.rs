//! Raw bindings; one declaration per entry point of `include/rtfhe.h` (same order).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rtfhe_params {
    pub n: i32,          // TLWE lvl0 dimension    hom_nand/src/tlwe.rs:175
    pub N: i32,          // TRLWE degree           hom_nand/src/trlwe.rs:76
    pub nbit: i32,       // log2(N)                hom_nand/src/tfhe.rs:16
    pub l: i32,          // gadget levels          hom_nand/src/trgsw.rs:115
    pub bgbit: i32,      // gadget base bits       hom_nand/src/trgsw.rs:112
    pub ks_t: i32,       // key-switch levels      hom_nand/src/tlwe.rs:178
    pub ks_basebit: i32, // key-switch base bits   hom_nand/src/tlwe.rs:179
}
/// What the runtime reported about entry d of a multi-device context against the primary (include/rtfhe.h: rtfhe_peer_info).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct rtfhe_peer_info {
    pub device: i32,
    pub same_device: i32,
    pub can_access_from_primary: i32,
    pub can_access_to_primary: i32,
    pub enabled_from_primary: i32,
    pub enabled_to_primary: i32,
    pub link_type: u32,
    pub hops: u32,
    pub scatter_ms: f32,
    pub compute_ms: f32,
    pub gather_ms: f32,
}
pub enum rtfhe_ctx {}
pub enum rtfhe_circuit {}
pub enum rtfhe_lut {}
pub enum rtfhe_trgsw {}
pub enum rtfhe_packing_key {}
pub enum rtfhe_mbk {}
pub enum rtfhe_plain {}
pub enum rtfhe_dense {}
pub enum rtfhe_trlwe_ksk {}
pub enum rtfhe_fft_plan {}

pub const RTFHE_NAND: c_int = 0;
pub const RTFHE_AND: c_int = 1;
pub const RTFHE_OR: c_int = 2;
pub const RTFHE_XOR: c_int = 3;
pub const RTFHE_NOT: c_int = 4;
pub const RTFHE_COPY: c_int = 5;
pub const RTFHE_ANDNY: c_int = 6;

pub const RTFHE_BACKEND_FFT64_MIRROR: c_int = 0;
pub const RTFHE_BACKEND_NTT_EXACT: c_int = 1;
pub const RTFHE_BACKEND_FFT_SPLIT_EXACT: c_int = 2;
pub const RTFHE_DECOMP_REFERENCE: c_int = 0;
pub const RTFHE_DECOMP_ROUNDED: c_int = 1;

pub const RTFHE_OK: c_int = 0;
pub const RTFHE_ERR_INVALID: c_int = -1;
pub const RTFHE_ERR_NO_DEVICE: c_int = -2;
pub const RTFHE_ERR_HIP: c_int = -3;
pub const RTFHE_ERR_STATE: c_int = -4;
pub const RTFHE_ERR_NOMEM: c_int = -5;

extern "C" {
    pub fn rtfhe_default_params(p: *mut rtfhe_params);
    pub fn rtfhe_ctx_create(p: *const rtfhe_params, device_id: c_int, out: *mut *mut rtfhe_ctx) -> c_int;
    pub fn rtfhe_ctx_create_multi(p: *const rtfhe_params, device_ids: *const c_int, n_dev: c_int, out: *mut *mut rtfhe_ctx) -> c_int;
    pub fn rtfhe_ctx_device_count(ctx: *const rtfhe_ctx) -> c_int;
    pub fn rtfhe_ctx_memory_bytes(ctx: *const rtfhe_ctx, d: c_int, bytes: *mut usize) -> c_int;
    pub fn rtfhe_ctx_peer_info(ctx: *mut rtfhe_ctx, d: c_int, out: *mut rtfhe_peer_info) -> c_int;
    pub fn rtfhe_device_link(dev_a: c_int, dev_b: c_int, can_access: *mut i32, link_type: *mut u32, hops: *mut u32) -> c_int;
    pub fn rtfhe_shard_range(count: usize, d: c_int, n_dev: c_int, begin: *mut usize, end: *mut usize) -> c_int;
    pub fn rtfhe_host_alloc(bytes: usize) -> *mut c_void;
    pub fn rtfhe_host_free(p: *mut c_void);
    pub fn rtfhe_ctx_destroy(ctx: *mut rtfhe_ctx);
    pub fn rtfhe_last_error(ctx: *const rtfhe_ctx) -> *const c_char;
    pub fn rtfhe_version() -> *const c_char;
    pub fn rtfhe_device_count() -> c_int;
    pub fn rtfhe_set_backend(ctx: *mut rtfhe_ctx, backend: c_int) -> c_int;
    pub fn rtfhe_get_backend(ctx: *const rtfhe_ctx) -> c_int;
    pub fn rtfhe_set_decomposition(ctx: *mut rtfhe_ctx, mode: c_int) -> c_int;
    pub fn rtfhe_get_decomposition(ctx: *const rtfhe_ctx) -> c_int;
    pub fn rtfhe_set_leveled_decomposition(ctx: *mut rtfhe_ctx, mode: c_int) -> c_int;
    pub fn rtfhe_get_leveled_decomposition(ctx: *const rtfhe_ctx) -> c_int;
    pub fn rtfhe_get_twiddles(ctx: *const rtfhe_ctx, ifft_table: *mut f64, fft_table: *mut f64) -> c_int;
    pub fn rtfhe_set_twiddles(ctx: *mut rtfhe_ctx, ifft_table: *const f64, fft_table: *const f64) -> c_int;
    pub fn rtfhe_ctx_params(ctx: *const rtfhe_ctx, p: *mut rtfhe_params) -> c_int;
    pub fn rtfhe_twiddles_load(ctx: *mut rtfhe_ctx, path: *const c_char, entries_changed: *mut i32) -> c_int;
    pub fn rtfhe_twiddles_write(ctx: *const rtfhe_ctx, path: *const c_char) -> c_int;
    pub fn rtfhe_twiddles_file_write(path: *const c_char, n: i32, ifft_table: *const f64, fft_table: *const f64) -> c_int;
    pub fn rtfhe_twiddles_file_read(path: *const c_char, n: i32, ifft_table: *mut f64, fft_table: *mut f64) -> c_int;

    pub fn rtfhe_load_bk_torus(ctx: *mut rtfhe_ctx, bk: *const u32) -> c_int;
    pub fn rtfhe_load_bk_fft(ctx: *mut rtfhe_ctx, bk_f: *const f64) -> c_int;
    pub fn rtfhe_export_bk_fft(ctx: *mut rtfhe_ctx, bk_f: *mut f64) -> c_int;
    pub fn rtfhe_load_ksk(ctx: *mut rtfhe_ctx, ksk: *const u32) -> c_int;
    /// `KeySwitchingKey(Vec<[[TLWERep<M>; IKS_T]; IKS_L]>)` flattened as it stands: `u32[N][8][4][n+1]` (tlwe.rs:243-245)
    pub fn rtfhe_load_ksk_ref(ctx: *mut rtfhe_ctx, ksk_ref: *const u32) -> c_int;

    pub fn rtfhe_gate_batch(ctx: *mut rtfhe_ctx, op: c_int, in0: *const u32, in1: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_mux_batch(ctx: *mut rtfhe_ctx, c: *const u32, in0: *const u32, in1: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_bootstrap_batch(ctx: *mut rtfhe_ctx, tlwe: *const u32, out: *mut u32, count: usize) -> c_int;

    pub fn rtfhe_gate_batch_dev(ctx: *mut rtfhe_ctx, op: c_int, d_in0: *const c_void, d_in1: *const c_void, d_out: *mut c_void,
                                count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_mux_batch_dev(ctx: *mut rtfhe_ctx, d_c: *const c_void, d_in0: *const c_void, d_in1: *const c_void, d_out: *mut c_void,
                               count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_bootstrap_batch_dev(ctx: *mut rtfhe_ctx, d_tlwe: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_circuit_wave_dev(ctx: *mut rtfhe_ctx, d_ops: *const c_void, d_idx0: *const c_void, d_idx1: *const c_void,
                                  d_idx_out: *const c_void, d_wires: *mut c_void, num_wires: usize, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_circuit_create(ctx: *mut rtfhe_ctx, d_ops: *const c_void, d_idx0: *const c_void, d_idx1: *const c_void, d_idx_out: *const c_void,
                                wave_offsets: *const i32, num_waves: i32, d_wires: *mut c_void, num_wires: usize, out: *mut *mut rtfhe_circuit) -> c_int;
    pub fn rtfhe_circuit_launch(c: *mut rtfhe_circuit, stream: *mut c_void) -> c_int;
    pub fn rtfhe_circuit_destroy(c: *mut rtfhe_circuit);
    // programmable bootstrapping: caller-supplied test polynomials [n_lut][N]; lut_idx null = table 0 for every gate
    pub fn rtfhe_lut_create(ctx: *mut rtfhe_ctx, tv: *const u32, n_lut: i32, out: *mut *mut rtfhe_lut) -> c_int;
    pub fn rtfhe_lut_destroy(lut: *mut rtfhe_lut);
    pub fn rtfhe_pbs_batch(ctx: *mut rtfhe_ctx, lut: *const rtfhe_lut, lut_idx: *const i32, tlwe: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_pbs_batch_dev(ctx: *mut rtfhe_ctx, lut: *const rtfhe_lut, d_lut_idx: *const c_void, d_tlwe: *const c_void, d_out: *mut c_void,
                               count: usize, stream: *mut c_void) -> c_int;
    // many-LUT PBS: n_out (1, 2, 4, 8) outputs per gate from one blind rotation, out [count][n_out][n+1]
    pub fn rtfhe_pbs_many_batch(ctx: *mut rtfhe_ctx, lut: *const rtfhe_lut, n_out: i32, lut_idx: *const i32, tlwe: *const u32, out: *mut u32,
                                count: usize) -> c_int;
    pub fn rtfhe_pbs_many_batch_dev(ctx: *mut rtfhe_ctx, lut: *const rtfhe_lut, n_out: i32, d_lut_idx: *const c_void, d_tlwe: *const c_void,
                                    d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // LUT circuits: waves of many-LUT bootstraps of weighted wire sums, recorded into one graph (replay / free with rtfhe_circuit_launch / _destroy)
    pub fn rtfhe_lut_circuit_create(ctx: *mut rtfhe_ctx, lut: *const rtfhe_lut, fan_in: i32, in_idx: *const i32, weights: *const i32, cst: *const u32,
                                    lut_idx: *const i32, wave_offsets: *const i32, wave_n_out: *const i32, num_waves: i32, out_idx: *const i32,
                                    d_wires: *mut c_void, num_wires: usize, out: *mut *mut rtfhe_circuit) -> c_int;
    // encrypted tables: rows TRLWE [n_lut][2][N] under key1, accepted by the PBS entries and rtfhe_lut_circuit_create (freed by rtfhe_lut_destroy)
    pub fn rtfhe_lut_create_encrypted(ctx: *mut rtfhe_ctx, trlwe: *const u32, n_lut: i32, out: *mut *mut rtfhe_lut) -> c_int;
    // CMUX-tree table lookup: selector sets (TRGSW samples [n_sel][2][2l][N] under key1), then one row out of 2^depth per lookup;
    // sel_idx [count][depth] (null: g * depth + k), row0 [count] (null: 0), coef [count] (null: 0); out [count][2][N] / extract form [count][n+1]
    pub fn rtfhe_trgsw_create(ctx: *mut rtfhe_ctx, trgsw: *const u32, n_sel: i32, out: *mut *mut rtfhe_trgsw) -> c_int;
    pub fn rtfhe_trgsw_destroy(sel: *mut rtfhe_trgsw);
    pub fn rtfhe_cmux_tree_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, sel_idx: *const i32, depth: i32, lut: *const rtfhe_lut, row0: *const i32,
                                 out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_cmux_tree_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_sel_idx: *const c_void, depth: i32, lut: *const rtfhe_lut,
                                     d_row0: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_cmux_tree_extract_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, sel_idx: *const i32, depth: i32, lut: *const rtfhe_lut,
                                         row0: *const i32, coef: *const i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_cmux_tree_extract_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_sel_idx: *const c_void, depth: i32, lut: *const rtfhe_lut,
                                             d_row0: *const c_void, d_coef: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // TRGSW blind rotation: depth steps acc <- cmux(S_k, X^rot[k] * acc, acc) on each TRLWE [2][N]; sel_idx [count][depth] (null: g * depth + k),
    // rot a HOST array [depth] in every form (null: 2N - 2^k, depth <= log2 N + 1); out [count][2][N] (d_out may be d_trlwe) / extract form [count][n+1]
    pub fn rtfhe_trgsw_rotate_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, sel_idx: *const i32, depth: i32, rot: *const i32, trlwe: *const u32,
                                    out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_rotate_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_sel_idx: *const c_void, depth: i32, rot: *const i32,
                                        d_trlwe: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_trgsw_rotate_extract_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, sel_idx: *const i32, depth: i32, rot: *const i32,
                                            trlwe: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_rotate_extract_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_sel_idx: *const c_void, depth: i32, rot: *const i32,
                                                d_trlwe: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // CMUX netlists: node i = cmux(S_var[i], X^rot[i] * hi[i], lo[i]) over TRLWEs; a reference r >= 0 is node r < i, r < 0 table row row0[g] + (-1 - r);
    // out_coef null: d_out [count][n_out][2][N], else [count][n_out][n+1]; recorded into one graph (replay / free with rtfhe_circuit_launch / _destroy)
    pub fn rtfhe_cmux_circuit_create(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, lut: *const rtfhe_lut, var: *const i32, hi: *const i32, lo: *const i32,
                                     rot: *const i32, n_nodes: i32, n_vars: i32, out_ref: *const i32, out_coef: *const i32, n_out: i32,
                                     d_sel_idx: *const c_void, d_row0: *const c_void, d_out: *mut c_void, count: usize, out: *mut *mut rtfhe_circuit) -> c_int;
    // rewrites selectors [first, first + n) of a live set (synchronous): the inputs of the circuits recorded on it
    pub fn rtfhe_trgsw_update(sel: *mut rtfhe_trgsw, trgsw: *const u32, first: i32, n: i32) -> c_int;
    // packing key switch: lvl0 samples [count][P][n+1] into TRLWE rows [count][2][N]; pk [n][t][base-1][2][N] under key1; pos HOST [P] (null: p * rep);
    // rtfhe_lut_update_dev rewrites rows of an encrypted table in place from device memory (stream-ordered)
    pub fn rtfhe_packing_keygen(p: *const rtfhe_params, key0: *const i32, key1: *const i32, pk: *mut u32) -> c_int;
    pub fn rtfhe_packing_keygen_deterministic(p: *const rtfhe_params, seed: u64, key0: *const i32, key1: *const i32, pk: *mut u32) -> c_int;
    pub fn rtfhe_packing_key_create(ctx: *mut rtfhe_ctx, pk: *const u32, out: *mut *mut rtfhe_packing_key) -> c_int;
    // multi-bit blind rotation (g = 2 or 3 key bits per step)
    pub fn rtfhe_mbk_words(p: *const rtfhe_params, g: i32) -> usize;
    pub fn rtfhe_mbk_keygen(p: *const rtfhe_params, g: i32, key0: *const i32, key1: *const i32, out: *mut u32) -> c_int;
    pub fn rtfhe_mbk_keygen_deterministic(p: *const rtfhe_params, seed: u64, g: i32, key0: *const i32, key1: *const i32, out: *mut u32) -> c_int;
    pub fn rtfhe_mb_roots(N: i32, out: *mut f64) -> c_int;
    pub fn rtfhe_mb_point_exponents(N: i32, out: *mut i32) -> c_int;
    pub fn rtfhe_mbk_create(ctx: *mut rtfhe_ctx, words: *const u32, g: i32, out: *mut *mut rtfhe_mbk) -> c_int;
    pub fn rtfhe_mbk_destroy(k: *mut rtfhe_mbk);
    pub fn rtfhe_pbs_mb_batch(ctx: *mut rtfhe_ctx, mbk: *const rtfhe_mbk, lut: *const rtfhe_lut, lut_idx: *const i32, tlwe: *const u32, out: *mut u32,
                              count: usize) -> c_int;
    pub fn rtfhe_pbs_mb_batch_dev(ctx: *mut rtfhe_ctx, mbk: *const rtfhe_mbk, lut: *const rtfhe_lut, d_lut_idx: *const c_void, d_tlwe: *const c_void,
                                  d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_packing_key_destroy(pk: *mut rtfhe_packing_key);
    pub fn rtfhe_pack_batch(ctx: *mut rtfhe_ctx, pk: *const rtfhe_packing_key, tlwe: *const u32, P: i32, pos: *const i32, rep: i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_pack_batch_dev(ctx: *mut rtfhe_ctx, pk: *const rtfhe_packing_key, d_tlwe: *const c_void, P: i32, pos: *const i32, rep: i32, d_out: *mut c_void,
                                count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_lut_update_dev(lut: *mut rtfhe_lut, d_trlwe: *const c_void, first: i32, n: i32, stream: *mut c_void) -> c_int;
    // CMUX demultiplexer tree (the CMUX tree run backwards): x [count][2][N] into out [count][2^depth][2][N], leaf `addr` a TRLWE of x's message and
    // every other leaf of 0; level t splits on selector depth - 1 - t.  rtfhe_lut_accumulate_dev adds [count][n][2][N] into rows
    // [first, first + n) of an encrypted table, wrapping (stream-ordered); rtfhe_lut_read_dev copies such rows out to device memory
    pub fn rtfhe_demux_tree_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, sel_idx: *const i32, depth: i32, x: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_demux_tree_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_sel_idx: *const c_void, depth: i32, d_x: *const c_void, d_out: *mut c_void,
                                      count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_lut_accumulate_dev(lut: *mut rtfhe_lut, d_trlwe: *const c_void, first: i32, n: i32, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_lut_read_dev(lut: *const rtfhe_lut, d_out: *mut c_void, first: i32, n: i32, stream: *mut c_void) -> c_int;
    // TRLWE sample extraction (the packing key switch's inverse): coefficients coef[0 .. P) (HOST, null: p * stride) of trlwe [count][2][N] as lvl0
    // ciphertexts out [count][P][n+1] (needs the key-switching key) or, the lvl1 forms, as lvl1 samples out [count][P][N+1] (no key at all)
    pub fn rtfhe_trlwe_extract_batch(ctx: *mut rtfhe_ctx, trlwe: *const u32, P: i32, coef: *const i32, stride: i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_extract_batch_dev(ctx: *mut rtfhe_ctx, d_trlwe: *const c_void, P: i32, coef: *const i32, stride: i32, d_out: *mut c_void, count: usize,
                                         stream: *mut c_void) -> c_int;
    pub fn rtfhe_trlwe_extract_lvl1_batch(ctx: *mut rtfhe_ctx, trlwe: *const u32, P: i32, coef: *const i32, stride: i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_extract_lvl1_batch_dev(ctx: *mut rtfhe_ctx, d_trlwe: *const c_void, P: i32, coef: *const i32, stride: i32, d_out: *mut c_void, count: usize,
                                              stream: *mut c_void) -> c_int;
    // exact TRLWE x plain-polynomial products: out[g] = (accumulate ? out[g] : 0) + sum_k w[w_idx[g][k]] * x[x_idx[g][k]] mod 2^32, K in 1 ..= 8,
    // K * wmax <= 192 N; w_idx / x_idx [count][K] (null: entry k / row g * K + k); needs no key, every backend
    pub fn rtfhe_plain_create(ctx: *mut rtfhe_ctx, w: *const i32, n_w: i32, out: *mut *mut rtfhe_plain) -> c_int;
    pub fn rtfhe_plain_destroy(w: *mut rtfhe_plain);
    pub fn rtfhe_trlwe_mul_plain_batch(ctx: *mut rtfhe_ctx, w: *const rtfhe_plain, w_idx: *const i32, x: *const u32, n_x: i32, x_idx: *const i32, K: i32,
                                       accumulate: i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_mul_plain_batch_dev(ctx: *mut rtfhe_ctx, w: *const rtfhe_plain, d_w_idx: *const c_void, d_x: *const c_void, n_x: i32,
                                           d_x_idx: *const c_void, K: i32, accumulate: i32, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // TRLWE x TRGSW multiply-accumulate: out[g] = (accumulate ? out[g] : 0) + sum_k S[s_idx[g][k]] (.) x[x_idx[g][k]], summed in the frequency domain,
    // K in 1 ..= 8; s_idx / x_idx [count][K] (null: entry g * K + k); FP64 mirror backend only, no key of the context
    pub fn rtfhe_trlwe_mul_trgsw_batch(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, s_idx: *const i32, x: *const u32, n_x: i32, x_idx: *const i32, K: i32,
                                       accumulate: c_int, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_mul_trgsw_batch_dev(ctx: *mut rtfhe_ctx, sel: *const rtfhe_trgsw, d_s_idx: *const c_void, d_x: *const c_void, n_x: i32,
                                           d_x_idx: *const c_void, K: i32, accumulate: c_int, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // TRLWE key switching: a program of 1 ..= 16 steps on every row, step k = sigma_t (X -> X^t, t = t[entry[k]]) followed by the key switch with
    // entry entry[k] of the switching key, replacing the row or (add[k] = 1) added into it; entry / add HOST arrays in both forms (add null: all
    // replace); words [n_t][l][2][N], t [n_t] distinct odd exponents in [1, 2N); d_out may be exactly d_x; FP64 mirror backend only, no key of the context
    pub fn rtfhe_trlwe_ksk_keygen(p: *const rtfhe_params, key_from: *const i32, key_to: *const i32, t: *const i32, n_t: i32, out: *mut u32) -> c_int;
    pub fn rtfhe_trlwe_ksk_keygen_deterministic(p: *const rtfhe_params, key_from: *const i32, key_to: *const i32, seed: u64, t: *const i32, n_t: i32,
                                                out: *mut u32) -> c_int;
    pub fn rtfhe_trlwe_automorphism(N: i32, t: i32, x: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_ksk_create(ctx: *mut rtfhe_ctx, words: *const u32, t: *const i32, n_t: i32, out: *mut *mut rtfhe_trlwe_ksk) -> c_int;
    pub fn rtfhe_trlwe_ksk_destroy(key: *mut rtfhe_trlwe_ksk);
    pub fn rtfhe_trlwe_auto_batch(ctx: *mut rtfhe_ctx, key: *const rtfhe_trlwe_ksk, entry: *const i32, add: *const i32, n_steps: i32, x: *const u32,
                                  out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_auto_batch_dev(ctx: *mut rtfhe_ctx, key: *const rtfhe_trlwe_ksk, entry: *const i32, add: *const i32, n_steps: i32,
                                      d_x: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    // lvl0 dense layers: out[g][o][c] = (accumulate ? out[g][o][c] : 0) + [c == n] bias[o] + sum_i W[o][i] x[g][i][c] mod 2^32, exact on every
    // backend; W [O][I] with every entry in -128 ..= 127; x [count][I][n+1], out [count][O][n+1]; bias a HOST array [O] or null in both forms
    pub fn rtfhe_dense_create(ctx: *mut rtfhe_ctx, W: *const i32, O: i32, I: i32, out: *mut *mut rtfhe_dense) -> c_int;
    pub fn rtfhe_dense_destroy(w: *mut rtfhe_dense);
    pub fn rtfhe_tlwe_dense_batch(ctx: *mut rtfhe_ctx, w: *const rtfhe_dense, x: *const u32, bias: *const u32, accumulate: i32, out: *mut u32,
                                  count: usize) -> c_int;
    pub fn rtfhe_tlwe_dense_batch_dev(ctx: *mut rtfhe_ctx, w: *const rtfhe_dense, d_x: *const c_void, bias: *const u32, accumulate: i32,
                                      d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_sync(ctx: *mut rtfhe_ctx, stream: *mut c_void) -> c_int;
    pub fn rtfhe_timer_begin(ctx: *mut rtfhe_ctx, stream: *mut c_void) -> c_int;
    pub fn rtfhe_timer_end(ctx: *mut rtfhe_ctx, stream: *mut c_void, ms: *mut f64, launches: *mut i64) -> c_int;
    pub fn rtfhe_timer_end_detail(ctx: *mut rtfhe_ctx, stream: *mut c_void, ms: *mut f64, key_switch_ms: *mut f64, launches: *mut i64) -> c_int;

    pub fn rtfhe_blind_rotate_batch(ctx: *mut rtfhe_ctx, tlwe: *const u32, steps: i32, acc: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_external_product_batch(ctx: *mut rtfhe_ctx, bk_index: *const i32, trlwe: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_key_switch_batch(ctx: *mut rtfhe_ctx, tlwe1: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_ifft_i32_batch(ctx: *mut rtfhe_ctx, src: *const i32, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_fft_u32_batch(ctx: *mut rtfhe_ctx, src: *const f64, res: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_ifft_f64_batch(ctx: *mut rtfhe_ctx, src: *const f64, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_fft_f64_batch(ctx: *mut rtfhe_ctx, src: *const f64, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_poly_mul_batch(ctx: *mut rtfhe_ctx, a: *const u32, b: *const u32, res: *mut u32, count: usize) -> c_int;

    // the reference's transforms at any power of two 16 <= N <= 2048 (FFT_Processor_Spqlios(N); Spqlios::new takes them all)
    pub fn rtfhe_fft_plan_create(n: i32, device_id: c_int, out: *mut *mut rtfhe_fft_plan) -> c_int;
    pub fn rtfhe_fft_plan_destroy(plan: *mut rtfhe_fft_plan);
    pub fn rtfhe_fft_plan_degree(plan: *const rtfhe_fft_plan) -> i32;
    pub fn rtfhe_fft_plan_get_twiddles(plan: *const rtfhe_fft_plan, ifft_table: *mut f64, fft_table: *mut f64) -> c_int;
    pub fn rtfhe_fft_plan_set_twiddles(plan: *mut rtfhe_fft_plan, ifft_table: *const f64, fft_table: *const f64) -> c_int;
    pub fn rtfhe_fft_plan_ifft_i32(plan: *mut rtfhe_fft_plan, src: *const i32, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_fft_plan_ifft_f64(plan: *mut rtfhe_fft_plan, src: *const f64, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_fft_plan_fft_u32(plan: *mut rtfhe_fft_plan, src: *const f64, res: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_fft_plan_fft_f64(plan: *mut rtfhe_fft_plan, src: *const f64, res: *mut f64, count: usize) -> c_int;
    pub fn rtfhe_fft_plan_poly_mul(plan: *mut rtfhe_fft_plan, a: *const u32, b: *const u32, res: *mut u32, count: usize) -> c_int;

    // production: randomness from the OS CSPRNG (like the reference's thread_rng)
    pub fn rtfhe_keygen(p: *const rtfhe_params, key0: *mut i32, key1: *mut i32, bk: *mut u32, ksk: *mut u32) -> c_int;
    pub fn rtfhe_keygen_with_keys(p: *const rtfhe_params, key0: *const i32, key1: *const i32, bk: *mut u32, ksk: *mut u32) -> c_int;
    pub fn rtfhe_tlwe_encrypt_bits(p: *const rtfhe_params, key0: *const i32, bits: *const u8, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_encrypt_torus(p: *const rtfhe_params, key0: *const i32, mu: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_encrypt_torus(p: *const rtfhe_params, key1: *const i32, mu: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_bits(p: *const rtfhe_params, key1: *const i32, bits: *const u8, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_polys(p: *const rtfhe_params, key1: *const i32, mu: *const i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_phase(p: *const rtfhe_params, key1: *const i32, ct: *const u32, phase: *mut u32, count: usize) -> c_int;
    // seeded ciphertexts: (seed [8], first_row, b [rows][N]) stands for the full layout [rows/group][2][group][N]; row R's mask is the ChaCha20
    // keystream of the public seed with R in the nonce.  The production encryptors write a fresh seed and the b halves; *_deterministic: TEST ONLY
    pub fn rtfhe_mask_expand(n: i32, seed: *const u32, first_row: u64, a: *mut u32, rows: usize) -> c_int;
    pub fn rtfhe_seeded_expand(p: *const rtfhe_params, seed: *const u32, first_row: u64, b: *const u32, group: i32, out: *mut u32, rows: usize) -> c_int;
    pub fn rtfhe_trlwe_encrypt_torus_seeded(p: *const rtfhe_params, key1: *const i32, mu: *const u32, seed: *mut u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_bits_seeded(p: *const rtfhe_params, key1: *const i32, bits: *const u8, seed: *mut u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_polys_seeded(p: *const rtfhe_params, key1: *const i32, mu: *const i32, seed: *mut u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_packing_keygen_seeded(p: *const rtfhe_params, key0: *const i32, key1: *const i32, seed: *mut u32, b: *mut u32) -> c_int;
    pub fn rtfhe_trlwe_encrypt_torus_seeded_deterministic(p: *const rtfhe_params, key1: *const i32, noise_seed: u64, seed: *const u32, first_row: u64,
                                                          mu: *const u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_bits_seeded_deterministic(p: *const rtfhe_params, key1: *const i32, noise_seed: u64, seed: *const u32, first_row: u64,
                                                         bits: *const u8, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_polys_seeded_deterministic(p: *const rtfhe_params, key1: *const i32, noise_seed: u64, seed: *const u32, first_row: u64,
                                                          mu: *const i32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_packing_keygen_seeded_deterministic(p: *const rtfhe_params, noise_seed: u64, key0: *const i32, key1: *const i32, seed: *const u32,
                                                     first_row: u64, b: *mut u32) -> c_int;
    // ... on the device: one launch expands d_b into d_out (stream-ordered, capturable); the upload calls' seeded forms ship b alone
    pub fn rtfhe_seeded_expand_dev(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, d_b: *const c_void, group: i32, d_out: *mut c_void, rows: usize,
                                   stream: *mut c_void) -> c_int;
    pub fn rtfhe_trgsw_create_seeded(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, b: *const u32, n_sel: i32, out: *mut *mut rtfhe_trgsw) -> c_int;
    pub fn rtfhe_trgsw_update_seeded(sel: *mut rtfhe_trgsw, seed: *const u32, first_row: u64, b: *const u32, first: i32, n: i32) -> c_int;
    pub fn rtfhe_lut_create_encrypted_seeded(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, b: *const u32, n_lut: i32, out: *mut *mut rtfhe_lut) -> c_int;
    pub fn rtfhe_load_bk_seeded(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, b: *const u32) -> c_int;
    pub fn rtfhe_packing_key_create_seeded(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, b: *const u32, out: *mut *mut rtfhe_packing_key) -> c_int;
    // seeded lvl0 ciphertexts and the seeded key-switching key: (seed [8], first_row, b [rows]) stands for u32[rows][n+1], a[0..n) then b; row R's
    // mask is the same keystream cut at n words.  *_deterministic: TEST ONLY
    pub fn rtfhe_tlwe_mask_expand(n: i32, seed: *const u32, first_row: u64, a: *mut u32, rows: usize) -> c_int;
    pub fn rtfhe_tlwe_seeded_expand(p: *const rtfhe_params, seed: *const u32, first_row: u64, b: *const u32, out: *mut u32, rows: usize) -> c_int;
    pub fn rtfhe_tlwe_encrypt_bits_seeded(p: *const rtfhe_params, key0: *const i32, bits: *const u8, seed: *mut u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_encrypt_torus_seeded(p: *const rtfhe_params, key0: *const i32, mu: *const u32, seed: *mut u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_ksk_keygen_seeded(p: *const rtfhe_params, key0: *const i32, key1: *const i32, seed: *mut u32, b: *mut u32) -> c_int;
    pub fn rtfhe_tlwe_encrypt_bits_seeded_deterministic(p: *const rtfhe_params, key0: *const i32, noise_seed: u64, seed: *const u32, first_row: u64,
                                                        bits: *const u8, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_encrypt_torus_seeded_deterministic(p: *const rtfhe_params, key0: *const i32, noise_seed: u64, seed: *const u32, first_row: u64,
                                                         mu: *const u32, b: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_ksk_keygen_seeded_deterministic(p: *const rtfhe_params, noise_seed: u64, key0: *const i32, key1: *const i32, seed: *const u32,
                                                 first_row: u64, b: *mut u32) -> c_int;
    pub fn rtfhe_tlwe_seeded_expand_dev(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, d_b: *const c_void, d_out: *mut c_void, rows: usize,
                                        stream: *mut c_void) -> c_int;
    pub fn rtfhe_load_ksk_seeded(ctx: *mut rtfhe_ctx, seed: *const u32, first_row: u64, b: *const u32) -> c_int;
    // compressed results: k-bit, bit-packed rows off the GPU; the CPU twins and inverses need no context
    pub fn rtfhe_tlwe_compress_batch_dev(ctx: *mut rtfhe_ctx, k: i32, d_tlwe: *const c_void, d_out: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_trlwe_compress_batch_dev(ctx: *mut rtfhe_ctx, k: i32, d_trlwe: *const c_void, P: i32, coef: *const i32, stride: i32, d_out: *mut c_void,
                                          count: usize, stream: *mut c_void) -> c_int;
    // ... and back: packed rows that came up from the host, expanded on the device in the computation's stream
    pub fn rtfhe_tlwe_expand_batch_dev(ctx: *mut rtfhe_ctx, k: i32, d_words: *const c_void, d_tlwe: *mut c_void, count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_trlwe_expand_batch_dev(ctx: *mut rtfhe_ctx, k: i32, d_words: *const c_void, P: i32, coef: *const i32, stride: i32, d_trlwe: *mut c_void,
                                        count: usize, stream: *mut c_void) -> c_int;
    pub fn rtfhe_compressed_words(L: usize, k: i32) -> usize;
    pub fn rtfhe_tlwe_compress(n: i32, k: i32, input: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_expand(n: i32, k: i32, input: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_compress(N: i32, k: i32, P: i32, coef: *const i32, stride: i32, input: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_expand(N: i32, k: i32, P: i32, coef: *const i32, stride: i32, input: *const u32, out: *mut u32, count: usize) -> c_int;
    // TEST ONLY (seeded xoshiro256**, not secure)
    pub fn rtfhe_ksk_expand_ref(p: *const rtfhe_params, key0: *const i32, key1: *const i32, ksk: *const u32, ksk_ref: *mut u32) -> c_int;
    pub fn rtfhe_ksk_expand_ref_deterministic(p: *const rtfhe_params, seed: u64, key0: *const i32, key1: *const i32, ksk: *const u32, ksk_ref: *mut u32) -> c_int;
    pub fn rtfhe_keygen_deterministic(p: *const rtfhe_params, seed: u64, key0: *mut i32, key1: *mut i32, bk: *mut u32, ksk: *mut u32) -> c_int;
    pub fn rtfhe_keygen_with_keys_deterministic(p: *const rtfhe_params, seed: u64, key0: *const i32, key1: *const i32, bk: *mut u32, ksk: *mut u32) -> c_int;
    pub fn rtfhe_tlwe_encrypt_bits_deterministic(p: *const rtfhe_params, key0: *const i32, seed: u64, bits: *const u8, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_encrypt_torus_deterministic(p: *const rtfhe_params, key0: *const i32, seed: u64, mu: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trlwe_encrypt_torus_deterministic(p: *const rtfhe_params, key1: *const i32, seed: u64, mu: *const u32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_bits_deterministic(p: *const rtfhe_params, key1: *const i32, seed: u64, bits: *const u8, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_trgsw_encrypt_polys_deterministic(p: *const rtfhe_params, key1: *const i32, seed: u64, mu: *const i32, out: *mut u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_decrypt_bits(p: *const rtfhe_params, key0: *const i32, input: *const u32, bits: *mut u8, count: usize) -> c_int;
    pub fn rtfhe_keys_write(path: *const c_char, p: *const rtfhe_params, key0: *const i32, key1: *const i32, bk: *const u32, ksk: *const u32) -> c_int;
    pub fn rtfhe_keys_read_header(path: *const c_char, p: *mut rtfhe_params, flags: *mut u32) -> c_int;
    pub fn rtfhe_keys_read(path: *const c_char, key0: *mut i32, key1: *mut i32, bk: *mut u32, ksk: *mut u32) -> c_int;
    pub fn rtfhe_tlwe_write(path: *const c_char, n: i32, cts: *const u32, count: usize) -> c_int;
    pub fn rtfhe_tlwe_read(path: *const c_char, n: *mut i32, count: *mut u64, cts: *mut u32, capacity: usize) -> c_int;
    pub fn rtfhe_compressed_write(path: *const c_char, kind: i32, dim: i32, k: i32, P: i32, coef: *const i32, words: *const u32, count: usize) -> c_int;
    pub fn rtfhe_compressed_read_header(path: *const c_char, kind: *mut i32, dim: *mut i32, k: *mut i32, P: *mut i32, count: *mut u64) -> c_int;
    pub fn rtfhe_compressed_read(path: *const c_char, coef: *mut i32, words: *mut u32, capacity: usize) -> c_int;
    pub fn rtfhe_tlwe_phase(p: *const rtfhe_params, key0: *const i32, input: *const u32, phase: *mut u32, count: usize) -> c_int;
}
