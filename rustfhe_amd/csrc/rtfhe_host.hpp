// rtfhe_host.hpp -- host-side internals shared by the translation units behind the C ABI (include/rtfhe.h).  Beside the declarations it holds
// the host rules that every family follows, each in one place: handles_ready / detach / orphan_all (the lifetime rule),
// NewHandle / handle_publish / handle_destroy (the handle owner), host_form (the host-buffer form), stream_scratch, launch_kernel and
// launch_leveled, circuit_record.  The argument checks that need no context are not here: rtfhe_plan_kit.hpp (header only, no HIP) and the
// host-only plan units built on it.  The units:
//   rtfhe_context.hip        contexts, keys (load / layouts on demand / footprint), twiddle-table calls, copies, error plumbing, the handle and
//                            device-pointer checks of the entry points
//   rtfhe_twiddles.hip       host twiddle tables (the reference's builders restated) and the per-kernel device tables
//   rtfhe_dispatch_fft.hip   the FP64 mirror backend's bootstrap kernels: which kernel shape a batch runs on
//   rtfhe_dispatch_ntt.hip   the exact-integer NTT backend: host tables, key transform, kernel shapes
//   rtfhe_dispatch_xfft.hip  the split-FFT exact backend (exact products through an FMA-contracted FP64 FFT, N = 1024)
//   rtfhe_stages.hip         stage-level kernels and entry points (transforms, external product, key switch, key permutes), FFT plans at any N
//   rtfhe_batch.hip          batches of gates: the backend switch, split path, host-pointer and device-pointer batches, MUX, PBS entry points, timers
//   rtfhe_lut.hip            PBS tables (rtfhe_lut): creation on every entry of the context, release, and the three row calls of an encrypted
//                            table (update, accumulate -- k_trlwe_accumulate --, read)
//   rtfhe_circuit.hip        levelised netlists: one wave per call, or all waves recorded into a HIP graph
//   rtfhe_multi.hip          one context over several GPUs: key replication, sharding of host batches and of device-resident batches
//   rtfhe_cmux_tree.hip      CMUX-tree table lookup: selector sets (caller-supplied TRGSW samples), one launch per tree level; TRGSW blind rotation
//                            and the CMUX demultiplexer tree
//   rtfhe_cmux_net.hip       CMUX netlists: decision diagrams over a selector set, levelised (rtfhe_cmux_net_plan.cpp, host only) and recorded into a HIP graph
//   rtfhe_pack.hip           packing key switch: packing keys (signed byte limbs in operand order), lvl0 samples into TRLWE rows (its argument
//                            checks: rtfhe_pack_plan in rtfhe_extract_plan.cpp, host only)
//   rtfhe_extract.hip        TRLWE sample extraction: chosen coefficients of existing TRLWEs as lvl1 samples or, through the extract tail, lvl0 ciphertexts
//                            (its argument checks: rtfhe_extract_plan.cpp, host only)
//   rtfhe_trgsw_mac.hip      TRLWE x TRGSW multiply-accumulate over the selector sets of rtfhe_cmux_tree.hip (its argument checks:
//                            rtfhe_trgsw_mac_plan.cpp, host only, the sum-of-products body it shares with rtfhe_plain_plan.cpp)
//   rtfhe_plain.hip          exact TRLWE x plain-polynomial products: plain sets (integer polynomials as spectra), sums of up to eight products per sample
//                            on the split-FFT exact backend's arithmetic, on every backend (its argument checks: rtfhe_plain_plan.cpp, host only)
//   rtfhe_dense.hip          lvl0 dense layers: an integer matrix (signed bytes in i8-MFMA operand order) times a batch of TLWE rows, exact, on every
//                            backend (its argument checks, correction words and launch rule: rtfhe_dense_plan.cpp, host only)
//   rtfhe_seeded.hip         seeded ciphertexts: masks expanded on the device from a public seed (k_seeded_expand for TRLWE rows, k_tlwe_seeded_expand
//                            for lvl0 rows), the staging step of the *_seeded upload calls, which live beside their unseeded twins (its argument
//                            checks and the CPU forms: rtfhe_seeded.cpp, host only; the encryptor core it shares with rtfhe_keygen.cpp:
//                            rtfhe_encrypt.hpp)
//   rtfhe_compress.hip       compressed results: result rows rounded to k bits per word and bit-packed on the device (k_compress_rows), lvl0 rows and
//                            TRLWE rows with a list of kept coefficients, and packed rows expanded on the device again (k_expand_rows) (its argument
//                            checks, the inverse map of the list and the key holder's CPU forms: rtfhe_compress_plan.cpp, host only)
//   rtfhe_pbs_mb.hip         multi-bit blind rotation: multi-bit keys (spectra of 2^g - 1 TRGSW samples per group of g key bits, the roots table and
//                            the point map beside them) and the programmable bootstrap over them, ceil(n / g) steps (its sizes, tables and argument
//                            checks: rtfhe_mb_plan.cpp, host only)
//   rtfhe_trlwe_auto.hip     TRLWE key switching: switching keys (rows of -sigma_t(key_from) times the gadget as spectra) and the automorphism /
//                            re-keying programs over them, one launch of k_trlwe_auto (its argument checks: rtfhe_trlwe_auto_plan.cpp, host only)
// Every kernel is instantiated in exactly one of them.  No CPU fallback anywhere: an entry point runs HIP kernels or fails.
#pragma once

#include "../../include/rtfhe.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "rtfhe_kernels.hpp"
#include "rtfhe_seeded_plan.h"

// ------------------------------------------------------------------------------------------------
// twiddle tables (host).  Values follow the reference's table builders so that a context created in
// the same process / against the same libm as the reference holds the same bits:
//   accurate_cos / accurate_sin   utils/src/spqlios/spqlios-fft-impl.cpp:99-113
//   new_ifft_table                utils/src/spqlios/spqlios-fft-impl.cpp:400-437
//   new_fft_table                 utils/src/spqlios/spqlios-fft-impl.cpp:158-193
// ------------------------------------------------------------------------------------------------
struct HostTw {
    int N = 0;
    // per-stage natural order; forward stages concatenated halfnn = P/2 .. 4, inverse halfnn = 4 .. P/2
    std::vector<double> twist_c, twist_s, untw_c, untw_s, fwd_c, fwd_s, inv_c, inv_s;
    int fwd_off(int halfnn) const { return N / 2 - 2 * halfnn; }
    int inv_off(int halfnn) const { return halfnn - 4; }

    void build(int N_);
    // the reference's memory layout (2N doubles per direction: per stage, blocks | c0 c1 c2 c3 | s0 s1 s2 s3 |)
    void export_ref(double* ifft_table, double* fft_table) const;
    void import_ref(const double* ifft_table, const double* fft_table);
    // device tables, one per kernel family (rtfhe_twiddles.hip)
    std::vector<rtfhe::cplx> device_table(int logn) const;     // Geo<LOGN>: per direction [twist R*64][pass1 (R-1)*64][pass2 (R-1)*NLOW][pass3 NLOW-4]
    std::vector<rtfhe::cplx> eo_table() const;                 // EoTw: k_bootstrap_eo / _eo4 (N = 2048)
    std::vector<rtfhe::cplx> q4_table() const;                 // Q4Tw: the parity sub-networks of k_bootstrap_wg / _pair4 (N = 1024)
};

// Device scratch between the launches of one call, ONE buffer (or pair) per stream the call was ever launched on: launches of one stream are
// ordered, launches on different streams of one context may overlap and must not share it.  cap: what each buffer holds, in its owner's units.
// captured: a call inside a caller's stream capture baked d into a graph -- never freed while the context lives (a larger eager call retires it
// to rtfhe_ctx::mux_retired and gets a new one).  rtfhe_host::stream_scratch is the one place that applies these rules.
struct StreamScratch { uint32_t* d[2] = {nullptr, nullptr}; size_t cap = 0; bool captured = false; };
typedef std::unordered_map<hipStream_t, StreamScratch> ScratchMap;

struct rtfhe_circuit;
struct rtfhe_lut;
struct rtfhe_trgsw;
struct rtfhe_packing_key;
struct rtfhe_plain;
struct rtfhe_dense;
struct rtfhe_mbk;
struct rtfhe_trlwe_ksk;
struct rtfhe_ctx {
    rtfhe_params p{};
    int device = 0;
    int logn = 10;
    HostTw tw;
    rtfhe::cplx* d_tw = nullptr;
    rtfhe::cplx* d_bk = nullptr;             // key spectra, canonical device layout [n][2l][2][R][64] (every N)
    rtfhe::cplx* d_etw = nullptr;            // N = 2048: tables of k_bootstrap_eo
    // second layouts of the key spectra, built from d_bk by the first batch whose dispatch reads them (ensure_bk_layout) and dropped when the key changes
    rtfhe::cplx* d_ebk = nullptr;            // N = 2048: the even / odd layout of k_bootstrap_eo / _eo4
    rtfhe::cplx* d_p4bk = nullptr;           // N = 1024: the layout of k_bootstrap_pair4
    bool ebk_valid = false, p4bk_valid = false;
    int pair4 = 3;                    // N = 1024, four waves per gate (k_bootstrap_pair4) for batches and tails of more than wg_max gates and up to
                                      // `pair4` gates per CU (RTFHE_PAIR4: 0 = never, 2, 3 = default)
    int rr = 6;                       // N = 1024: a last whole round and the remainder behind it, up to `rr` gates per CU in all, as ONE time-sliced launch
                                      // (k_bootstrap_pair_rr; RTFHE_PAIR_RR: 0 = never, 5, 6 = default)
    int xrr = 0;                      // ... the same on the split-FFT exact backend (k_bootstrap_xpair_rr): min(rr, what fits), set when that backend's kernels are primed
    int eo4 = 1;                      // N = 2048, up to two gates per CU: 1 = four waves per gate (k_bootstrap_eo4), 0 = two (RTFHE_N2048_EO4)
    int eo_round = 4;                 // N = 2048: gates per CU in a whole round of k_bootstrap_eo: 4, or 3 where four gates' LDS passes 160 KiB (n >= 704), set when the kernels are primed
    int backend = RTFHE_BACKEND_FFT64_MIRROR;
    int decomp = RTFHE_DECOMP_REFERENCE;   // the gadget decomposition of the PBS family (rtfhe_set_decomposition); gates never read it
    int leveled_decomp = RTFHE_DECOMP_REFERENCE;   // ... of the leveled entry points (rtfhe_set_leveled_decomposition): tree, rotation, CMUX netlists
                                           // at creation, the mirror backend's external product; independent of `decomp`
    uint32_t* d_bk_torus = nullptr;   // kept when the key came in torus form: source for the NTT-domain key
    double* d_ntt_bk = nullptr;
    double* d_ntt_tw = nullptr;
    bool ntt_ready = false;
    rtfhe::cplx* d_xbk = nullptr;     // split-FFT exact backend: the key as two 16-bit halves, each as spectra (2 x the canonical size)
    rtfhe::cplx* d_xtw = nullptr;
    bool xfft_ready = false;
    uint32_t* d_ksk = nullptr;
    int ksw = 0;
    uint4* d_ksmat = nullptr;         // the key-switching key as signed byte limbs in i8-MFMA operand order (rtfhe_kernels_ksmm.hpp)
    size_t ksk_bytes = 0, ksmat_bytes = 0;
    // lvl1 samples between the two launches of the split path (d[0]; cap in samples), plus a circuit's own during its capture
    ScratchMap tlwe1;
    StreamScratch* tlwe1_capture = nullptr;   // set by circuit_record around a circuit's capture: the circuit's buffer
    bool foreign_capture = false;     // set by launch_bootstrap for the duration of a call made inside a stream capture that is NOT
                                      // rtfhe_circuit_create's: such a batch stays on the fused kernel (see split_ok)
    int ks_mm_min = 1;                // batches of at least this many gates take the split path (0 = never: fused kernel); RTFHE_KS_MM_MIN
    bool has_bk = false, has_ksk = false;
    void* d_a = nullptr; void* d_b = nullptr; void* d_c = nullptr;   // device staging for host-pointer calls (and a peer's shard of a device-resident batch)
    size_t cap_a = 0, cap_b = 0, cap_c = 0;
    void* h_pin[3] = {nullptr, nullptr, nullptr};                     // pinned host staging (pageable caller buffers go through it)
    size_t cap_pin[3] = {0, 0, 0};
    bool stage_pinned = false;                                        // RTFHE_STAGING=1: stage pageable caller buffers through h_pin (measured slower
                                                                      // than the runtime's own pageable path: +3.4 % vs +1.5 % at 1024 gates)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_shard = nullptr;    // multi-device, device-resident batches: "inputs ready" on the primary / "shard gathered" on a peer
    hipEvent_t ev_sh[3] = {nullptr, nullptr, nullptr};   // a peer's share of such a batch: before its pull, after it, after its bootstrap (ev_shard: after its push)
    bool shard_timed = false;         // ev_sh / ev_shard bracket a batch
    // what rtfhe_ctx_create_multi found out about this entry against the primary (rtfhe_ctx_peer_info)
    struct PeerLink { int same_device = 0, can_from = 0, can_to = 0, en_from = 0, en_to = 0; uint32_t link_type = 0xffffffffu, hops = 0; } link;
    int64_t launches = 0;
    // between rtfhe_timer_begin and _end every batch key switch of the split path is bracketed by a pair of events of its own, so
    // that the timer can report the blind-rotation kernel's and the key-switch kernel's device time separately
    bool timing = false;
    std::vector<hipEvent_t> ks_events;     // pool, pairs (before memset + k_key_switch_mm, after)
    size_t ks_events_used = 0;
    int32_t* d_fault = nullptr;            // set by a kernel that skipped a netlist gate (bad wire index / opcode)
    unsigned long long* d_dbg = nullptr;   // RTFHE_WG_STAMPS builds: 128 words of phase timings
    std::unordered_map<const void*, size_t> lds_allowed;   // kernel -> dynamic LDS bytes already granted on this device
    // multi-device context (rtfhe_ctx_create_multi): one full single-device context per further device; `this` is device 0 of
    // the set.  Keys are loaded once on this context and copied device-to-device; batches are sharded (rtfhe_multi.hip).
    std::vector<rtfhe_ctx*> peers;
    std::vector<rtfhe_circuit*> circuits;   // live HIP-graph circuits of this context: orphaned (not freed) by rtfhe_ctx_destroy
    std::vector<rtfhe_lut*> luts;           // live PBS tables of this context (primary only): their device copies go with it, the handles stay
    ScratchMap mux;                        // device intermediates (i1, i0) of a MUX batch: a pair, cap in bytes of EACH
    std::vector<void*> mux_retired;        // scratch of any kind below or above that a caller's graph holds and a larger eager call replaced: freed with the context
    // the two ping-pong buffers of a CMUX tree's or demultiplexer's levels (rtfhe_cmux_tree.hip): a pair, cap in words of EACH; not counted by
    // rtfhe_ctx_memory_bytes
    ScratchMap tree;
    std::vector<rtfhe_trgsw*> trgsws;      // live selector sets of this context: their spectra go with it, the handles stay
    // the key-switched samples S[count * P][2N] between the two launches of a packing key switch (rtfhe_pack.hip): d[0], cap in samples; not
    // counted by rtfhe_ctx_memory_bytes
    ScratchMap pack;
    std::vector<rtfhe_packing_key*> pack_keys;      // live packing keys of this context: their matrices go with it, the handles stay
    std::vector<rtfhe_plain*> plains;      // live plain sets of this context: their spectra go with it, the handles stay
    std::vector<rtfhe_dense*> denses;      // live dense layers of this context: their matrices go with it, the handles stay
    std::vector<rtfhe_mbk*> mbks;          // live multi-bit keys of this context: their spectra go with it, the handles stay; counted by rtfhe_ctx_memory_bytes
    std::vector<rtfhe_trlwe_ksk*> trlwe_ksks;      // live TRLWE switching keys of this context: their spectra go with it, the handles stay
    int num_cus = 256;
    int force_waves = 0;   // RTFHE_FORCE_WAVES=1|2|4|8: one kernel shape for every batch (the parity tests' second opinions)
    int wg_max = 512;      // RTFHE_WG_MAX_GATES: largest batch routed to the workgroup-per-gate kernel
    std::string err;
};

// The eight handle types below hang on their context by one rule.  `ctx` points back at it and the context lists the live handles of each type.
// A handle destroyed first detaches itself from that list (rtfhe_host::detach) and releases its device memory; a context destroyed first releases
// the device memory of every listed handle and clears their `ctx` (rtfhe_host::orphan_all): the handle then only remains to be freed, and every
// call made with it is refused by rtfhe_host::handles_ready.

// a whole levelised netlist recorded into a HIP graph (rtfhe_circuit_create)
struct rtfhe_circuit {
    rtfhe_ctx* ctx = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int device = 0;            // kept here: the context may be destroyed before the circuit
    uint32_t* d_samples = nullptr;   // the circuit's own lvl1 sample buffer (split path): replays on any stream never share one with other work
    std::vector<void*> d_owned;      // a LUT circuit's other device buffers (rtfhe_lut_circuit_create): description, gathered inputs, key-switched
                                     // outputs, its copy of the table rows
    int32_t waves = 0;
    int64_t launches = 0;      // kernel launches one replay stands for
    int backend = RTFHE_BACKEND_FFT64_MIRROR;   // the backend it was recorded on
    bool stale = false;        // recorded on an exact backend whose key form could not follow a key change (rebuild_derived_keys)
    const rtfhe_trgsw* sel = nullptr;   // a CMUX netlist (rtfhe_cmux_circuit_create): the selector set whose spectra its graph reads in place
    bool sel_gone = false;     // ... and that set is gone (rtfhe_trgsw_destroy): the graph holds freed addresses
};

// the test polynomials of a programmable bootstrap (rtfhe_lut_create), one copy on every entry of the context
struct rtfhe_lut {
    rtfhe_ctx* ctx = nullptr;           // the primary
    std::vector<uint32_t*> d_tv;        // [entry] u32[n_lut][N] on entry d of the context (0: the primary, d: peers[d - 1]); encrypted: [n_lut][2][N]
    int32_t n_lut = 0;
    bool encrypted = false;             // rtfhe_lut_create_encrypted: TRLWE rows (b, a), run by the k_pbs_enc_* kernels on the many-LUT path
};

// a selector set of a CMUX tree (rtfhe_trgsw_create): caller-supplied TRGSW samples as spectra on the primary device
struct rtfhe_trgsw {
    rtfhe_ctx* ctx = nullptr;
    rtfhe::cplx* d_spec = nullptr;      // [n_sel][2l][2][R][64], the layout of one bootstrapping-key entry each
    int32_t n_sel = 0;
};

// a packing key (rtfhe_packing_key_create): the key rows as signed byte limbs in i8-MFMA operand order on the primary device
struct rtfhe_packing_key {
    rtfhe_ctx* ctx = nullptr;
    uint4* d_kmat = nullptr;            // [2N / 16 column groups][n16 / 2 K-steps][4 limbs][64 lanes] x 16 B (rtfhe_kernels_pack.hpp)
    int32_t n16 = 0, colgroups = 0;
};

// a plain set (rtfhe_plain_create): integer polynomials as spectra on the primary device, the small operand of rtfhe_trlwe_mul_plain_batch
struct rtfhe_plain {
    rtfhe_ctx* ctx = nullptr;
    rtfhe::cplx* d_spec = nullptr;      // N = 1024: [n_w][512]; N = 2048: [n_w][2 halves][512] (rtfhe_kernels_plain.hpp)
    int32_t n_w = 0;
    int64_t wmax = 0;                   // max over the set of a polynomial's l1 norm: a call is accepted iff K * wmax <= 192 N
};

// a dense layer (rtfhe_dense_create): the matrix as signed bytes in i8-MFMA operand order on the primary device, the small operand of
// rtfhe_tlwe_dense_batch
struct rtfhe_dense {
    rtfhe_ctx* ctx = nullptr;
    uint4* d_wmat = nullptr;            // [planes][otiles][ksteps][64 lanes] x 16 B (rtfhe_kernels_dense.hpp)
    uint32_t* d_corr = nullptr;         // [O]: 128 * 0x01010101 * sum_i W[o][i], what the signed byte limbs of the ciphertext drop
    int32_t O = 0, I = 0, ksteps = 0, otiles = 0;
    int32_t planes = 1;                 // byte planes of the weights (W = sum_p 256^p W_p): one today
};

// a multi-bit bootstrapping key (rtfhe_mbk_create): the TRGSW samples of every group as spectra on the primary device, with the two tables the
// key combination reads
struct rtfhe_mbk {
    rtfhe_ctx* ctx = nullptr;
    rtfhe::cplx* d_spec = nullptr;      // [n_trgsw][2l][2][R][64], the layout of one bootstrapping-key entry each; groups in order, subsets ascending
    rtfhe::cplx* d_roots = nullptr;     // W[2N] (rtfhe_mb_roots)
    int32_t* d_qmap = nullptr;          // [N/2] (rtfhe_mb_point_exponents)
    int32_t g = 0, n_trgsw = 0;
    size_t bytes = 0;                   // of the three together
};

// a TRLWE switching key (rtfhe_trlwe_ksk_create): the rows of every exponent as spectra on the primary device, with the exponents and the
// inverses the kernel gathers by
struct rtfhe_trlwe_ksk {
    rtfhe_ctx* ctx = nullptr;
    rtfhe::cplx* d_spec = nullptr;      // [n_t][l][2][R][64]: row j of entry e as (b, a) (rtfhe_kernels_trlwe_auto.hpp)
    int32_t n_t = 0;
    int32_t t[64] = {}, tinv[64] = {};  // t[e], and t[e]^-1 mod 2N
};

namespace rtfhe_host {

using rtfhe::BootstrapArgs;

// what a bootstrap launch reads its test polynomials from: tv null = the gates' own (k_bootstrap_*), else the k_pbs_* twins with table
// idx[g] of tv (idx null: table 0) for gate g of the launch
// (shift >= 0: a many-LUT PBS with 2^shift outputs per gate, the k_pbs_many_* kernels in MODE_EXTRACT, launch_pbs_many; enc: tv holds
// encrypted rows [n_tv][2][N], the k_pbs_enc_* kernels, which need shift >= 0; rounded: the rounded gadget decomposition, the k_pbs_round_*
// kernels, which need shift >= 0 too -- a plain-table PBS in rounded mode is a many-LUT PBS with shift = 0)
struct LutRef { const uint32_t* tv = nullptr; const int32_t* idx = nullptr; int32_t n_tv = 0; int32_t shift = -1; bool enc = false; bool rounded = false; };
inline LutRef lut_segment(LutRef l, size_t off) { if (l.idx) l.idx += off; return l; }     // ... for the segment starting at gate `off`
inline LutRef lut_on(const rtfhe_lut* lut, int entry, const int32_t* d_idx, int32_t shift = -1) {
    return lut ? LutRef{lut->d_tv[entry], d_idx, lut->n_lut, shift, lut->encrypted, lut->ctx && lut->ctx->decomp == RTFHE_DECOMP_ROUNDED} : LutRef{};
}
// the path of a one-output PBS with this table: the many-LUT path (shift 0) for an encrypted table and in rounded mode, else the fused kernels (-1)
// does a leveled entry point of this context launch the ROUNDED = true twin of its kernel?
inline bool leveled_rounded(const rtfhe_ctx* ctx) { return ctx->leveled_decomp == RTFHE_DECOMP_ROUNDED; }
inline int32_t pbs_shift(const rtfhe_ctx* ctx, const rtfhe_lut* lut) { return (lut->encrypted || ctx->decomp == RTFHE_DECOMP_ROUNDED) ? 0 : -1; }
using rtfhe::cplx;

constexpr int KSQ = 3;        // uint4 loads per lane per key-switch row: rows up to 768 words
constexpr int NPAD_MAX = 256 * KSQ;                 // n + 1 <= 768 (rtfhe_ctx_create): the largest npad = (n + 1) rounded up to 64 a kernel is sized for
constexpr size_t LDS_LIMIT = (size_t)160 * 1024;    // LDS of a gfx950 CU = the most dynamic LDS one workgroup can be granted
// the time-sliced launches (k_bootstrap_pair_rr, k_bootstrap_xpair_rr): as many gates per CU, five .. GMAX, as a mask length leaves room for; 0 = none
template <typename Lds>
constexpr int rr_fit(int npad) {
    int fit = 0;
    for (int g = 5; g <= Lds::GMAX; g++)
        if (Lds::bytes(g, npad) <= LDS_LIMIT) fit = g;
    return fit;
}
constexpr int KSMM_MT = 4;    // gate tiles (of 16) per wave of k_key_switch_mm

// ---- errors (rtfhe_context.hip) ----
int fail(rtfhe_ctx* ctx, int code, const std::string& msg);
const std::string& last_error_of_thread();
#define HIPCHECK(ctx, expr)                                                                                     \
    do {                                                                                                        \
        hipError_t e__ = (expr);                                                                                \
        if (e__ != hipSuccess)                                                                                  \
            return rtfhe_host::fail(ctx, RTFHE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));    \
    } while (0)

inline size_t bk_cplx_count(const rtfhe_params& p) { return (size_t)p.n * 2 * 2 * p.l * (p.N / 2); }
inline size_t bk_word_count(const rtfhe_params& p) { return (size_t)p.n * 2 * 2 * p.l * p.N; }
inline size_t ksk_rows(const rtfhe_params& p) { return (size_t)p.N * p.ks_t * ((1 << p.ks_basebit) - 1); }

// ---- context helpers (rtfhe_context.hip) ----
int use(rtfhe_ctx* ctx);                                                  // null check + hipSetDevice
int ensure(rtfhe_ctx* ctx, void** ptr, size_t* cap, size_t bytes);        // grow-only device buffer
int allow_lds_raw(rtfhe_ctx* ctx, const void* kernel, size_t bytes);      // raises the kernel's dynamic-LDS limit on this device once
template <typename K>
int allow_lds(rtfhe_ctx* ctx, K kernel, size_t bytes) { return allow_lds_raw(ctx, reinterpret_cast<const void*>(kernel), bytes); }
bool is_pinned_host(const void* p);
int copy_in(rtfhe_ctx* ctx, void* dst, const void* src, size_t bytes, int slot);      // host -> device on ctx->stream
int copy_out(rtfhe_ctx* ctx, void* dst, const void* src, size_t bytes, int slot);     // device -> host on ctx->stream, synchronous on return
// what a *_dev entry point (and a circuit's creation) asks of its pointers before anything is launched: every `required` one and every non-null
// `optional` one memory that a kernel on ctx->device may dereference, else RTFHE_ERR_INVALID "`name` needs device pointers ..."; nothing is allocated unless it refuses
int device_pointers(rtfhe_ctx* ctx, const char* name, std::initializer_list<const void*> required, std::initializer_list<const void*> optional = {});
// host-pointer forms: up to two optional host int32 arrays of `words` each staged back to back in the staging buffer *buf (d_a / d_b with its cap),
// copied from the caller's memory on ctx->stream (not through the pinned slots); d: their device addresses, null where the input is null
struct StagedIdx { const int32_t* first = nullptr; const int32_t* second = nullptr; };
int stage_idx(rtfhe_ctx* ctx, void** buf, size_t* cap, size_t words, const int32_t* first, const int32_t* second, StagedIdx& d);
void circuit_release(rtfhe_circuit* c);                                   // rtfhe_circuit.hip
// ---- circuits in the making (rtfhe_circuit.hip; the recorder's rule: DESIGN.md 6.1) ----
// a circuit that no context lists yet: released and deleted when its *_create returns without having handed it to the caller
struct CircuitDrop { void operator()(rtfhe_circuit* c) const { circuit_release(c); delete c; } };
typedef std::unique_ptr<rtfhe_circuit, CircuitDrop> NewCircuit;
// its own device buffers: every (pointer, bytes) allocated and listed in c->d_owned; a failed one is RTFHE_ERR_HIP "`name`: hipMalloc"
int circuit_own(rtfhe_ctx* ctx, rtfhe_circuit* c, const char* name, std::initializer_list<std::pair<void**, size_t>> bufs);
// a table's rows in bytes (an encrypted table's rows are TRLWEs: 2N words), and what both circuit kinds over a table put into their buffers before
// the recording: the description's words, the circuit's own copy of the rows, `zero_bytes` of zeros; a failure is "`name`: hipMemcpy / hipMemset"
inline size_t lut_bytes(const rtfhe_ctx* ctx, const rtfhe_lut* lut) { return (size_t)lut->n_lut * ctx->p.N * (lut->encrypted ? 2 : 1) * 4; }
int circuit_fill(rtfhe_ctx* ctx, const char* name, void* d_desc, const std::vector<int32_t>& desc, void* d_tv, const rtfhe_lut* lut, void* d_zero, size_t zero_bytes);
// THE recorder of every circuit kind: waits for ctx->stream, captures what enqueue() launches on it (ctx->tlwe1_capture = capture_samples
// meanwhile) into c's graph, moves the launches counted meanwhile from the context's counter to c->launches, instantiates, lists c in
// ctx->circuits and hands it out.  enqueue() returns the library's int; its error is reported before the capture's.
int circuit_record(rtfhe_ctx* ctx, NewCircuit c, StreamScratch* capture_samples, rtfhe_circuit** out, const std::function<int()>& enqueue);
void lut_release(rtfhe_lut* lut);                                         // frees a table's device copies (rtfhe_lut.hip)
void trgsw_release(rtfhe_trgsw* t);                                       // frees a selector set's spectra (rtfhe_cmux_tree.hip)
void packing_key_release(rtfhe_packing_key* k);                           // frees a packing key's matrix (rtfhe_pack.hip)
void plain_release(rtfhe_plain* w);                                       // frees a plain set's spectra (rtfhe_plain.hip)
void dense_release(rtfhe_dense* w);                                       // frees a dense layer's matrix and correction words (rtfhe_dense.hip)
void mbk_release(rtfhe_mbk* k);                                           // frees a multi-bit key's spectra and tables (rtfhe_pbs_mb.hip)
void trlwe_ksk_release(rtfhe_trlwe_ksk* k);                               // frees a TRLWE switching key's spectra (rtfhe_trlwe_auto.hip)
int prime_trgsw_mac(rtfhe_ctx* ctx);                                      // grants the TRLWE x TRGSW product's twins their LDS (rtfhe_trgsw_mac.hip)
// ---- seeded ciphertexts (rtfhe_seeded.hip; the checks themselves: rtfhe_seeded.cpp, host only) ----
// rtfhe_seeded_plan at the context's N with its refusal as the context's error (what: RTFHE_SEEDED_DEVICE / _UPLOAD of rtfhe_seeded_plan.h)
int seeded_ready(rtfhe_ctx* ctx, const char* name, int what, const void* seed, uint64_t first_row, const void* b, int group, const void* out, size_t rows);
// the one launch of k_seeded_expand on s: d_out [rows / group][2][group][N] from the seed and d_b [rows][N]; arguments already checked
int launch_seeded_expand(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* d_b, int group, uint32_t* d_out, size_t rows, hipStream_t s);
// what a *_seeded upload call does where its unseeded twin copies the caller's words in: the host b halves up through ctx->d_b, then the expansion into
// d_full, both queued on ctx->stream
int stage_seeded(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int group, size_t rows, void* d_full);
// the same two for lvl0 rows (rtfhe_tlwe_seeded_plan at the context's n; k_tlwe_seeded_expand): d_out rows of `stride` >= n + 1 words, of which
// columns 0 .. n are written -- the masks, then d_b [rows]
int tlwe_seeded_ready(rtfhe_ctx* ctx, const char* name, int what, const void* seed, uint64_t first_row, const void* b, const void* out, size_t rows);
int launch_tlwe_seeded_expand(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* d_b, uint32_t* d_out, size_t stride, size_t rows,
                              hipStream_t s);
// ---- the lifetime rule of the handles (rtfhe_context.hip) ----
// a handle as a call's check sees it: its noun and type name for the messages, whether the caller gave one, and the context it hangs on
struct HandleRef { const char* noun; const char* type; bool given; const rtfhe_ctx* owner; };
inline HandleRef ref(const rtfhe_lut* h) { return {"table", "rtfhe_lut", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_trgsw* h) { return {"selector set", "rtfhe_trgsw", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_packing_key* h) { return {"packing key", "rtfhe_packing_key", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_plain* h) { return {"plain set", "rtfhe_plain", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_dense* h) { return {"dense layer", "rtfhe_dense", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_mbk* h) { return {"multi-bit key", "rtfhe_mbk", h != nullptr, h ? h->ctx : nullptr}; }
inline HandleRef ref(const rtfhe_trlwe_ksk* h) { return {"switching key", "rtfhe_trlwe_ksk", h != nullptr, h ? h->ctx : nullptr}; }
// The ownership check of the one or two handles of a call made on ctx (a call made through a handle alone passes that handle's own context,
// null for a null handle): first every null one (RTFHE_ERR_INVALID "null NOUN (TYPE)"), then every one whose context is gone (RTFHE_ERR_STATE),
// then every one of another context (RTFHE_ERR_INVALID).
int handles_ready(rtfhe_ctx* ctx, std::initializer_list<HandleRef> handles);
// a handle destroyed before its context leaves the context's list of live handles
template <typename H>
void detach(std::vector<H*>& live, H* h) {
    for (size_t i = 0; i < live.size(); i++) if (live[i] == h) { live.erase(live.begin() + i); break; }
}
// a context destroyed before its handles: their device memory goes now, the handles stay valid for their destroy call, which then only frees them
template <typename H>
void orphan_all(std::vector<H*>& live, void (*release)(H*)) {
    for (H* h : live) { release(h); h->ctx = nullptr; }
    live.clear();
}
// ---- the handle owner (the rule: DESIGN.md 6.1) ----
// A data handle that no context lists yet, `ctx` set: released (X_release, after the one hipGetLastError() that clears what made the creation
// fail) and deleted when its *_create returns without having published it.  No *_create rolls back by hand.
template <typename H>
struct HandleDrop {
    void (*release)(H*);
    void operator()(H* h) const { (void)hipGetLastError(); release(h); delete h; }
};
template <typename H>
using NewHandle = std::unique_ptr<H, HandleDrop<H>>;
template <typename H>
NewHandle<H> new_handle(rtfhe_ctx* ctx, void (*release)(H*)) {
    NewHandle<H> h(new H(), HandleDrop<H>{release});
    h->ctx = ctx;
    return h;
}
// THE place a data handle is listed in its context and handed out
template <typename H>
int handle_publish(std::vector<H*>& live, NewHandle<H> h, H** out) {
    live.push_back(h.get());
    *out = h.release();
    return 0;
}
// THE body of the seven rtfhe_*_destroy: a handle still attached leaves its context's list and, after before(ctx) -- what has to happen while its
// device memory still stands --, releases that memory; then it is freed
template <typename H, typename Before>
void handle_destroy(std::vector<H*> rtfhe_ctx::*live, H* h, void (*release)(H*), Before before) {
    if (!h) return;
    if (rtfhe_ctx* ctx = h->ctx) {     // still attached
        detach(ctx->*live, h);
        before(ctx);
        release(h);
    }
    delete h;
}
template <typename H>
void handle_destroy(std::vector<H*> rtfhe_ctx::*live, H* h, void (*release)(H*)) { handle_destroy(live, h, release, [](rtfhe_ctx*) {}); }

// ---- the host-buffer form (the rule: DESIGN.md 6.1) ----
// A staging buffer of the context with its capacity and the pinned slot its copies go through; a call says which carries what.
struct Staging { void** buf; size_t* cap; int slot; };
inline Staging staging_a(rtfhe_ctx* ctx) { return {&ctx->d_a, &ctx->cap_a, 0}; }
inline Staging staging_b(rtfhe_ctx* ctx) { return {&ctx->d_b, &ctx->cap_b, 1}; }
inline Staging staging_c(rtfhe_ctx* ctx) { return {&ctx->d_c, &ctx->cap_c, 2}; }
struct HostRows { Staging via; const void* rows; size_t bytes; };                     // the caller's input rows (rows null: the call has none)
struct HostResult { Staging via; void* out; size_t bytes; bool accumulate; };         // the caller's result; accumulate: it goes up first, through pinned slot 1
struct HostIdx { Staging via; size_t words; const int32_t* first; const int32_t* second; };      // one stage_idx request
// THE host-pointer form of a leveled call, behind its argument checks: the device made current; count = 0 returns before anything is allocated;
// the staging buffers grown; the index arrays, the rows and -- when accumulating -- the caller's result copied up; launch(d_rows, d_idx, d_out)
// on ctx->stream (d_idx[i]: the device addresses of request i); the result copied down, synchronous on return.
template <typename Launch>
int host_form(rtfhe_ctx* ctx, size_t count, const HostRows& in, const HostResult& res, std::initializer_list<HostIdx> idx, Launch launch) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (in.rows)
        if (int rc = ensure(ctx, in.via.buf, in.via.cap, in.bytes)) return rc;
    if (int rc = ensure(ctx, res.via.buf, res.via.cap, res.bytes)) return rc;
    StagedIdx d_idx[2];
    size_t i = 0;
    for (const HostIdx& r : idx)
        if (int rc = stage_idx(ctx, r.via.buf, r.via.cap, r.words, r.first, r.second, d_idx[i++])) return rc;
    if (in.rows)
        if (int rc = copy_in(ctx, *in.via.buf, in.rows, in.bytes, in.via.slot)) return rc;
    if (res.accumulate)
        if (int rc = copy_in(ctx, *res.via.buf, res.out, res.bytes, 1)) return rc;
    if (int rc = launch(in.rows ? (const void*)*in.via.buf : nullptr, d_idx, *res.via.buf)) return rc;
    return copy_out(ctx, res.out, *res.via.buf, res.bytes, res.via.slot);
}
// what every entry point over a selector set checks first (rtfhe_cmux_tree.hip): the handles (lut only with_table), the caller's other pointers
// (args_ok), the mirror backend -- who: "the CMUX tree runs", for the message
int selector_set_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, bool with_table, const rtfhe_lut* lut, bool args_ok, const char* who);
// what rtfhe_trgsw_create[_seeded] and rtfhe_trgsw_update[_seeded] share (rtfhe_cmux_tree.hip): n TRGSW samples, brought into ctx->d_a by
// stage(words), transformed into the spectra at dst_spec; queued on ctx->stream, which the caller then waits for
int convert_selectors(rtfhe_ctx* ctx, rtfhe::cplx* dst_spec, int32_t n, const std::function<int(size_t)>& stage);

// ---- twiddles (rtfhe_twiddles.hip) ----
bool unit_twiddles_ok(const HostTw& tw);
int upload_twiddles(rtfhe_ctx* ctx);

// ---- FP64 mirror backend (rtfhe_dispatch_fft.hip) ----
int prime_fft_kernels(rtfhe_ctx* ctx);                                    // grants every bootstrap kernel of the parameter set its dynamic LDS
int launch_bootstrap_fft(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s, const LutRef& lut);
// builds (outside any stream capture) the second key layouts the dispatch of a `count`-gate batch in `mode` will read; no-op when they stand
int ensure_bk_layouts(rtfhe_ctx* ctx, size_t count, int mode);
int rebuild_derived_keys(rtfhe_ctx* ctx);                               // after a key change: every derived key form that already exists, in place, now

// ---- exact-integer NTT backend (rtfhe_dispatch_ntt.hip) ----
int prime_ntt_kernels(rtfhe_ctx* ctx);
int ntt_prepare(rtfhe_ctx* ctx);                                          // tables + NTT-domain key on first use
int launch_bootstrap_ntt(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s);
int launch_extprod_ntt(rtfhe_ctx* ctx, const int32_t* d_idx, const uint32_t* d_in, uint32_t* d_out, int32_t count, hipStream_t s);

// ---- split-FFT exact backend (rtfhe_dispatch_xfft.hip) ----
int prime_xfft_kernels(rtfhe_ctx* ctx);
int xfft_prepare(rtfhe_ctx* ctx);                                         // table + split key spectra on first use
int xfft_table_ensure(rtfhe_ctx* ctx);                                    // the table alone (d_xtw), built if absent: what a plain set needs of this backend
int launch_bootstrap_xfft(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s);
int launch_extprod_xfft(rtfhe_ctx* ctx, const int32_t* d_idx, const uint32_t* d_in, uint32_t* d_out, int32_t count, hipStream_t s);
// tables / derived keys of whichever exact backend is selected (no-op on the mirror): allocates and synchronises, so outside stream captures only
int backend_prepare(rtfhe_ctx* ctx);

// ---- stage kernels (rtfhe_stages.hip) ----
int launch_fft(rtfhe_ctx* ctx, bool forward, rtfhe::FftArgs a, hipStream_t s);
int launch_bk_permute(rtfhe_ctx* ctx, const double* src, double* dst, size_t polys, int dir, hipStream_t s);
int launch_ksk_combine(rtfhe_ctx* ctx, const uint32_t* d_raw, hipStream_t s);
int launch_ksmat_build(rtfhe_ctx* ctx, const uint32_t* d_raw, int colgroups, hipStream_t s);
// the identity key switch of a whole batch as one exact i8 contraction (second launch of the split path)
int launch_key_switch_mm(rtfhe_ctx* ctx, const BootstrapArgs& a, const uint32_t* samples, hipStream_t s);
// the same key switch one wave per sample from the gathered key rows (k_key_switch_ext): contexts without the matrix form (RTFHE_KS_MM_MIN=0)
int launch_key_switch_ext(rtfhe_ctx* ctx, uint32_t* samples, uint32_t* d_out, size_t count, hipStream_t s);
// the extract tail of every entry point that leaves lvl1 samples behind (many-LUT PBS, tree, rotation, CMUX netlist): the identity key switch of
// `rows` samples into d_out [rows][n+1] -- without the matrix key _ext, else d_out zeroed (the K-slices add into it) and _mm
// (zero_out = false: d_out is zero already -- a LUT circuit's key-switched buffer, which k_lut_scatter clears)
int launch_key_switch_rows(rtfhe_ctx* ctx, uint32_t* samples, uint32_t* d_out, size_t rows, hipStream_t s, bool zero_out = true);
// ... and behind it the rows of skipped items as they were before the call (k_rows_restore, rtfhe_kernels.hpp: the one parked-row rule): row g
// was skipped when one of d_idx[g][0 .. per_row) lies outside [0, bound).  d_idx null: no row was skipped and nothing is launched -- unless the
// launch is `counted` (what rtfhe_timer_end reports): an entry point's count does not depend on its arguments, its restore is launched regardless.
int launch_key_switch_rows_restore(rtfhe_ctx* ctx, uint32_t* samples, uint32_t* d_out, size_t rows, const int32_t* d_idx, int32_t per_row, int32_t bound,
                                   bool counted, hipStream_t s);

// ---- batches (rtfhe_batch.hip) ----
int launch_bootstrap(rtfhe_ctx* ctx, int op, int mode, int steps, const void* d_in0, const void* d_in1, void* d_out,
                     size_t count, hipStream_t s, const int32_t* d_ops = nullptr, const int32_t* d_idx0 = nullptr,
                     const int32_t* d_idx1 = nullptr, const int32_t* d_idx_out = nullptr, int32_t num_wires = 0, const LutRef& lut = LutRef{});
// ---- per-stream scratch (rtfhe_batch.hip) ----
inline bool capturing(hipStream_t s) {      // is a stream capture under way on s?  (a failed query counts as one: nothing is allocated then)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
    return cs != hipStreamCaptureStatusNone;
}
// how a kind of scratch is allocated: `bufs` buffers (1 or 2) of unit_bytes per unit of cap each, at least min_cap units, whole tiles of `tile`
struct ScratchShape { int bufs; size_t unit_bytes, min_cap = 0, tile = 1; };
// the lvl1 sample buffer: at least 1024 samples, whole tiles of 16 (rtfhe::ext_slot), N + 1 words each
inline ScratchShape tlwe1_shape(const rtfhe_ctx* ctx) { return {1, ((size_t)ctx->p.N + 1) * 4, 1024, 16}; }
// The rule of every per-stream scratch buffer, applied to the one of stream s in `map` (own: a buffer that lives in no map and takes precedence
// -- a circuit's, tlwe1_capture).  Outside a capture (in_capture = capturing(s), asked once per call) a buffer that holds fewer than `need` units
// is replaced (grow_scratch); inside one nothing may be allocated: the buffer must hold the call already, else RTFHE_ERR_STATE with the caller's
// `refusal`, and the graph then owns its address (captured).  out: the buffer.
int stream_scratch(rtfhe_ctx* ctx, ScratchMap& map, hipStream_t s, bool in_capture, const ScratchShape& shape, size_t need, const char* refusal,
                   StreamScratch*& out, StreamScratch* own = nullptr);
// ... its eager half, also for a buffer that lives in no map: no-op when b holds `need` units, else device-sync (earlier launches may still read
// it), b cleared, the old buffers freed -- or retired to mux_retired when a graph holds them --, new ones allocated
int grow_scratch(rtfhe_ctx* ctx, StreamScratch& b, const ScratchShape& shape, size_t need);
inline int ensure_tlwe1(rtfhe_ctx* ctx, StreamScratch& b, size_t gates) { return grow_scratch(ctx, b, tlwe1_shape(ctx), gates); }
int run_host_bootstrap_one(rtfhe_ctx* ctx, int op, int mode, int steps, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count, size_t out_words);
int mux_host_one(rtfhe_ctx* ctx, const uint32_t* c, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count);
// a programmable bootstrap of host buffers on one device (lut_idx already checked; null = table 0)
// (lut.shift >= 0: a many-LUT PBS, out [count][2^shift][n+1])
int run_host_pbs_one(rtfhe_ctx* ctx, const LutRef& lut, const int32_t* lut_idx, const uint32_t* in, uint32_t* out, size_t count);
// a many-LUT PBS (lut.shift >= 0) of device buffers on one device: the k_pbs_many_* launch(es), then the key switch of count << shift samples
// (zero_out = false: d_out is zero already and is not cleared first -- a LUT circuit's key-switched buffer, which k_lut_scatter clears)
int launch_pbs_many(rtfhe_ctx* ctx, const LutRef& lut, const void* d_in, void* d_out, size_t count, hipStream_t s, bool zero_out = true);
int mux_dev_one(rtfhe_ctx* ctx, const void* d_c, const void* d_in0, const void* d_in1, void* d_out, size_t count, hipStream_t s);

// ---- several GPUs (rtfhe_multi.hip) ----
inline size_t shard_begin(size_t count, int d, int n_dev) { return count * (size_t)d / (size_t)n_dev; }     // contiguous ranges, sizes differ by at most one
int replicate(rtfhe_ctx* ctx, rtfhe_ctx* peer, const void* src, void** dst_of_peer, size_t bytes);           // the primary's copy of a key -> a peer, device to device
int sharded_host_bootstrap(rtfhe_ctx* ctx, int op, int mode, int steps, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count, size_t out_words);
int sharded_host_mux(rtfhe_ctx* ctx, const uint32_t* c, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count);
// a batch that LIVES ON THE PRIMARY DEVICE, sharded over the context's devices: op < 0 = MUX (d_c, d_in0, d_in1), else a gate batch (d_in0, d_in1)
// (lut: a programmable bootstrap, op = RTFHE_COPY, d_lut_idx its int32[count] indices on the primary or null; shift >= 0: a many-LUT PBS,
// 2^shift output rows per gate)
int sharded_dev_batch(rtfhe_ctx* ctx, int op, const void* d_c, const void* d_in0, const void* d_in1, void* d_out, size_t count, hipStream_t s,
                      const rtfhe_lut* lut = nullptr, const int32_t* d_lut_idx = nullptr, int32_t shift = -1);
int sharded_host_pbs(rtfhe_ctx* ctx, const rtfhe_lut* lut, const int32_t* lut_idx, const uint32_t* in, uint32_t* out, size_t count, int32_t shift = -1);

// words per gate of the output buffer, by mode (MODE_EXTRACT: the final TLWE rows; the lvl1 samples go to `ext`)
inline size_t mode_out_words(const BootstrapArgs& a, int N) { return a.mode == rtfhe::MODE_BLIND_ROTATE ? (size_t)2 * N : (size_t)a.n + 1; }

// `cnt` gates of a batch starting at gate `off` (plain batches advance the ciphertext pointers, netlist waves the index arrays)
inline BootstrapArgs batch_segment(const rtfhe_ctx* ctx, BootstrapArgs a, size_t off, size_t cnt, size_t out_words) {
    if (a.idx0) { a.ops += off; a.idx0 += off; a.idx1 += off; a.idx_out += off; }
    else { a.in0 += off * ((size_t)a.n + 1); a.in1 += off * ((size_t)a.n + 1); a.out += off * out_words; }
    if (a.ext) a.ext_first += (int32_t)off;     // one sample buffer per batch, tiled by batch-wide gate number (rtfhe::ext_slot)
    a.count = (int32_t)cnt;
    return a;
}

// The split path of a plain batch (whole rounds of the two-waves-per-gate kernels): blind rotation + sample extract of every gate
// (the bootstrap kernel in MODE_EXTRACT, launched by `blind_rotate`), then the key switch of the whole batch as one exact i8
// contraction on the matrix pipe (k_key_switch_mm) -- two launches back to back on the caller's stream, the lvl1 samples in between
// stay in HBM (4 MB per 1024 gates at N = 1024).
inline StreamScratch* tlwe1_of(rtfhe_ctx* ctx, hipStream_t s) {
    if (ctx->tlwe1_capture) return ctx->tlwe1_capture;
    auto it = ctx->tlwe1.find(s);
    return it == ctx->tlwe1.end() ? nullptr : &it->second;
}
inline bool split_ok(rtfhe_ctx* ctx, const BootstrapArgs& a, hipStream_t s) {
    if (!(a.mode == rtfhe::MODE_GATE && ctx->d_ksmat && ctx->ks_mm_min > 0 && (size_t)a.count >= (size_t)ctx->ks_mm_min)) return false;
    // A caller's own capture would bake THIS stream's scratch pointer into a graph the library does not own: a later, larger eager batch
    // on the stream frees and reallocates that buffer (ensure_tlwe1) and a replay then writes freed memory; a replay on another stream
    // would share the scratch with eager work on this one.  Only rtfhe_circuit_create's captures (which own their sample buffer) split.
    if (ctx->foreign_capture) return false;
    const StreamScratch* b = tlwe1_of(ctx, s);
    return b && (size_t)a.count <= b->cap;      // (the sample buffer is sized by ensure_tlwe1 before any launch or capture)
}
// blind_rotate(ctx, a', s) launches the bootstrap kernel(s) of the whole batch with a'.mode = MODE_EXTRACT: every gate's lvl1 sample goes to
// a'.ext in the key switch's operand order (rtfhe::ext_slot; segments of a batch advance ext_first, not the pointer) and its output row is zeroed for the key switch's atomics
template <typename F>
int launch_split(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s, F blind_rotate) {
    uint32_t* samples = tlwe1_of(ctx, s)->d[0];
    a.mode = rtfhe::MODE_EXTRACT; a.ext = samples;
    if (int rc = blind_rotate(ctx, a, s)) return rc;
    return launch_key_switch_mm(ctx, a, samples, s);
}

// ---- kernel shapes and their launches (the three rtfhe_dispatch_*.hip units) ----
// One launch, and the only place but two that moves ctx->launches (launch_key_switch_mm: one for a whole batch; rtfhe_circuit_launch: what a
// recording counted): grants the kernel its dynamic LDS (once per device, allow_lds_raw; at 0 bytes that calls nothing in HIP and notes the
// kernel in two maps), launches and checks.  counted: a launch that rtfhe_timer_end reports; the stage-level calls and the key builds are not.
// grant = false: the two per-sample key switches, whose LDS (4N bytes per wave) has never needed a grant and whose first launch of a context may
// sit in a circuit's capture, where nothing but launches may happen.
template <typename K, typename A>
int launch_kernel(rtfhe_ctx* ctx, K k, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a, bool counted = true, bool grant = true) {
    if (grant)
        if (int rc = allow_lds(ctx, k, lds)) return rc;
    hipLaunchKernelGGL(k, grid, block, lds, s, a);
    HIPCHECK(ctx, hipGetLastError());
    if (counted) ctx->launches++;
    return 0;
}

// ---- the leveled kernels (tree, demultiplexer, rotation, CMUX netlist, the mirror's external product) ----
// A kernel and its ROUNDED twin (rtfhe_set_leveled_decomposition) with their dynamic LDS; a wave per node, LEVELED_WAVES waves per workgroup at both N.
constexpr int LEVELED_WAVES = 4;
template <typename A>
struct LeveledTwins { void (*reference)(A); void (*rounded)(A); size_t lds; };
// defines name(ctx): the twins of family `kernel` at the context's ring, the template arguments stated once; the last argument is the LDS at LOGN
#define RTFHE_LEVELED_FAMILY(name, Args, kernel, ...)                                                                                                    \
    template <int LOGN>                                                                                                                                 \
    rtfhe_host::LeveledTwins<Args> name##_t() {                                                                                                          \
        return {kernel<LOGN, 3, 6, rtfhe_host::LEVELED_WAVES, false>, kernel<LOGN, 3, 6, rtfhe_host::LEVELED_WAVES, true>, __VA_ARGS__};                  \
    }                                                                                                                                                   \
    rtfhe_host::LeveledTwins<Args> name(const rtfhe_ctx* ctx) { return ctx->logn == 11 ? name##_t<11>() : name##_t<10>(); }
// grants both twins their LDS (where the first launch of a context may already sit in a stream capture)
template <typename A>
int prime_leveled(rtfhe_ctx* ctx, const LeveledTwins<A>& k) {
    if (int rc = allow_lds(ctx, k.reference, k.lds)) return rc;
    return allow_lds(ctx, k.rounded, k.lds);
}
// One launch over `waves` nodes: the twin of the leveled mode in force now, when the call is made.  The other twin is granted its LDS too: the
// eager call a capture rule asks for may have run in the other mode.
template <typename A>
int launch_leveled(rtfhe_ctx* ctx, const LeveledTwins<A>& k, size_t waves, hipStream_t s, const A& a, bool counted = true) {
    const bool r = leveled_rounded(ctx);
    if (int rc = allow_lds(ctx, r ? k.reference : k.rounded, k.lds)) return rc;
    return launch_kernel(ctx, r ? k.rounded : k.reference, dim3((unsigned)((waves + LEVELED_WAVES - 1) / LEVELED_WAVES)), dim3(64 * LEVELED_WAVES), k.lds, s, a, counted);
}

// The kernels of one shape, all with the same block size, LDS and key layout.  The exact backends have the gate kernel alone; a family of the FP64
// mirror has its twins beside it: the programmable bootstrap (k_pbs_*), the many-LUT PBS (k_pbs_many_*), the encrypted table (k_pbs_enc_*) and
// the last two under the rounded decomposition (k_pbs_round_*<.., false / true>).
template <typename A>
struct GateKernel { void (*gate)(A); };
template <typename A>
struct TwinKernels { void (*gate)(A); void (*pbs)(rtfhe::LutArgs<A>); void (*many)(rtfhe::ManyArgs<A>), (*enc)(rtfhe::ManyArgs<A>), (*many_round)(rtfhe::ManyArgs<A>), (*enc_round)(rtfhe::ManyArgs<A>); };
// ... of family k_bootstrap`suffix`, the template arguments stated once for all six
#define RTFHE_TWINS(suffix, ...)                                                                                                         \
    { k_bootstrap##suffix<__VA_ARGS__>, k_pbs##suffix<__VA_ARGS__>, k_pbs_many##suffix<__VA_ARGS__>, k_pbs_enc##suffix<__VA_ARGS__>,    \
      k_pbs_round##suffix<__VA_ARGS__, false>, k_pbs_round##suffix<__VA_ARGS__, true> }

// One launch of a kernel family: the gate kernel (k_bootstrap_*) or, for a programmable bootstrap (lut.tv set), its twin (k_pbs_*) with the
// family's own arguments wrapped in LutArgs.  The twins share shapes, LDS and key layouts, so every choice of the dispatch is made once for all.
// A many-LUT PBS (lut.shift >= 0) takes k.many, in MODE_EXTRACT, and one with an encrypted table (lut.enc) k.enc, with the same arguments
// (ManyArgs); in rounded mode (lut.rounded) those two are replaced by k.many_round / k.enc_round.
template <typename A>
int launch_twin(rtfhe_ctx* ctx, const TwinKernels<A>& k, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a, const LutRef& lut) {
    if (lut.tv && lut.enc && lut.shift < 0) return fail(ctx, RTFHE_ERR_STATE, "an encrypted table runs on the many-LUT path only (launch_pbs_many)");
    if (lut.tv && lut.rounded && lut.shift < 0) return fail(ctx, RTFHE_ERR_STATE, "the rounded decomposition runs on the many-LUT path only (launch_pbs_many)");
    if (lut.tv && lut.shift >= 0) {
        rtfhe::ManyArgs<A> p{};
        p.base = a; p.tv = lut.tv; p.tv_idx = lut.idx; p.n_tv = lut.n_tv; p.t = lut.shift;
        return launch_kernel(ctx, lut.rounded ? (lut.enc ? k.enc_round : k.many_round) : (lut.enc ? k.enc : k.many), grid, block, lds, s, p);
    }
    if (lut.tv) return launch_kernel(ctx, k.pbs, grid, block, lds, s, rtfhe::LutArgs<A>{a, lut.tv, lut.idx, lut.n_tv});
    return launch_kernel(ctx, k.gate, grid, block, lds, s, a);
}
// (an exact backend's family: launch_bootstrap has refused a table before it gets here)
template <typename A>
int launch_twin(rtfhe_ctx* ctx, const GateKernel<A>& k, dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a, const LutRef&) {
    return launch_kernel(ctx, k.gate, grid, block, lds, s, a);
}
template <typename A>
int prime_kernels(rtfhe_ctx* ctx, const TwinKernels<A>& k, size_t lds) {
    if (int rc = allow_lds(ctx, k.gate, lds)) return rc;
    if (int rc = allow_lds(ctx, k.pbs, lds)) return rc;
    for (auto m : {k.many, k.enc, k.many_round, k.enc_round})
        if (int rc = allow_lds(ctx, m, lds)) return rc;
    return 0;
}
template <typename A>
int prime_kernels(rtfhe_ctx* ctx, const GateKernel<A>& k, size_t lds) { return allow_lds(ctx, k.gate, lds); }

// A shape -- a kernel family at one number of gates per workgroup -- is described once, by a struct Shape<GATES> with
//   kernels()          its GateKernel / TwinKernels
//   grid(count, cus)   workgroups for `count` gates on `cus` CUs, block(): threads of one
//   lds(npad)          dynamic LDS bytes at this mask length
//   args(ctx, b)       BootstrapArgs wrapped into the family's own argument struct
// and a Family lists the GATES a shape exists for.  The dispatch launches through Family::launch and prime_*_kernels grants LDS through
// Family::prime, so what can be launched and what is primed are one list; a gate count outside it is an error, not a new instantiation.
template <int GATES, int THREADS_PER_GATE>
struct GatesPerWorkgroup {      // GATES gates per workgroup, the last workgroup partly filled
    static dim3 grid(int count, int) { return dim3((count + GATES - 1) / GATES); }
    static dim3 block() { return dim3(THREADS_PER_GATE * GATES); }
};
struct WorkgroupPerCu {         // the time-sliced kernels: the gates shared evenly by one 8-wave workgroup per CU
    static dim3 grid(int, int cus) { return dim3(cus); }
    static dim3 block() { return dim3(512); }
};
template <template <int> class Shape, int... GATES>
struct Family {
    static int launch(rtfhe_ctx* ctx, int gates, const BootstrapArgs& b, hipStream_t s, const LutRef& lut = LutRef{}) {
        int rc = 0;
        if (((gates == GATES && ((rc = launch_twin(ctx, Shape<GATES>::kernels(), Shape<GATES>::grid(b.count, ctx->num_cus), Shape<GATES>::block(), Shape<GATES>::lds(b.npad), s,
                                                   Shape<GATES>::args(ctx, b), lut)), true)) || ...)) return rc;
        return fail(ctx, RTFHE_ERR_STATE, "no kernel shape of this family takes " + std::to_string(gates) + " gates per workgroup (" + std::to_string(b.count) + " gates on " +
                                              std::to_string(ctx->num_cus) + " CUs)");
    }
    // (most: the shapes of up to `most` gates only, where a long mask leaves room for fewer)
    static int prime(rtfhe_ctx* ctx, int npad, int most = INT_MAX) {
        int rc = 0;
        ((rc = rc || GATES > most ? rc : prime_kernels(ctx, Shape<GATES>::kernels(), Shape<GATES>::lds(npad))), ...);
        return rc;
    }
    static constexpr bool fits(int npad, int most = INT_MAX) { return ((GATES > most || Shape<GATES>::lds(npad) <= LDS_LIMIT) && ...); }
};

// ---- the ladder every backend's dispatch walks ----
// Whole rounds of round_gates gates per CU, then the remainder with ceil(rem / CUs) gates per workgroup, one workgroup per CU (a gate's waves then
// share their SIMDs with fewer other waves: a tail of 1-3 gates per CU takes 0.67 x the time of a full round instead of all of it).
struct LadderSplit { size_t full, rem; int tail_gates; };
constexpr LadderSplit ladder_split(size_t count, size_t cus, int round_gates) {
    const size_t round = (size_t)round_gates * cus, full = count / round * round, rem = count - full;
    return {full, rem, (int)((rem + cus - 1) / cus)};
}
constexpr bool ladder_is(size_t count, size_t cus, int round_gates, size_t full, size_t rem, int tail_gates) {
    const LadderSplit sp = ladder_split(count, cus, round_gates);
    return sp.full == full && sp.rem == rem && sp.tail_gates == tail_gates;
}
static_assert(ladder_is(0, 256, 4, 0, 0, 0) && ladder_is(1, 256, 4, 0, 1, 1) && ladder_is(256, 256, 4, 0, 256, 1) && ladder_is(257, 256, 4, 0, 257, 2), "tails of one and two gates per CU");
static_assert(ladder_is(1023, 256, 4, 0, 1023, 4) && ladder_is(1024, 256, 4, 1024, 0, 0) && ladder_is(1025, 256, 4, 1024, 1, 1), "around one whole round");
static_assert(ladder_is(767, 256, 3, 0, 767, 3) && ladder_is(768, 256, 3, 768, 0, 0) && ladder_is(1025, 256, 3, 768, 257, 2), "rounds of three gates per CU");

// The segments are queued back to back on stream s: launch(segment, its tables, gates per workgroup, tail) once for the whole rounds (tail =
// false) and once for the remainder.  A plain batch that may take the split path (split_ok) walks the ladder in MODE_EXTRACT and ends in the
// batch key switch.  merge_last: the backend's own condition for its time-sliced kernel -- the last whole round rides with the remainder in one
// tail of round_gates + 1 .. + 2 gates per CU.  A programmable bootstrap's table indices travel with the ciphertexts of each segment.
template <typename F>
int walk_ladder(rtfhe_ctx* ctx, const BootstrapArgs& a, hipStream_t s, const LutRef& lut, int round_gates, bool merge_last, F launch) {
    if (split_ok(ctx, a, s))
        return launch_split(ctx, a, s, [&](rtfhe_ctx* c, const BootstrapArgs& b, hipStream_t st) { return walk_ladder(c, b, st, lut, round_gates, merge_last, launch); });
    const size_t cus = (size_t)ctx->num_cus, out_words = mode_out_words(a, ctx->p.N);
    LadderSplit sp = ladder_split((size_t)a.count, cus, round_gates);
    if (merge_last) sp = {sp.full - round_gates * cus, sp.rem + round_gates * cus, sp.tail_gates + round_gates};
    if (sp.full)
        if (int rc = launch(batch_segment(ctx, a, 0, sp.full, out_words), lut, round_gates, false)) return rc;
    return sp.rem ? launch(batch_segment(ctx, a, sp.full, sp.rem, out_words), lut_segment(lut, sp.full), sp.tail_gates, true) : 0;
}

}  // namespace rtfhe_host
