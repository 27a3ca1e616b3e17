/*
 * rtfhe.h -- C ABI of librtfhe_hip.so, the MI355X (gfx950) engine for the HomNAND hot path of
 * hideki1217/rusTfhe.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo root):
 *
 *   rtfhe_ctx_create / _destroy      <- thread_local FFT_MAP + Spqlios_new / Spqlios_destructor
 *                                       (utils/src/math.rs:349-360, utils/src/spqlios.rs:18-20,139-145)
 *   rtfhe_ctx_create_multi           <- (no reference counterpart: it is single-threaded, tlwe.rs:264 TODO) one context over the
 *                                       GPUs of a node; the same batch calls then shard gates over them
 *   rtfhe_load_bk_torus              <- BootstrappingKey::new's TRGSWRepF::from (hom_nand/src/tfhe.rs:119-126,
 *                                       hom_nand/src/trgsw.rs:68-76)
 *   rtfhe_load_bk_fft                <- BootstrappingKey(Vec<TRGSWRepF>) as the reference holds it (tfhe.rs:116)
 *   rtfhe_load_ksk_ref               <- KeySwitchingKey(Vec<[[TLWERep<M>; IKS_T]; IKS_L]>) = [[TLWERep; 4]; 8] per coefficient, exactly as
 *                                       the reference holds it (hom_nand/src/tlwe.rs:178-180, 243-245): entry [i][l][t-1] = get(i, l, t),
 *                                       t = 1 .. 4 (:252-283)
 *   rtfhe_load_ksk                   <- the same key without the entry t = 4 of every level, which identity_key_switch never reads
 *                                       (its digits are basebit = 2 bits wide, tlwe.rs:43-73): [[TLWERep; 3]; 8]
 *   rtfhe_gate_batch[_dev]           <- TFHE::hom_nand/and/or/xor/not (hom_nand/src/tfhe.rs:41-71), count gates at once
 *   rtfhe_mux_batch[_dev]            <- TFHE::hom_mux (tfhe.rs:27-40)
 *   rtfhe_circuit_wave_dev           <- eval_logic_expr over impl Logip for TFHE (nander/src/lib.rs:40-89), one level at a time
 *   rtfhe_circuit_create / _launch   <- the same evaluation, all levels of a netlist recorded once and replayed as one submission
 *   rtfhe_bootstrap_batch[_dev]      <- TFHE::bootstrap (tfhe.rs:73-80)
 *   rtfhe_blind_rotate_batch         <- TFHE::blind_rotate with the gate test vector (tfhe.rs:81-113)
 *   rtfhe_lut_* / rtfhe_pbs_batch[_dev]  (no reference counterpart: its test vector is fixed to 1/8) the same bootstrap with
 *                                       caller-supplied test polynomials: programmable bootstrapping
 *   rtfhe_pbs_many_batch[_dev]       (no reference counterpart) several tables from one blind rotation: sample extract at indices
 *                                       0 .. n_out-1 (TRLWERep::sample_extract_index, hom_nand/src/trlwe.rs:110-121)
 *   rtfhe_lut_circuit_create         (no reference counterpart) netlists of many-LUT bootstraps of weighted wire sums, recorded once and
 *                                       replayed through rtfhe_circuit_launch
 *   rtfhe_lut_create_encrypted       (no reference counterpart) tables the server holds only as TRLWE ciphertexts: the blind rotation
 *                                       starts from TRLWERep encryptions (hom_nand/src/trlwe.rs) instead of the trivial (tv, 0)
 *   rtfhe_trgsw_create / rtfhe_cmux_tree_batch[_dev] / rtfhe_cmux_tree_extract_batch[_dev]
 *                                    <- TRGSWRepF::from and TRGSWRepF::cmux (hom_nand/src/trgsw.rs:68-76, 319-321) on caller-supplied TRGSW samples:
 *                                       one row out of 2^d rows of a table selected by d encrypted address bits (the reference has the CMUX,
 *                                       not the tree)
 *   rtfhe_trgsw_rotate_batch[_dev] / rtfhe_trgsw_rotate_extract_batch[_dev]
 *                                    <- one step of TFHE::blind_rotate (hom_nand/src/tfhe.rs:103-110) per caller-supplied TRGSW sample and exponent
 *   rtfhe_cmux_circuit_create / rtfhe_trgsw_update
 *                                    (no reference counterpart) netlists of such CMUXes -- decision diagrams over TRGSW-encrypted inputs --
 *                                       recorded once and replayed through rtfhe_circuit_launch
 *   rtfhe_packing_key_create / rtfhe_pack_batch[_dev] / rtfhe_lut_update_dev
 *                                    (no reference counterpart) TFHE's public packing key switch: lvl0 samples into TRLWE rows, with the digits of
 *                                       identity_key_switch (hom_nand/src/tlwe.rs:43-73) and TRLWE key rows (hom_nand/src/trlwe.rs) in the place of TLWE ones
 *   rtfhe_demux_tree_batch[_dev] / rtfhe_lut_accumulate_dev / rtfhe_lut_read_dev
 *                                    <- TRGSWRepF::cross (hom_nand/src/trgsw.rs:264-306) on caller-supplied TRGSW samples: the tree run backwards, one
 *                                       TRLWE into leaf `addr` of 2^d and zero into the others, and the leaves added into an encrypted table's rows
 *                                       (the reference has the product, not the demultiplexer)
 *   rtfhe_trlwe_extract_batch[_dev] / rtfhe_trlwe_extract_lvl1_batch[_dev]
 *                                    <- TRLWERep::sample_extract_index (hom_nand/src/trlwe.rs:110-121) at caller-chosen coefficients of TRLWEs that already
 *                                       exist, then TLWERep::identity_key_switch (hom_nand/src/tlwe.rs:43-73): leveled mode -> bootstrapped mode
 *   rtfhe_plain_create / rtfhe_trlwe_mul_plain_batch[_dev]
 *                                    <- Polynomial::cross (utils/src/math.rs:238-257) of both polynomials of a TRLWE row with a plain integer polynomial:
 *                                       the exact ciphertext x plaintext product, sums of up to eight per sample (the reference has the polynomial
 *                                       product, not the TRLWE operation)
 *   rtfhe_trlwe_mul_trgsw_batch[_dev] / rtfhe_trgsw_encrypt_polys[_deterministic]
 *                                    <- TRGSWRepF::cross (hom_nand/src/trgsw.rs:264-306) on caller-supplied TRGSW samples of small-integer polynomials
 *                                       (Crypto<i32> for TRGSW, trgsw.rs:118-138, with a polynomial in the bit's place), its fold-add carried over
 *                                       up to eight products per sample (the reference has the product, not the sum)
 *   rtfhe_trlwe_ksk_keygen[_deterministic] / rtfhe_trlwe_ksk_create / rtfhe_trlwe_auto_batch[_dev] / rtfhe_trlwe_automorphism
 *                                    <- TRGSWRepF::cross (hom_nand/src/trgsw.rs:264-306) with a switching key in the sample's place: the TRLWE -> TRLWE key
 *                                       switch, for the automorphisms X -> X^t and for re-keying (the reference has the product, not the key switch)
 *   rtfhe_dense_create / rtfhe_tlwe_dense_batch[_dev]
 *                                    <- the Add / scalar multiples of TLWERep (hom_nand/src/tlwe.rs) carried over a whole integer matrix: the weighted sums of
 *                                       lvl0 ciphertexts in front of a bootstrap (the reference has the row operations, not the layer)
 *   rtfhe_tlwe_compress_batch_dev / rtfhe_trlwe_compress_batch_dev / rtfhe_tlwe_compress / _expand / rtfhe_trlwe_compress / _expand
 *                                    (no reference counterpart) results rounded to k bits per word and bit-packed on the GPU, expanded by the key holder
 *   rtfhe_tlwe_expand_batch_dev / rtfhe_trlwe_expand_batch_dev
 *                                    (no reference counterpart) packed rows expanded on the GPU: stored or forwarded results as inputs again
 *   rtfhe_external_product_batch     <- Cross for TRGSWRepF (hom_nand/src/trgsw.rs:264-306)
 *   rtfhe_key_switch_batch          <- TLWERep::identity_key_switch (hom_nand/src/tlwe.rs:43-73)
 *   rtfhe_ifft_i32_batch             <- Spqlios_ifft_i32 / _u32 (utils/src/spqlios.rs:22-23, spqlios-wrapper.cpp:22-28)
 *   rtfhe_fft_u32_batch              <- Spqlios_fft_u32 (utils/src/spqlios.rs:25, spqlios-wrapper.cpp:34-36)
 *   rtfhe_ifft_f64_batch / _fft_f64_batch / _poly_mul_batch
 *                                    <- Spqlios_ifft / Spqlios_fft / Spqlios_poly_mul (spqlios-wrapper.cpp:18-20,30-32,38-53)
 *   rtfhe_keys_* / rtfhe_tlwe_write/read  (no reference counterpart: it has no serialization; fixes App. A's layouts into files)
 *   rtfhe_keygen / rtfhe_tlwe_*      <- TFHE::new, Cryptor::encrypto/decrypto(TLWE, ..) (tfhe.rs:21-25, tlwe.rs:213-241);
 *                                       randomness from the OS CSPRNG like the reference's thread_rng; *_deterministic = seeded, TEST ONLY
 *
 * Conventions: every call returns 0 on success or a negative rtfhe_status; nothing aborts or throws
 * across the ABI; rtfhe_last_error() gives the message of the last failure on that context.  The caller
 * owns every buffer.  Host-pointer calls copy in/out and are synchronous; *_dev calls take device
 * pointers, enqueue on the given hipStream_t (passed as void*) and return without synchronising.
 * A context is bound to one device (rtfhe_ctx_create) or to a set of devices (rtfhe_ctx_create_multi) and is not thread-safe (the reference's handle is not either:
 * one per thread, utils/src/math.rs:349-351).  There is NO CPU fallback: without a usable HIP device
 * rtfhe_ctx_create fails with RTFHE_ERR_NO_DEVICE.
 *
 * Flat little-endian layouts (the reference defines none):
 *   TLWE lvl0   u32[n+1]           a[0..n), b
 *   TLWE lvl1   u32[N+1]           a'[0..N), b'
 *   TRLWE       u32[2][N]          b(X), a(X)
 *   BK torus    u32[n][2][2l][N]   comp 0 = TRGSWRep.cipher rows, comp 1 = TRGSWRep.p_key rows
 *   BK fft      f64[n][2][2l][N]   same order; each poly an FrrSeries: Re[0..N/2) then Im[0..N/2),
 *                                  in the transform's native order (utils/src/spqlios.rs:147,205-208)
 *   KSK         u32[N][t][base-1][n+1]   rows d = 1 .. base-1 of level l of coefficient i   (rtfhe_load_ksk, rtfhe_keygen*)
 *   PK          u32[n][t][base-1][2][N]  packing key: row d = 1 .. base-1 of level j of coefficient i, a TRLWE (rtfhe_packing_keygen*)
 *   KSK (ref)   u32[N][t][base][n+1]     the reference's [[TLWERep; IKS_T]; IKS_L]: one more row (t = base) per level, never read
 *                                        (rtfhe_load_ksk_ref drops it)
 */
#ifndef RTFHE_H
#define RTFHE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtfhe_ctx rtfhe_ctx;

typedef struct {
    int32_t n;          /* TLWE lvl0 dimension    (635)   hom_nand/src/tlwe.rs:175  */
    int32_t N;          /* TRLWE degree           (1024)  hom_nand/src/trlwe.rs:76  */
    int32_t nbit;       /* log2(N)                (10)    hom_nand/src/tfhe.rs:16   */
    int32_t l;          /* gadget levels          (3)     hom_nand/src/trgsw.rs:115 */
    int32_t bgbit;      /* gadget base bits       (6)     hom_nand/src/trgsw.rs:112 */
    int32_t ks_t;       /* key-switch levels      (8)     hom_nand/src/tlwe.rs:178  */
    int32_t ks_basebit; /* key-switch base bits   (2)     hom_nand/src/tlwe.rs:179  */
} rtfhe_params;

typedef enum {
    RTFHE_NAND = 0, RTFHE_AND = 1, RTFHE_OR = 2, RTFHE_XOR = 3, RTFHE_NOT = 4, RTFHE_COPY = 5,
    RTFHE_ANDNY = 6   /* hom_and(-in0, in1): the second AND of hom_mux, hom_nand/src/tfhe.rs:34 */
} rtfhe_gate;

typedef enum {
    RTFHE_OK = 0,
    RTFHE_ERR_INVALID = -1,     /* bad argument / unsupported parameter set */
    RTFHE_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    RTFHE_ERR_HIP = -3,         /* a HIP runtime call failed */
    RTFHE_ERR_STATE = -4,       /* keys not loaded yet */
    RTFHE_ERR_NOMEM = -5
} rtfhe_status;

/* polynomial-multiply backend of the external product */
typedef enum {
    RTFHE_BACKEND_FFT64_MIRROR = 0,  /* default: FP64 transform mirroring the reference's spqlios operation for operation;
                                        outputs bit-identical to the reference CPU path */
    RTFHE_BACKEND_NTT_EXACT = 1,     /* exact negacyclic NTT mod P = 2^50 - 16383 (N = 1024 and 2048): reference semantics of the exact
                                        Polynomial::cross (utils/src/math.rs:238-257); bit-identical to an exact-integer
                                        evaluation, decrypt-level parity with the reference's FFT path */
    RTFHE_BACKEND_FFT_SPLIT_EXACT = 2 /* the same exact products (bit-identical to RTFHE_BACKEND_NTT_EXACT) through an FMA-contracted FP64 FFT:
                                        the key split into signed 16-bit halves, each half-product rounded to the nearest integer (distance from
                                        an integer proven < 2^-8 at N = 1024, < 2^-6 at N = 2048, for every input) and recombined mod 2^32;
                                        N = 1024 and 2048; needs the key in torus form; 1.4 x / 1.7 x the NTT backend's rate */
} rtfhe_backend;

/* ---- context ---- */
/* Sizes.  Every array a call takes or fills -- and the context's own scratch, 4 (N + 1) bytes per sample between the two launches of a batch:
 * 4.3 GB at a million gates -- may exceed 4 GiB: rows are addressed with 64-bit offsets wherever they lie, and a count is a size_t.  What bounds
 * a call is its number of ITEMS, stated with each entry point and refused with RTFHE_ERR_INVALID above it: count, count * P, count * K,
 * count << log2(n_out), count * depth or count * 2^(depth-1), rows * N / 16 and n_x are at most 2^31 - 1; the compressed results also keep
 * count * L, and a dense layer count * max(I, O) * (n + 1), below 2^31 words.  One item is at most 16 KiB (a TRLWE row at N = 2048).  Past that
 * only the device's memory bounds an array. */
void rtfhe_default_params(rtfhe_params *p);
int rtfhe_ctx_create(const rtfhe_params *p, int device_id, rtfhe_ctx **out);
/* One context over n_dev GPUs of the node (what a Rust `hom_nand_batch` binds for a whole-node batch).
 * device_ids[0] is the primary.  Keys loaded into the context are transformed once on the primary and copied
 * device-to-device to the others.  Every batch call shards contiguous gate ranges over the devices -- device d gets
 * [count d / n_dev, count (d+1) / n_dev) -- and outputs land at the same indices as on one device, bit-identical:
 *   - host-pointer calls (rtfhe_gate_batch, rtfhe_mux_batch, rtfhe_bootstrap_batch, rtfhe_blind_rotate_batch): one host thread and one
 *     stream per device, direct host<->device copies per device;
 *   - device-pointer calls (rtfhe_gate_batch_dev, rtfhe_mux_batch_dev, rtfhe_bootstrap_batch_dev): the batch lives on the PRIMARY device;
 *     every other device pulls its range over xGMI (hipMemcpyPeerAsync on its own stream), bootstraps it and pushes the outputs back,
 *     while the primary computes its own range; the caller's stream then waits for the other devices' events, so stream order holds as
 *     on one device and the call stays asynchronous.  Inside a stream capture the whole batch stays on the primary.
 * Netlist waves / circuits and stage-level calls run on the primary device only.  A device may be named more than once: every entry is
 * a full context of its own (stream, staging buffers, key replica). */
int rtfhe_ctx_create_multi(const rtfhe_params *p, const int *device_ids, int n_dev, rtfhe_ctx **out);
int rtfhe_ctx_device_count(const rtfhe_ctx *ctx);      /* devices behind this context (1 for rtfhe_ctx_create) */
/* device memory entry d (0 = primary) of the context holds right now, in bytes: the keys in every form built so far (second layouts of
 * the bootstrapping key are built by the first batch whose kernel shape reads them), staging and scratch buffers.  Not counted: the twiddle
 * tables (a few hundred KiB), the sample buffers of live circuits and the buffers of live LUT circuits (rtfhe_lut_circuit_create). */
int rtfhe_ctx_memory_bytes(const rtfhe_ctx *ctx, int d, size_t *bytes);
/* What the runtime reported about entry d (1 <= d < rtfhe_ctx_device_count) of a multi-device context against entry 0, the primary, when
 * rtfhe_ctx_create_multi set it up -- peer access is queried in both directions and enabled explicitly there, never left to a first copy -- and
 * how long that entry's share of the LAST device-resident sharded batch (rtfhe_gate_batch_dev / rtfhe_mux_batch_dev / rtfhe_bootstrap_batch_dev)
 * took on its own stream.  Nothing here is assumed: a field says what a HIP call returned on this machine. */
typedef struct rtfhe_peer_info {
    int32_t device;                   /* HIP device id of entry d */
    int32_t same_device;              /* 1: entry d names the primary's own device (a rehearsal on one card: no peer access involved) */
    int32_t can_access_from_primary;  /* hipDeviceCanAccessPeer(primary -> entry d) */
    int32_t can_access_to_primary;    /* hipDeviceCanAccessPeer(entry d -> primary) */
    int32_t enabled_from_primary;     /* hipDeviceEnablePeerAccess on the primary for entry d's device succeeded (or was already in force) */
    int32_t enabled_to_primary;       /* ... on entry d's device for the primary */
    uint32_t link_type;               /* hipExtGetLinkTypeAndHopCount(primary, entry d): 1 HyperTransport, 2 QPI, 3 PCIe, 4 InfiniBand, 5 xGMI;
                                       * 0xffffffff when the query failed or same_device */
    uint32_t hops;
    float scatter_ms;                 /* last sharded device-resident batch: entry d pulling its range of the inputs from the primary, */
    float compute_ms;                 /* bootstrapping it, */
    float gather_ms;                  /* pushing its outputs into the caller's buffer on the primary; -1 when there was no such batch yet,
                                       * the entry had no gates in it, or it has not completed (call rtfhe_sync first) */
} rtfhe_peer_info;
int rtfhe_ctx_peer_info(rtfhe_ctx *ctx, int d, rtfhe_peer_info *out);
/* the same questions about any two devices of the node, without a context (a one-process-per-GPU job prints this per rank): *can_access =
 * hipDeviceCanAccessPeer(dev_a -> dev_b), *link_type / *hops = hipExtGetLinkTypeAndHopCount (0xffffffff / 0 when the query fails).  Queries
 * only: nothing is enabled. */
int rtfhe_device_link(int dev_a, int dev_b, int32_t *can_access, uint32_t *link_type, uint32_t *hops);
/* the range [*begin, *end) of a `count`-gate host batch that entry d of an n_dev-device context bootstraps (no GPU needed) */
int rtfhe_shard_range(size_t count, int d, int n_dev, size_t *begin, size_t *end);
void rtfhe_ctx_destroy(rtfhe_ctx *ctx);
/* pinned host memory for ciphertext buffers: host-pointer calls DMA straight from / into such a buffer.  Any other host
 * pointer is handed to the runtime's own pageable-copy path (measured faster than staging it here); RTFHE_STAGING=1 in the
 * environment stages pageable buffers through the context's pinned buffers instead (one extra host copy). */
void *rtfhe_host_alloc(size_t bytes);
void rtfhe_host_free(void *p);
const char *rtfhe_last_error(const rtfhe_ctx *ctx);   /* ctx may be NULL: last ctx-less error */
const char *rtfhe_version(void);
int rtfhe_device_count(void);
int rtfhe_set_backend(rtfhe_ctx *ctx, int backend);   /* takes effect for subsequent calls; the NTT-domain key is derived from
                                                         the torus-form key (rtfhe_load_bk_torus) on first use */
int rtfhe_get_backend(const rtfhe_ctx *ctx);
/* twiddle tables in the reference's memory layout (2N doubles each direction; blocks 4 cos | 4 sin) */
int rtfhe_get_twiddles(const rtfhe_ctx *ctx, double *ifft_table, double *fft_table);
int rtfhe_set_twiddles(rtfhe_ctx *ctx, const double *ifft_table, const double *fft_table);
int rtfhe_ctx_params(const rtfhe_ctx *ctx, rtfhe_params *p);     /* the parameter set the context was created with */
/* The tables are DATA: the reference builds them with libm's cos / sin of a double-rounded angle (accurate_cos / accurate_sin,
 * utils/src/spqlios/spqlios-fft-impl.cpp:99-113), two hosts' libms may differ by an ulp in a few entries, and one differing entry changes
 * torus words.  rtfhe_ctx_create builds them with THIS host's libm -- what a reference built on this host would hold.  To
 * reproduce another build's bits, ship its tables as a file ("RTFHETW1" | i32 N | i32 0 | f64 ifft_table[2N] | f64 fft_table[2N] | u64 fnv1a):
 * rtfhe_twiddles_load installs the file's tables only if they differ from the context's (*entries_changed = differing entries, may be
 * NULL; a key loaded in torus form is re-transformed); rtfhe_twiddles_write saves the context's.  rustfhe_amd/assets/twiddles_N*.bin are
 * the tables of the reference build the golden vectors under tests/golden/ were made with. */
int rtfhe_twiddles_load(rtfhe_ctx *ctx, const char *path, int32_t *entries_changed);
int rtfhe_twiddles_write(const rtfhe_ctx *ctx, const char *path);
/* the same file format without a context (pure file I/O, checksum verified on read): N = ring degree, 2N doubles per table */
int rtfhe_twiddles_file_write(const char *path, int32_t N, const double *ifft_table, const double *fft_table);
int rtfhe_twiddles_file_read(const char *path, int32_t N, double *ifft_table, double *fft_table);

/* ---- keys ----
 * Loading a bootstrapping key (or new twiddle tables under a torus-form key) into a context that already holds one replaces it IN PLACE: the
 * spectra and every further form of the key that has been built (second kernel layouts, the exact backends' forms) are rebuilt in their
 * existing buffers before the call returns, on every device of the context.  A recorded circuit, or a capture the caller took around a *_dev
 * call, therefore replays against the new key.  One exception: a key given as spectra (rtfhe_load_bk_fft) has no torus form, the exact
 * backends' forms cannot follow it, and circuits recorded on those backends fail with RTFHE_ERR_STATE from then on (record them again after
 * loading a torus-form key); a caller's own capture of an exact-backend batch must be retaken in that case. */
int rtfhe_load_bk_torus(rtfhe_ctx *ctx, const uint32_t *bk /* [n][2][2l][N] */);
int rtfhe_load_bk_fft(rtfhe_ctx *ctx, const double *bk_f /* [n][2][2l][N] */);
int rtfhe_export_bk_fft(rtfhe_ctx *ctx, double *bk_f /* [n][2][2l][N] */);
int rtfhe_load_ksk(rtfhe_ctx *ctx, const uint32_t *ksk /* [N][t][base-1][n+1] */);
/* the reference's container flattened as it stands: [N][IKS_L = t][IKS_T = base][n+1], each TLWERep as a[0..n) then b */
int rtfhe_load_ksk_ref(rtfhe_ctx *ctx, const uint32_t *ksk_ref /* [N][t][base][n+1] */);

/* ---- the hot path: host buffers ---- */
int rtfhe_gate_batch(rtfhe_ctx *ctx, int op, const uint32_t *in0, const uint32_t *in1,
                     uint32_t *out, size_t count);            /* [count][n+1] each; in1 ignored for NOT/COPY */
int rtfhe_mux_batch(rtfhe_ctx *ctx, const uint32_t *c, const uint32_t *in0, const uint32_t *in1,
                    uint32_t *out, size_t count);
int rtfhe_bootstrap_batch(rtfhe_ctx *ctx, const uint32_t *tlwe, uint32_t *out, size_t count);

/* ---- the hot path: device buffers, asynchronous on `stream` (a hipStream_t, may be NULL) ---- */
int rtfhe_gate_batch_dev(rtfhe_ctx *ctx, int op, const void *d_in0, const void *d_in1, void *d_out,
                         size_t count, void *stream);
int rtfhe_mux_batch_dev(rtfhe_ctx *ctx, const void *d_c, const void *d_in0, const void *d_in1, void *d_out,
                        size_t count, void *stream);          /* d_out may alias none of the inputs.  The two intermediate batches live
                                                                 * in buffers of the context that belong to `stream` (MUX batches on different
                                                                 * streams may overlap).  Inside a caller's stream capture the call succeeds only
                                                                 * if an eager MUX batch of at least `count` gates ran on that stream before
                                                                 * (nothing may be allocated inside a capture): RTFHE_ERR_STATE otherwise; the
                                                                 * buffers a capture used are then kept until the context is destroyed. */
int rtfhe_bootstrap_batch_dev(rtfhe_ctx *ctx, const void *d_tlwe, void *d_out, size_t count, void *stream);
/* one dependency wave of a gate netlist (the build-side counterpart of nander's eager tree walk, nander/src/lib.rs:72-89):
 * gate g reads rows idx0[g] and idx1[g] of the wire table d_wires (u32[num_wires][n+1]), applies ops[g] and writes row
 * idx_out[g]; all four arrays are int32[count] in device memory.  Gates of one call must be independent.  Indices and
 * opcodes are validated on the device against num_wires: an offending gate is skipped (nothing is read or written through
 * it) and the next rtfhe_sync returns RTFHE_ERR_INVALID. */
int rtfhe_circuit_wave_dev(rtfhe_ctx *ctx, const void *d_ops, const void *d_idx0, const void *d_idx1,
                           const void *d_idx_out, void *d_wires, size_t num_wires, size_t count, void *stream);
/* A whole levelised netlist as ONE submission (BASELINE config 4; the reference walks its expression tree gate by gate,
 * nander/src/lib.rs:72-89): the waves wave_offsets[w] .. wave_offsets[w+1] (host array, num_waves + 1 entries) of the same four
 * device arrays are captured once into a HIP graph; rtfhe_circuit_launch replays it on `stream` (asynchronous, one runtime
 * call per evaluation).  The device arrays and the wire table must stay alive and in place while the circuit exists.  A circuit
 * is normally destroyed before its context; if the context goes first, the circuit's graph is released with it, a later
 * rtfhe_circuit_launch fails with RTFHE_ERR_STATE and rtfhe_circuit_destroy only frees the handle. */
typedef struct rtfhe_circuit rtfhe_circuit;
int rtfhe_circuit_create(rtfhe_ctx *ctx, const void *d_ops, const void *d_idx0, const void *d_idx1, const void *d_idx_out,
                         const int32_t *wave_offsets, int32_t num_waves, void *d_wires, size_t num_wires, rtfhe_circuit **out);
int rtfhe_circuit_launch(rtfhe_circuit *c, void *stream);
void rtfhe_circuit_destroy(rtfhe_circuit *c);
/* ---- programmable bootstrapping (PBS): the bootstrap with a test polynomial the caller chooses ----
 * For an input t = (a_0 .. a_{n-1}, b) in the lvl0 layout, SH = 32 - log2(N) - 1, gate g of a batch computes
 *     bbar = b >> SH ;  abar_i = (a_i + 2^(SH-1)) >> SH                 (the gates' own mod switch)
 *     acc  = X^{-bbar} (tv, 0),  tv = row lut_idx[g] of the table:  acc[c] = e < N ? tv[e] : -tv[e-N],  e = (c + bbar) mod 2N
 *     for i in 0 .. n:  acc = CMUX(bk_i, X^{abar_i} acc, acc)
 *     out[g] = identity_key_switch(sample_extract_0(acc))
 * With tv = 0x20000000 at every position the output equals rtfhe_bootstrap_batch's words (every batch shape, every count).
 * A table is uploaded once by rtfhe_lut_create, to every device of the context (each entry of an rtfhe_ctx_create_multi context holds a
 * copy); a PBS call allocates nothing for it, so rtfhe_pbs_batch_dev may sit inside a stream capture under the rule of
 * rtfhe_bootstrap_batch_dev (an eager batch of at least `count` gates must have run on that stream before).  A table is normally destroyed
 * before its context; if the context goes first, its device copies are released with it, a later PBS call with it fails with
 * RTFHE_ERR_STATE and rtfhe_lut_destroy only frees the handle.  lut_idx NULL = table 0 for every gate.
 *   rtfhe_pbs_batch      checks lut_idx against [0, n_lut) on the host: RTFHE_ERR_INVALID before anything is launched.
 *   rtfhe_pbs_batch_dev  checks each index on the device: a gate with a bad index is skipped (its output row is not a valid ciphertext)
 *                        and the next rtfhe_sync returns RTFHE_ERR_INVALID, as for netlist waves.
 * On a multi-device context both calls shard the batch as rtfhe_bootstrap_batch[_dev] do, each range with its own lut_idx range.
 * The FP64 mirror backend only: on RTFHE_BACKEND_NTT_EXACT / RTFHE_BACKEND_FFT_SPLIT_EXACT both calls fail with RTFHE_ERR_INVALID
 * (the context stays usable). */
typedef struct rtfhe_lut rtfhe_lut;
int rtfhe_lut_create(rtfhe_ctx *ctx, const uint32_t *tv /* [n_lut][N] */, int32_t n_lut, rtfhe_lut **out);
void rtfhe_lut_destroy(rtfhe_lut *lut);
int rtfhe_pbs_batch(rtfhe_ctx *ctx, const rtfhe_lut *lut, const int32_t *lut_idx /* [count] or NULL */,
                    const uint32_t *tlwe /* [count][n+1] */, uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_pbs_batch_dev(rtfhe_ctx *ctx, const rtfhe_lut *lut, const void *d_lut_idx /* int32[count] or NULL */,
                        const void *d_tlwe, void *d_out, size_t count, void *stream);
/* ---- many-LUT PBS: n_out = 2^t functions of one value from ONE blind rotation ----
 * Take an input t = (a_0 … a_{n−1}, b) and n_out = ϑ = 2^t with t ∈ {0,1,2,3}. Let SH = 32 − log2 N − 1 and S = SH + t.
 *
 *     bbar   = (b >> S) << t                                      (floor, as the gates)
 *     abar_i = (((a_i + 2^(S-1)) mod 2^32) >> S) << t            (round, as the gates; all values in [0, 2N), multiples of ϑ)
 *     acc    = X^{-bbar} (tv, 0),  tv = row lut_idx[g] of the table   (exactly as rtfhe_pbs_batch)
 *     for i in 0 .. n:  acc = CMUX(bk_i, X^{abar_i} acc, acc)
 *     out[g][j] = identity_key_switch(sample_extract_index(acc, j))   for j = 0 .. ϑ-1
 *
 * sample_extract_index(acc, j) is the reference's TRLWERep::sample_extract_index(j) (hom_nand/src/trlwe.rs:110-121):
 * a'_i = acc_a[j−i] for i ≤ j, −acc_a[N+j−i] otherwise, b' = acc_b[j].  With ϑ = 1 this is exactly rtfhe_pbs_batch.
 * A table for ϑ functions interleaves them: coefficient k ϑ + j serves function j (rustfhe_amd.pbs.many_lut_polynomial builds one).
 * n_out must be 1, 2, 4 or 8 (anything else: RTFHE_ERR_INVALID).  Outputs are [count][n_out][n+1]: the n_out rows of a gate lie together.
 * Tables, index checks (on the host before any launch / on the device, reported at the next rtfhe_sync), sharding over the entries of an
 * rtfhe_ctx_create_multi context and the refusal on the exact backends are rtfhe_pbs_batch[_dev]'s.  Inside a stream capture
 * rtfhe_pbs_many_batch_dev allocates nothing: an eager rtfhe_pbs_many_batch_dev of at least `count` gates and at least this n_out must have run
 * on that stream first (else RTFHE_ERR_STATE). */
int rtfhe_pbs_many_batch(rtfhe_ctx *ctx, const rtfhe_lut *lut, int32_t n_out, const int32_t *lut_idx /* [count] or NULL */,
                         const uint32_t *tlwe /* [count][n+1] */, uint32_t *out /* [count][n_out][n+1] */, size_t count);
int rtfhe_pbs_many_batch_dev(rtfhe_ctx *ctx, const rtfhe_lut *lut, int32_t n_out, const void *d_lut_idx /* int32[count] or NULL */,
                             const void *d_tlwe, void *d_out /* [count][n_out][n+1] */, size_t count, void *stream);
/* ---- encrypted tables: the test polynomial as a TRLWE ciphertext the server cannot read ----
 * An encrypted table holds n_lut rows, each a TRLWE u32[2][N] in the TRLWE layout (b(X) then a(X)) under the lvl1 key key1, e.g. from
 * rtfhe_trlwe_encrypt_torus of test polynomials built as for rtfhe_lut_create / rtfhe_pbs_many_batch.  For gate g with row (tb, ta)
 * everything is exactly rtfhe_pbs_many_batch -- the same bbar and abar_i (mod switch at SH + t for ϑ = 2^t outputs), the same n CMUX
 * steps, out[g][j] = identity_key_switch(sample_extract_index(acc, j)) -- except where the accumulator starts:
 *
 *     acc_b[c] = e < N ? tb[e] : -tb[e-N],   acc_a[c] = e < N ? ta[e] : -ta[e-N],   e = (c + bbar) mod 2N
 *
 * i.e. acc = X^{-bbar} (tb, ta).  A trivial encryption (ta = 0, tb = tv) gives word for word what the plain table tv gives through
 * rtfhe_pbs_batch[_dev] and rtfhe_pbs_many_batch[_dev] (every n_out, every batch shape).  The outputs decrypt under key0 as before; their
 * noise is the plain table's plus the table's own (alpha = 2^-25 from rtfhe_trlwe_encrypt_torus), carried through the rotation unchanged.
 * What the server learns: n_lut, each call's n_out, and which row each gate uses (lut_idx stays plaintext) -- not the rows' contents.
 *
 * rtfhe_lut_create_encrypted returns an ordinary rtfhe_lut: uploaded to every entry of the context as rtfhe_lut_create does, freed by
 * rtfhe_lut_destroy under the same lifetime rules, and accepted without a signature change by rtfhe_pbs_batch[_dev],
 * rtfhe_pbs_many_batch[_dev] and rtfhe_lut_circuit_create, with the same index checks, sharding and refusal on the exact backends.
 * rtfhe_pbs_batch[_dev] runs an encrypted table as rtfhe_pbs_many_batch[_dev] with n_out = 1 (MODE_EXTRACT, then the batch key switch);
 * so inside a stream capture rtfhe_pbs_batch_dev with an encrypted table follows rtfhe_pbs_many_batch_dev's capture rule: an eager call of
 * at least `count` gates (and, for the many entry, at least this n_out) must have run on that stream first (else RTFHE_ERR_STATE). */
int rtfhe_lut_create_encrypted(rtfhe_ctx *ctx, const uint32_t *trlwe /* [n_lut][2][N] */, int32_t n_lut, rtfhe_lut **out);
/* ---- rounded gadget decomposition: 4-bit messages through one PBS at N = 1024 ----
 * In every CMUX step each word x of the difference polynomials X^{abar_i} acc - acc becomes
 *
 *     u = ((x + MA) mod 2^32) ^ MX ;   digit j = the signed bgbit-wide field of u at bit 32 - bgbit (j+1),   j = 0 .. l-1
 *
 *   RTFHE_DECOMP_REFERENCE   MA = MX = make_decomp_mask(l, bgbit) (utils/src/math.rs:542-560), the reference's constants: 0x02084000 for
 *                            l = 3, bgbit = 6.  With them x - Sum_j d_j 2^(32 - bgbit (j+1)) lies in [-2^-17, 2^-18] of the torus with mean
 *                            -2^-19 at every coefficient; multiplied by the key that mean is most of a bootstrapped ciphertext's noise.
 *   RTFHE_DECOMP_ROUNDED     MX = Sum_{j=1..l} 2^(32 - bgbit j + bgbit - 1)  and  MA = MX + 2^(32 - l bgbit - 1):  0x82080000 and 0x82082000
 *                            for l = 3, bgbit = 6.  The digits are balanced (in [-2^(bgbit-1), 2^(bgbit-1) - 1]) and x is rounded to the
 *                            nearest multiple of 2^(32 - l bgbit): the error lies in [-2^-19, 2^-19) with mean ~0.
 *
 * Nothing else changes: not the mod switch, the transforms, the accumulation order, the truncation, the extract or the key switch, and the
 * bootstrapping key is the same.  A rounded-mode output is therefore NOT the reference's word; it decrypts to the same message with about a
 * fifth of the noise at N = 1024 (measured: DESIGN.md 5.12), which moves the PBS family from 2-bit to 4-bit messages there.
 *
 * The mode is a property of the context, RTFHE_DECOMP_REFERENCE until set, and is read by these calls only:
 *   rtfhe_pbs_batch[_dev], rtfhe_pbs_many_batch[_dev]   with plain and encrypted tables, when the call is made;
 *   rtfhe_lut_circuit_create                            which RECORDS the mode in force at creation: the circuit replays in that mode
 *                                                       whatever the context is set to later.
 * Gates, MUX, rtfhe_bootstrap_batch[_dev], gate circuits, rtfhe_blind_rotate_batch, rtfhe_external_product_batch and the leveled entry points
 * (CMUX tree, TRGSW rotation, CMUX netlists, packing) always use the reference decomposition unless rtfhe_set_leveled_decomposition (below)
 * says otherwise for some of them: the gate path stays bit-identical to the reference in either mode.  On a multi-device context the setter sets every entry.  Any other mode value: RTFHE_ERR_INVALID, the mode in force
 * stays.  The setter works on every backend; on the exact backends the PBS calls keep failing with RTFHE_ERR_INVALID as before.
 * In rounded mode rtfhe_pbs_batch[_dev] with a plain table runs as rtfhe_pbs_many_batch[_dev] with n_out = 1, as an encrypted table already
 * does; so inside a stream capture rtfhe_pbs_batch_dev in rounded mode follows rtfhe_pbs_many_batch_dev's capture rule: an eager call of at
 * least `count` gates must have run on that stream first (else RTFHE_ERR_STATE). */
typedef enum {
    RTFHE_DECOMP_REFERENCE = 0,
    RTFHE_DECOMP_ROUNDED = 1
} rtfhe_decomposition;
int rtfhe_set_decomposition(rtfhe_ctx *ctx, int mode);
int rtfhe_get_decomposition(const rtfhe_ctx *ctx);      /* the mode in force, or RTFHE_ERR_INVALID for a NULL context */
/* ---- the same choice for the leveled entry points: 6-bit table rows through a depth-8 tree and a 10-step rotation ----
 * A second, independent mode with the same two values and the same rules (host state only, RTFHE_DECOMP_REFERENCE until set, every entry
 * of a multi-device context set, NULL context or unknown mode: RTFHE_ERR_INVALID and the mode in force stays, accepted on every backend).
 * Neither setter touches the other's state; rtfhe_set_decomposition keeps meaning the PBS family only.  In a CMUX the decomposition error
 * is multiplied by the encrypted selector bit, so the reference constants' mean error shows only at levels whose bit is 1 (about 1e-3 of
 * the torus per such level at N = 1024); in rounded mode the selectors' own noise is what remains (measured: DESIGN.md 5.13).
 * The mode is read by these calls only:
 *   rtfhe_cmux_tree_batch[_dev], rtfhe_cmux_tree_extract_batch[_dev],
 *   rtfhe_trgsw_rotate_batch[_dev], rtfhe_trgsw_rotate_extract_batch[_dev]   when the call is made (inside a stream capture: when it is
 *                                                       captured; the capture rules of these calls hold in either mode);
 *   rtfhe_external_product_batch                        on the mirror backend, when the call is made.  On RTFHE_BACKEND_NTT_EXACT and
 *                                                       RTFHE_BACKEND_FFT_SPLIT_EXACT with the rounded leveled mode in force it returns
 *                                                       RTFHE_ERR_INVALID before anything is launched; in reference mode it runs there as before;
 *   rtfhe_cmux_circuit_create                           which RECORDS the mode in force at creation: the circuit replays in that mode
 *                                                       whatever the context is set to later.
 * Gates, MUX, rtfhe_bootstrap_batch[_dev], rtfhe_blind_rotate_batch, the PBS family, packing and the key switch behind the extract forms
 * never read it.  A rounded-mode output is NOT the reference's word; it decrypts to the same message. */
int rtfhe_set_leveled_decomposition(rtfhe_ctx *ctx, int mode);
int rtfhe_get_leveled_decomposition(const rtfhe_ctx *ctx);      /* the mode in force, or RTFHE_ERR_INVALID for a NULL context */
/* ---- LUT circuits: netlists of many-LUT bootstraps, recorded once and replayed as one submission ----
 * A LUT circuit works on the wire table d_wires, u32[num_wires][n+1] lvl0 ciphertexts in device memory, as a gate circuit does.  It is a
 * sequence of waves: wave w holds nodes wave_offsets[w] .. wave_offsets[w+1] (host array, num_waves + 1 entries, strictly increasing from
 * >= 0, as for rtfhe_circuit_create) and one n_out ϑ = wave_n_out[w] ∈ {1, 2, 4, 8}.  Node g of wave w computes
 *
 *     t     = Σ_k weights[g][k] · wire[in_idx[g][k]]     k = 0 .. fan_in-1; wrapping u32 arithmetic on all n+1 words; in_idx -1 = unused slot
 *     t.b  += cst[g]                                      a torus constant on the b word only (cst NULL: 0)
 *     out   = many-LUT PBS of t with table lut_idx[g] and ϑ outputs      (exactly rtfhe_pbs_many_batch; lut_idx NULL: table 0)
 *     wire[out_idx[r + j]] = out[j],  j = 0 .. ϑ-1,  r = Σ_{v<w} (nodes of v) · ϑ_v + (g - wave_offsets[w]) · ϑ
 *
 * i.e. out_idx lists the output wires wave by wave, node by node, starting with the first node of wave 0.  Every node of a wave reads the wire
 * table as it stood before the wave, so a wave may overwrite a wire it also reads (a carry updated in place); two nodes of one wave must not
 * write the same wire.  All description arrays are host memory (in_idx, weights: [nodes][fan_in] with fan_in 1 .. 8, indexed by the absolute
 * node number g; cst, lut_idx: [nodes]).  They are checked completely before anything is allocated or captured -- every index in range, each
 * n_out 1, 2, 4 or 8, no wire written twice in one wave, the wave_offsets rules -- and a failed check returns RTFHE_ERR_INVALID naming the wave
 * and the node, with nothing launched.  The FP64 mirror backend only: on either exact backend creation fails with RTFHE_ERR_INVALID.
 *
 * Each wave is recorded as three steps of one single-stream capture on the primary device: k_lut_gather writes the wave's sums into a
 * circuit-owned buffer, the many-LUT PBS (bootstrap in sample-extract mode, then the batch key switch) writes [count][ϑ][n+1] into another,
 * k_lut_scatter copies the rows to their wires.  The returned handle is an ordinary rtfhe_circuit: rtfhe_circuit_launch replays it (asynchronous),
 * rtfhe_circuit_destroy frees it, and the rules for a context destroyed first are rtfhe_circuit_create's.  Keys are read in place: a key
 * loaded on the context later is what the next replay computes with.  The wire table must stay alive and in place while the circuit exists;
 * nothing else must: the circuit owns its own copy of the description and of the table rows, so the rtfhe_lut may be destroyed right after
 * creation.  Its device footprint, not counted by rtfhe_ctx_memory_bytes (as for gate circuits' sample buffers):
 *     description      4 · (nodes · (2 fan_in + 2) + Σ_w nodes_w · ϑ_w)  bytes
 *     gathered inputs  4 · (n+1) · max_w nodes_w
 *     key-switched     4 · (n+1) · max_w nodes_w · ϑ_w
 *     sample buffer    4 · (N+1) · max(1024, max_w nodes_w · ϑ_w) rounded up to 16
 *     table rows       4 · N · n_lut  (an encrypted table: 4 · 2N · n_lut) */
int rtfhe_lut_circuit_create(rtfhe_ctx *ctx, const rtfhe_lut *lut, int32_t fan_in /* 1 .. 8 */,
                             const int32_t *in_idx /* [nodes][fan_in] */, const int32_t *weights /* [nodes][fan_in] */,
                             const uint32_t *cst /* [nodes] or NULL */, const int32_t *lut_idx /* [nodes] or NULL */,
                             const int32_t *wave_offsets /* [num_waves + 1] node offsets */, const int32_t *wave_n_out /* [num_waves] */,
                             int32_t num_waves, const int32_t *out_idx /* [Σ over nodes of its wave's n_out] */, void *d_wires,
                             size_t num_wires, rtfhe_circuit **out);
/* ---- CMUX-tree table lookup: one row out of 2^d, selected by TRGSW-encrypted address bits (TFHE's leveled mode) ----
 * A selector set holds n_sel TRGSW samples under the lvl1 key key1, each in the torus layout of ONE bootstrapping-key entry, u32[2][2l][N]
 * (comp 0 = TRGSWRep.cipher rows, comp 1 = TRGSWRep.p_key rows), e.g. from rtfhe_trgsw_encrypt_bits.  rtfhe_trgsw_create converts them as
 * rtfhe_load_bk_torus converts the key -- TRGSWRepF::from (hom_nand/src/trgsw.rs:68-76): the forward transform of the words viewed as signed
 * i32 -- and keeps the spectra on the primary device in the canonical device layout [2l][2][R][64].  The set owns its device copy and is
 * independent of the context's bootstrapping key: a context with no keys loaded runs rtfhe_cmux_tree_batch.  It is normally destroyed before
 * its context; if the context goes first, the spectra are released with it, a later tree call fails with RTFHE_ERR_STATE and
 * rtfhe_trgsw_destroy only frees the handle.
 *
 * Lookup g of a batch has the depth d = `depth` (1 .. 16, the same for the whole batch), selector indices sel_idx[g][0 .. d) -- entry k is
 * address bit k, least significant first -- and the first table row row0[g] of an rtfhe_lut with n_lut rows (plain or encrypted).  It computes
 *
 *     level 0 nodes   r_j = row (row0[g] + j),  j = 0 .. 2^d - 1;  a plain row tv is the trivial TRLWE (b = tv, a = 0), an encrypted row is (tb, ta)
 *     level k = 0 .. d-1:   r'_j = cmux(S_k, r_{2j+1}, r_{2j}) = cross(S_k, r_{2j+1} - r_{2j}) + r_{2j},   S_k = selector sel_idx[g][k]
 *     result          the single node left after level d - 1: a TRLWE of row row0[g] + sum_k bit_k 2^k
 *
 * The subtraction and the addition wrap on every word of both polynomials; cross is Cross for TRGSWRepF (trgsw.rs:264-306: gadget
 * decomposition of both polynomials, 2l forward transforms, multiply-accumulate against the selector's spectra in the order h = b then a,
 * digit 0 .. l-1, two inverse transforms with truncation), i.e. exactly what rtfhe_external_product_batch computes for a key entry.
 * sel_idx NULL: lookup g uses selectors g * depth + k.  row0 NULL: 0 for every lookup.
 *   rtfhe_cmux_tree_batch[_dev]          out[g] = the result, u32[2][N] (b then a): the row format rtfhe_lut_create_encrypted takes, so high address
 *                                        bits by CMUX tree and low bits by PBS compose into full vertical packing
 *   rtfhe_cmux_tree_extract_batch[_dev]  out[g] = identity_key_switch(sample_extract_index(result, coef[g])), u32[n+1]: coefficient coef[g] of the
 *                                        selected row as a lvl0 ciphertext (plaintext low address bits for free: N values per row).  coef NULL:
 *                                        index 0.  Needs the key-switching key (RTFHE_ERR_STATE otherwise), not the bootstrapping key.  The samples
 *                                        go through the batch key switch of rtfhe_pbs_many_batch (the stream's lvl1 sample buffer, then the key
 *                                        switch as one i8 contraction, or one wave per sample under RTFHE_KS_MM_MIN=0).
 * Checks: the handles, depth, count (count * 2^(depth-1) < 2^31), every host-side index -- sel_idx in [0, n_sel), row0 >= 0 and
 * row0 + 2^depth <= n_lut, coef in [0, N), and with sel_idx NULL count * depth <= n_sel -- are checked before anything is allocated or launched:
 * RTFHE_ERR_INVALID with a message naming the lookup.  The _dev forms take sel_idx / row0 / coef as device arrays and check them in the kernel:
 * a lookup with a bad index is skipped (its output is not a valid ciphertext) and the next rtfhe_sync returns RTFHE_ERR_INVALID, as for
 * rtfhe_pbs_batch_dev.  The FP64 mirror backend only: on either exact backend every tree call fails with RTFHE_ERR_INVALID (the context stays
 * usable).  A multi-device context runs the tree on its primary device.
 * Scratch: level k writes count * 2^(d-1-k) nodes; the levels alternate between two buffers that belong to the stream, each of
 *     4 * count * 2^(depth-1) * 2N  bytes      (none for depth 1)
 * grown outside stream captures only and kept until the context is destroyed; rtfhe_ctx_memory_bytes does not count them (as for LUT circuits).
 * Growing them synchronises the whole device (hipDeviceSynchronize: earlier trees of the stream may still read the old pair), so a call that
 * needs a larger pair than the stream has -- the first call on a stream, or a larger count * 2^(depth-1) -- stalls every stream of the process
 * once, also in the otherwise asynchronous _dev forms; run the largest shape once up front to keep later calls asynchronous.
 * Inside a caller's stream capture the rule of rtfhe_pbs_many_batch_dev applies: an eager call of the same entry point with at least this
 * count * 2^(depth-1) (and, for the extract form, at least this count) must have run on that stream first, else RTFHE_ERR_STATE. */
typedef struct rtfhe_trgsw rtfhe_trgsw;
int rtfhe_trgsw_create(rtfhe_ctx *ctx, const uint32_t *trgsw /* [n_sel][2][2l][N] */, int32_t n_sel, rtfhe_trgsw **out);
void rtfhe_trgsw_destroy(rtfhe_trgsw *sel);
int rtfhe_cmux_tree_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *sel_idx /* [count][depth] or NULL */, int32_t depth,
                          const rtfhe_lut *lut, const int32_t *row0 /* [count] or NULL */, uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_cmux_tree_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_sel_idx /* int32[count][depth] or NULL */, int32_t depth,
                              const rtfhe_lut *lut, const void *d_row0 /* int32[count] or NULL */, void *d_out /* [count][2][N] */, size_t count,
                              void *stream);
int rtfhe_cmux_tree_extract_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *sel_idx /* [count][depth] or NULL */, int32_t depth,
                                  const rtfhe_lut *lut, const int32_t *row0 /* [count] or NULL */, const int32_t *coef /* [count] or NULL */,
                                  uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_cmux_tree_extract_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_sel_idx /* int32[count][depth] or NULL */, int32_t depth,
                                      const rtfhe_lut *lut, const void *d_row0 /* int32[count] or NULL */, const void *d_coef /* int32[count] or NULL */,
                                      void *d_out /* [count][n+1] */, size_t count, void *stream);
/* ---- TRGSW blind rotation: a TRLWE rotated by encrypted address bits (horizontal packing, the other half of TFHE's leveled table lookup) ----
 * Lookup g of a batch takes a TRLWE trlwe[g], u32[2][N] (b then a) -- an rtfhe_cmux_tree_batch result, a row of an encrypted table, or a
 * trivial (tv, 0) --, a depth d = `depth` (1 .. 16, the same for the whole batch), selector indices sel_idx[g][0 .. d) into an rtfhe_trgsw
 * set (NULL: lookup g uses selectors g * depth + k, as in the tree) and exponents rot[0 .. d), ONE host array shared by the whole batch, each in
 * [0, 2N).  It computes
 *
 *     acc_0     = trlwe[g]
 *     acc_{k+1} = cmux(S_k, X^{rot[k]} * acc_k, acc_k) = cross(S_k, X^{rot[k]} * acc_k - acc_k) + acc_k,   S_k = selector sel_idx[g][k]
 *     result    = acc_d
 *
 * X^r * p is the negacyclic rotation of the bootstrap (utils/src/math.rs:85-132) applied to both polynomials; every step is one step of
 * TFHE::blind_rotate (hom_nand/src/tfhe.rs:103-110) with the key entry replaced by S_k and abar_i by rot[k]; cross is what
 * rtfhe_external_product_batch computes.  rot NULL: rot[k] = 2N - 2^k, i.e. X^{-2^k}, which requires depth <= log2 N + 1: with address bit k
 * in S_k the result is X^{-addr} * trlwe[g], whose coefficient 0 is coefficient addr of the row.  A CMUX tree of depth d and this rotation
 * look up a table of 2^d * N entries under a fully encrypted address in (2^d - 1) + log2 N CMUXes, without a bootstrapping key.
 *   rtfhe_trgsw_rotate_batch[_dev]          out[g] = the result, u32[2][N].  rot is a host array in both forms: it is copied into the
 *                                           kernel's arguments when the call is enqueued (a stream capture bakes it in).  d_out may be exactly
 *                                           d_trlwe (every lookup reads its whole row before it stores); no other overlap is allowed.  The
 *                                           _dev form allocates nothing: it may sit in a caller's stream capture without a prior eager call.
 *   rtfhe_trgsw_rotate_extract_batch[_dev]  out[g] = identity_key_switch(sample_extract_index(result, 0)), u32[n+1], through the route of
 *                                           rtfhe_cmux_tree_extract_batch (the stream's lvl1 sample buffer, then the key switch as one i8
 *                                           contraction, or one wave per sample under RTFHE_KS_MM_MIN=0).  Needs the key-switching key
 *                                           (RTFHE_ERR_STATE otherwise), not the bootstrapping key.  Inside a caller's stream capture an eager
 *                                           call of this entry point with at least this count must have run on the stream first, else
 *                                           RTFHE_ERR_STATE.
 * Checks before anything is launched: the handles, depth, count (count * depth < 2^31), every rot[k] in [0, 2N), the depth limit of rot NULL,
 * null in / out pointers, host sel_idx in [0, n_sel), and with sel_idx NULL count * depth <= n_sel: RTFHE_ERR_INVALID with a message naming the
 * lookup or the step.  The _dev forms check d_sel_idx in the kernel, all d indices of a lookup before its row is touched: a lookup with a bad
 * index is skipped whole, its output row keeps the bytes it had, and the next rtfhe_sync returns RTFHE_ERR_INVALID once, as for
 * rtfhe_cmux_tree_batch_dev.  The FP64 mirror backend only: on either exact backend every call fails with RTFHE_ERR_INVALID (the context
 * stays usable).  A multi-device context runs the rotation on its primary device. */
int rtfhe_trgsw_rotate_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *sel_idx /* [count][depth] or NULL */, int32_t depth,
                             const int32_t *rot /* [depth] or NULL */, const uint32_t *trlwe /* [count][2][N] */, uint32_t *out /* [count][2][N] */,
                             size_t count);
int rtfhe_trgsw_rotate_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_sel_idx /* int32[count][depth] or NULL */, int32_t depth,
                                 const int32_t *rot /* HOST [depth] or NULL */, const void *d_trlwe /* [count][2][N] */,
                                 void *d_out /* [count][2][N], may be d_trlwe */, size_t count, void *stream);
int rtfhe_trgsw_rotate_extract_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *sel_idx /* [count][depth] or NULL */, int32_t depth,
                                     const int32_t *rot /* [depth] or NULL */, const uint32_t *trlwe /* [count][2][N] */,
                                     uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_trgsw_rotate_extract_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_sel_idx /* int32[count][depth] or NULL */,
                                         int32_t depth, const int32_t *rot /* HOST [depth] or NULL */, const void *d_trlwe /* [count][2][N] */,
                                         void *d_out /* [count][n+1] */, size_t count, void *stream);
/* ---- CMUX netlists: decision diagrams over TRGSW-encrypted inputs, recorded once and replayed as one submission ----
 * The tree and the rotation above are the two degenerate shapes of one node,
 *   node = cmux(S_var, X^rot * hi, lo),
 * the fully expanded one and the single chain.  A CMUX netlist is any shape between: an arbitrary function of TRGSW-encrypted bits through
 * its reduced decision diagram, equal sub-diagrams computed once, several outputs from one diagram.
 *
 * A netlist has n_vars input variables and n_nodes nodes in topological order; every node value is a TRLWE u32[2][N] (b then a).  Node i
 * carries var[i] in [0, n_vars), the references hi[i] and lo[i], and rot[i] in [0, 2N) (rot NULL: all zero).  A reference r >= 0 is node r
 * and must satisfy r < i; a reference r < 0 is table row row0[g] + (-1 - r) of `lut`, plain or encrypted (a plain row tv is the trivial TRLWE
 * (tv, 0)).  For replica g of a batch of `count`:
 *   S        = selector d_sel_idx[g][var[i]]          (d_sel_idx NULL: g * n_vars + var[i])
 *   value_i  = cmux(S, X^rot[i] * value(hi[i]), value(lo[i])) = cross(S, X^rot[i] * hi - lo) + lo     (wrapping on every word)
 * with X^r the bootstrap's negacyclic rotation (rotated_coef, utils/src/math.rs:85-132), cmux TRGSWRepF::cmux (hom_nand/src/trgsw.rs:319-321)
 * and cross what rtfhe_external_product_batch computes.  With rot = 0 and a full binary shape this is rtfhe_cmux_tree_batch; with hi = lo =
 * the previous node it is one step of rtfhe_trgsw_rotate_batch.
 *
 * out_ref[0 .. n_out) names nodes only (a table row is refused).  Two forms, chosen at creation: out_coef NULL gives the TRLWE form,
 * d_out[count][n_out][2][N]; with out_coef given, d_out[count][n_out][n+1] = identity_key_switch(sample_extract_index(node, out_coef[o]))
 * through the tree's extract route (the batch key switch many-LUT uses, or under RTFHE_KS_MM_MIN=0 the wave-per-sample one); that form needs
 * the key-switching key only.
 *
 * rtfhe_cmux_circuit_create checks, before anything is allocated: the handles; n_nodes, n_vars, n_out, count >= 1; every var, every reference
 * (the topological order; the row range against the table when d_row0 is NULL), every rot and every out_coef (< N); with d_sel_idx NULL
 * count * n_vars <= n_sel; that the node buffer's byte count fits size_t.  A failure is RTFHE_ERR_INVALID and the message names the node or
 * output.  It then levelises the netlist -- level(i) = 1 + the largest level of its node children, 0 for a node with only leaf children --,
 * uploads the description, allocates what the circuit owns (the node buffer [count][n_nodes][2][N]: no slot is reused, it is
 * count * n_nodes * 8N bytes; its own copy of the table rows, so `lut` may be destroyed afterwards; one flag per replica; in the extract
 * form the sample buffer) and records ONE linear HIP graph: the check kernel, one launch per level, the output kernel, and in the extract form
 * the key switch.  The handle is an ordinary rtfhe_circuit: rtfhe_circuit_launch replays it on any stream (asynchronous, nothing is
 * allocated), rtfhe_circuit_destroy frees it, and a context destroyed first is rtfhe_circuit_create's case.  Two replays of one circuit must
 * not overlap (they share the node buffer).
 *
 * d_sel_idx, d_row0 and d_out belong to the caller, stay in place while the circuit exists and are read or written at replay.  The circuit
 * reads the selector set's spectra in place -- they are its inputs: rtfhe_trgsw_update rewrites selectors [first, first + n) of a live set
 * with rtfhe_trgsw_create's conversion (synchronous; it waits for the device first), and the next replay computes on the new ciphertexts.
 * Destroying the set marks the circuits recorded on it: their rtfhe_circuit_launch then fails with RTFHE_ERR_STATE.
 *
 * The device-resident indices are checked at every replay by the first kernel, all n_vars selector indices of a replica and its row0 against
 * the smallest and largest leaf the netlist names.  A bad replica is skipped whole: nothing is read or written through its indices, its node
 * slots are not written, its TRLWE output rows keep their bytes, its extract-form rows are all zero (no valid ciphertexts), and the next
 * rtfhe_sync returns RTFHE_ERR_INVALID once, as for rtfhe_cmux_tree_batch_dev.  The FP64 mirror backend only; a multi-device context runs
 * the circuit on its primary device. */
int rtfhe_cmux_circuit_create(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const rtfhe_lut *lut, const int32_t *var /* [n_nodes] */,
                              const int32_t *hi /* [n_nodes] */, const int32_t *lo /* [n_nodes] */, const int32_t *rot /* [n_nodes] or NULL */,
                              int32_t n_nodes, int32_t n_vars, const int32_t *out_ref /* [n_out] */,
                              const int32_t *out_coef /* [n_out], or NULL: TRLWE form */, int32_t n_out,
                              const void *d_sel_idx /* int32[count][n_vars] or NULL */, const void *d_row0 /* int32[count] or NULL */,
                              void *d_out, size_t count, rtfhe_circuit **out);
int rtfhe_trgsw_update(rtfhe_trgsw *sel, const uint32_t *trgsw /* [n][2][2l][N] */, int32_t first, int32_t n);
/* ---- packing key switch: lvl0 ciphertexts into TRLWE rows (bootstrapped mode -> leveled mode) ----
 * Packing key.  pk is u32[n][t][base-1][2][N], with t = ks_t and base = 2^ks_basebit.  Row (i, j, d) is a TRLWE in the project's layout (b(X),
 * then a(X)) under key1.  It encrypts the constant polynomial (d+1) · key0[i] · 2^(-ks_basebit·(j+1)) with alpha = 2^-25.  The message word is
 * formed exactly as the key-switching key's: torus_from_f32((float)key0[i] * pw * (float)(d+1)).  rtfhe_packing_keygen draws it from the OS
 * CSPRNG, rtfhe_packing_keygen_deterministic (TEST ONLY) from a seed; both reject non-binary keys.
 * The rows' noise MUST BE ZERO-MEAN: about 3/4 · n · t · P · rep row coefficients (4 · 10^6 at n = 635, P · rep = 1024) add into every packed
 * coefficient, so a common mean grows linearly where the noise itself grows with the square root.  The f32 sampler of the other keys
 * (Normal f32 through torus_from_f32, as the reference's) has a mean of about +10 · 2^-32 at alpha = 2^-25: rows drawn with it give a packed
 * error of 9 · 10^-3 of the torus where zero-mean rows give 4 · 10^-4.  The two generators here draw the noise in double precision, rounded to
 * the nearest torus word; a key made elsewhere must do the same.
 *
 * Key switch of one sample.  Take a lvl0 sample c = (a_0 … a_{n-1}, b).
 *   - Let ROUND = 2^(32 - t·ks_basebit - 1).
 *   - Let d_{i,j} = ((a_i + ROUND) >> (32 - (j+1)·ks_basebit)) & (base - 1).  These are the digits of identity_key_switch.
 *   - S(c) is the TRLWE with
 *       S.b[k] = [k = 0]·b - Σ_{i,j : d_{i,j} ≠ 0} pk[i][j][d_{i,j}-1].b[k]
 *       S.a[k] =           - Σ_{i,j : d_{i,j} ≠ 0} pk[i][j][d_{i,j}-1].a[k]
 *   - Every word wraps mod 2^32.
 *
 * Packing.  Output g of a batch is out[g] = Σ_{p<P} X^{pos[p]} · (1 + X + … + X^{rep-1}) · S(c[g][p]) mod X^N + 1, on both halves.  Word for word:
 *   - out[g][h][c] = Σ_p Σ_{k<rep} ± S_p[h][u mod N], where u = (c - pos[p] - k) mod 2N.
 *   - The sign is + if u < N and - otherwise.
 *   - u32 addition is associative and commutative.  Any summation order gives the same words.
 *
 * Parameters.
 *   - pos is a host array int32[P], shared by the batch (copied into the launch's arguments when the call is enqueued: a stream capture bakes
 *     it in).  pos NULL means pos[p] = p·rep.
 *   - The calls check 1 ≤ P ≤ N, 1 ≤ rep ≤ N and pos[p] ∈ [0, 2N) (also for the positions pos NULL stands for).  A failed check returns
 *     RTFHE_ERR_INVALID before anything is launched.
 *   - Overlapping runs are allowed; they add.
 *   - The key type needs ks_t = 8 and ks_basebit = 2, the one instantiation the batch key switch has.  Anything else returns RTFHE_ERR_INVALID
 *     at key generation and at key creation.
 *
 * Backends and devices.  Nothing here multiplies polynomials.  The calls work on every rtfhe_backend and never read the bootstrapping key or
 * the key-switching key.  On an rtfhe_ctx_create_multi context they run on the primary device only.
 *
 * Table layout.  With rep = B = N / 2^p and pos[e] = (e·B - B/2) mod 2N, packing the 2^p ciphertexts of enc_out(f(e)) yields an encryption of
 * the test polynomial of f on p-bit messages (rustfhe_amd.pbs.lut_polynomial; rustfhe_amd.pbs.lut_pack_layout gives pos and rep).  Box e covers
 * [eB - B/2, eB + B/2), and entry 0's lower half-box lands on the top coefficients with the sign flipped.
 *
 * Key handle.  rtfhe_packing_key_create uploads the rows to the primary device, turns them into signed byte limbs in the operand order of the
 * i8 matrix pipe and frees the upload.  Device footprint of a handle: N · n16 · 256 bytes, n16 = n rounded up to a multiple of 16 (168 MB at
 * n = 635, N = 1024; creation also holds the 2N · 4 · n · t · (base-1) bytes of the upload, 125 MB, until it returns).  It is not counted by
 * rtfhe_ctx_memory_bytes, as for selector sets.  Lifetime as rtfhe_trgsw: normally destroyed before its context; if the context goes first,
 * the matrix is released with it, a later pack call with the handle fails with RTFHE_ERR_STATE and rtfhe_packing_key_destroy only frees the
 * handle.
 *
 * rtfhe_pack_batch takes host buffers and is synchronous.  rtfhe_pack_batch_dev is asynchronous and stream-ordered.  The key-switched samples
 * S[count·P][2N] live in a buffer of the context that belongs to `stream` (8N bytes per sample; not counted by rtfhe_ctx_memory_bytes), grown
 * outside stream captures only -- growing an existing one synchronises the device -- and kept until the context is destroyed.  Inside a
 * stream capture the call allocates nothing: an eager rtfhe_pack_batch_dev of at least count·P samples must have run on that stream first,
 * else RTFHE_ERR_STATE.  This is the rule of rtfhe_pbs_many_batch_dev.
 *
 * rtfhe_lut_update_dev rewrites rows first … first+n-1 of an ENCRYPTED table in place from device memory, a stream-ordered copy: a packed row
 * becomes a table row without a host round trip.  It returns RTFHE_ERR_INVALID for a plain table, for a range outside the table and on a
 * multi-device context, and RTFHE_ERR_STATE after the context is gone.  PBS calls enqueued later on the same stream read the new rows.  LUT
 * circuits and CMUX netlists own a copy of their rows and are not affected. */
typedef struct rtfhe_packing_key rtfhe_packing_key;
int rtfhe_packing_keygen(const rtfhe_params *p, const int32_t *key0, const int32_t *key1, uint32_t *pk /* [n][t][base-1][2][N] */);
/* TEST ONLY -- NOT SECURE (see rtfhe_keygen_deterministic) */
int rtfhe_packing_keygen_deterministic(const rtfhe_params *p, uint64_t seed, const int32_t *key0, const int32_t *key1, uint32_t *pk);
int rtfhe_packing_key_create(rtfhe_ctx *ctx, const uint32_t *pk /* [n][t][base-1][2][N] */, rtfhe_packing_key **out);
void rtfhe_packing_key_destroy(rtfhe_packing_key *pk);
int rtfhe_pack_batch(rtfhe_ctx *ctx, const rtfhe_packing_key *pk, const uint32_t *tlwe /* [count][P][n+1] */, int32_t P,
                     const int32_t *pos /* [P] or NULL */, int32_t rep, uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_pack_batch_dev(rtfhe_ctx *ctx, const rtfhe_packing_key *pk, const void *d_tlwe /* [count][P][n+1] */, int32_t P,
                         const int32_t *pos /* HOST [P] or NULL */, int32_t rep, void *d_out /* [count][2][N] */, size_t count, void *stream);
int rtfhe_lut_update_dev(rtfhe_lut *lut, const void *d_trlwe /* [n][2][N] */, int32_t first, int32_t n, void *stream);
/* ---- CMUX demultiplexer tree: a TRLWE written to leaf `addr` of 2^d, addr given as TRGSW-encrypted bits (the tree above run backwards) ----
 * Lookup g of a batch takes a TRLWE x[g], u32[2][N] (b then a) -- a plain polynomial tv is passed as the trivial (tv, 0) --, a depth
 * d = `depth` (1 .. 16, the same for the whole batch) and selector indices sel_idx[g][0 .. d) into an rtfhe_trgsw set: entry k is address bit k,
 * least significant first; NULL: lookup g uses selectors g * depth + k.  These are the tree's conventions.  It computes
 *
 *     level 0 node    x[g]
 *     level t = 0 .. d-1, 2^t nodes, selector k = demux_level_selector(d, t) = d - 1 - t, S_k = selector sel_idx[g][k]:
 *         child[2j+1] = cross(S_k, node_j)
 *         child[2j]   = node_j - child[2j+1]
 *     result          the 2^d children of level d - 1: leaf i is out[g][i]
 *
 * The subtraction wraps on every word of both polynomials; cross is Cross for TRGSWRepF (hom_nand/src/trgsw.rs:264-306), i.e. exactly what
 * rtfhe_external_product_batch computes for a key entry, and cross(S, x) = cmux(S, x, 0).  Leaf sum_k bit_k 2^k is a TRLWE of x[g]'s message
 * and every other leaf a TRLWE of 0, each having passed d external products: 2^d - 1 products per lookup.  Level t splits on the selector
 * the tree's level d - 1 - t joins on (the tree's level k uses selector k), so the demultiplexer is the tree's inverse: rtfhe_cmux_tree_batch
 * over the 2^d leaves (as an encrypted table) with the same selectors returns a TRLWE of x[g]'s message, and with any address bit flipped a
 * TRLWE of 0.
 *   rtfhe_demux_tree_batch[_dev]   out[g][i] = leaf i, u32[count][2^d][2][N]: rows in the format of rtfhe_lut_create_encrypted and of
 *                                  rtfhe_lut_accumulate_dev
 * Checks before anything is allocated or launched: the handles, depth, count (count * 2^(depth-1) < 2^31), null x / out, host sel_idx in
 * [0, n_sel), with sel_idx NULL count * depth <= n_sel, and in the _dev form d_out overlapping d_x: RTFHE_ERR_INVALID with a message naming
 * the lookup.  The _dev form checks d_sel_idx in the kernel, all d indices of a lookup at every level: a lookup with a bad index is skipped
 * whole, its 2^d output rows keep the bytes they had, and the next rtfhe_sync returns RTFHE_ERR_INVALID once, as for
 * rtfhe_cmux_tree_batch_dev.  Only the selector set is needed, no key of the context.  The FP64 mirror backend only: on either exact backend
 * every call fails with RTFHE_ERR_INVALID (the context stays usable).  A multi-device context runs it on its primary device.  The call reads
 * rtfhe_set_leveled_decomposition when it is made, as the tree does.
 * Scratch: level t < d - 1 writes count * 2^(t+1) nodes; the levels alternate between the two buffers of the stream that the CMUX tree uses,
 * each of 4 * count * 2^(depth-1) * 2N bytes (none for depth 1), under the tree's rules: grown outside stream captures only (growing
 * synchronises the device), kept until the context is destroyed, and inside a caller's stream capture an eager call with at least this
 * count * 2^(depth-1) must have run on that stream first, else RTFHE_ERR_STATE (depth 1 needs none).
 *
 * rtfhe_lut_accumulate_dev adds TRLWEs into rows first .. first+n-1 of an ENCRYPTED table in place, stream-ordered:
 *     row[first + r] += sum_{g < count} d_trlwe[g][r]      for r in [0, n), wrapping on every word of both polynomials
 * Wrapping addition is exact in any order, so the result is deterministic.  With d_trlwe the leaves of `count` demultiplexed writes
 * (n = 2^d) this is an oblivious scatter-add: the server adds x[g] into the row each encrypted address names without learning it.  It follows
 * rtfhe_lut_update_dev's rules: RTFHE_ERR_INVALID for a plain table, for first < 0 or first + n > n_lut, for count < 1 and on a multi-device
 * context, RTFHE_ERR_STATE after the context is gone; calls enqueued later on the same stream read the new rows; LUT circuits and CMUX netlists
 * own a copy of their rows and are not affected.  d_trlwe must not overlap the table.
 *
 * rtfhe_lut_read_dev is rtfhe_lut_update_dev the other way: a stream-ordered copy of rows first .. first+n-1 of an ENCRYPTED table into
 * device memory u32[n][2][N], under the same rules and refusals.  A table the server has written is state only the server holds; this is
 * how its rows leave for whoever holds the key (the histogram's counts), and how the accumulation is checked word for word. */
int rtfhe_demux_tree_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *sel_idx /* [count][depth] or NULL */, int32_t depth,
                           const uint32_t *x /* [count][2][N] */, uint32_t *out /* [count][2^depth][2][N] */, size_t count);
int rtfhe_demux_tree_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_sel_idx /* int32[count][depth] or NULL */, int32_t depth,
                               const void *d_x /* [count][2][N] */, void *d_out /* [count][2^depth][2][N] */, size_t count, void *stream);
int rtfhe_lut_accumulate_dev(rtfhe_lut *lut, const void *d_trlwe /* [count][n][2][N] */, int32_t first, int32_t n, size_t count, void *stream);
int rtfhe_lut_read_dev(const rtfhe_lut *lut, void *d_out /* [n][2][N] */, int32_t first, int32_t n, void *stream);
/* ---- TRLWE sample extraction: coefficients of TRLWE rows as lvl0 ciphertexts (leveled mode -> bootstrapped mode) ----
 * The inverse of the packing key switch.  It takes TRLWEs that already exist -- a row read with rtfhe_lut_read_dev, a packed row, a
 * demultiplexer leaf, a row a client sent -- and returns ciphertexts of chosen coefficients, which the bootstrapped entry points (gates,
 * PBS, LUT circuits) take as they are.
 *
 * Sample (g, p).  For the TRLWE x[g], u32[2][N] (b then a), and the coefficient list coef[0 .. P), sample (g, p) is
 * e = sample_extract_index(x[g], coef[p]), the reference's TRLWERep::sample_extract_index (hom_nand/src/trlwe.rs:110-121).  Word for word,
 * with j = coef[p]:
 *   - e.a[c] = x.a[j - c]            for c <= j;
 *   - e.a[c] = 0 - x.a[N + j - c]    for c > j, wrapping mod 2^32;
 *   - e.b    = x.b[j].
 * Its layout is that of rtfhe_key_switch_batch's input, the lvl1 TLWE: a'[0 .. N), then b'.
 *   rtfhe_trlwe_extract_lvl1_batch[_dev]   out[g][p] = e, u32[N+1].  Needs no key at all: a context with nothing loaded runs it.
 *   rtfhe_trlwe_extract_batch[_dev]        out[g][p] = identity_key_switch(e), u32[n+1], by the route every extract form takes (the stream's
 *                                          lvl1 sample buffer, then the key switch as one i8 contraction, or one wave per sample under
 *                                          RTFHE_KS_MM_MIN=0).  Needs the key-switching key (RTFHE_ERR_STATE otherwise), not the bootstrapping key.
 *
 * Parameters.
 *   - coef is a host array int32[P], shared by the whole batch like rtfhe_pack_batch's pos (copied into the launches' arguments when the call is
 *     enqueued: a stream capture bakes it in).  Duplicates are allowed.
 *   - coef NULL means coef[p] = p * stride: rtfhe_trlwe_extract_batch(P, NULL, rep) reads back what rtfhe_pack_batch(P, NULL, rep) wrote.
 *     stride is ignored when coef is given.
 *   - Checked before anything is allocated or launched, RTFHE_ERR_INVALID with a message naming the sample: 1 <= P <= N; coef[p] in [0, N);
 *     with coef NULL stride >= 1 and (P - 1) * stride < N; count * P < 2^31; no null buffer; out does not overlap trlwe.
 *   - count == 0 returns 0.
 *
 * Backends and devices.  No polynomial is multiplied: both forms run on every rtfhe_backend, as packing does, and on an
 * rtfhe_ctx_create_multi context on the primary device.
 *
 * Scratch and captures.  The lvl1 form allocates nothing and may sit in a caller's stream capture without a prior eager call.  The samples of
 * the lvl0 form go through the stream's lvl1 sample buffer, 4 (N + 1) bytes per sample, under rtfhe_pbs_many_batch_dev's rule: grown outside
 * stream captures only (growing an existing one synchronises the device) and kept until the context is destroyed; inside a caller's capture
 * an eager rtfhe_trlwe_extract_batch_dev of at least count * P samples must have run on that stream first, else RTFHE_ERR_STATE.
 * A call is ceil(P / 512) launches of the extract kernel plus, in the lvl0 form, the key switch. */
int rtfhe_trlwe_extract_batch(rtfhe_ctx *ctx, const uint32_t *trlwe /* [count][2][N] */, int32_t P, const int32_t *coef /* [P] or NULL */,
                              int32_t stride, uint32_t *out /* [count][P][n+1] */, size_t count);
int rtfhe_trlwe_extract_batch_dev(rtfhe_ctx *ctx, const void *d_trlwe /* [count][2][N] */, int32_t P, const int32_t *coef /* HOST [P] or NULL */,
                                  int32_t stride, void *d_out /* [count][P][n+1] */, size_t count, void *stream);
int rtfhe_trlwe_extract_lvl1_batch(rtfhe_ctx *ctx, const uint32_t *trlwe /* [count][2][N] */, int32_t P, const int32_t *coef /* [P] or NULL */,
                                   int32_t stride, uint32_t *out /* [count][P][N+1] */, size_t count);
int rtfhe_trlwe_extract_lvl1_batch_dev(rtfhe_ctx *ctx, const void *d_trlwe /* [count][2][N] */, int32_t P, const int32_t *coef /* HOST [P] or NULL */,
                                       int32_t stride, void *d_out /* [count][P][N+1] */, size_t count, void *stream);
/* ---- exact TRLWE x plain-polynomial products: ciphertext x plaintext, the linear layer of the leveled mode ----
 * A plain set holds n_w integer polynomials w[e], int32[N], transformed once at creation.  A call computes, for g in [0, count):
 *
 *   out[g] = (accumulate ? out[g] : 0) + sum_{k < K} w[w_idx[g][k]] * x[x_idx[g][k]]        in Z_{2^32}[X]/(X^N + 1)
 *
 * on both polynomials of the TRLWE row (u32[2][N], b then a), every word wrapping mod 2^32.  The result is EXACT: no rounding anywhere, so it
 * does not depend on the backend and adds no noise of its own.  The output noise is the input's scaled by the weights: variance
 * sum_k ||w_k||_2^2 sigma_x^2, mean ||w||_1 times the input's mean.
 *
 * Parameters.
 *   - x is an array of n_x rows.  w_idx NULL means entry k for every g (it needs n_w >= K: the same weights for every sample); x_idx NULL means
 *     row g * K + k (it needs n_x >= count * K).  Duplicates are allowed.
 *   - accumulate = 1 adds into out: a bias (the caller initialises out with the trivial TRLWE: bias in b, 0 in a), more than K terms, residual
 *     adds.  accumulate = 0 overwrites out.
 *   - Exactness domain.  Creation records wmax = max_e ||w[e]||_1.  A call is accepted iff K * wmax <= 192 * N, 1 <= K <= 8: the total l1 norm
 *     6 * 32 * N of the small operand at which the split-FFT exact backend's products are proven exact (worst-case transform error 2^-8.25 at
 *     N = 1024, 2^-6.62 at N = 2048, against the 1/2 of the rounding), here with the roles reversed: the weights are transformed once, the
 *     ciphertext is split into signed 16-bit halves when it is read.
 *   - Checked on the host before anything is allocated or launched, RTFHE_ERR_INVALID with a message naming the sample: handles and buffers
 *     non-null; K; K * wmax; n_w, n_x >= 1; count * K < 2^31; every host index in range and the NULL-index rules above; out overlaps no part of x
 *     (in-place products are not supported).  count == 0 returns 0.
 *   - The _dev form takes the index arrays on the device and checks them in the kernel: a sample with a bad index is skipped, its output row
 *     untouched, and the next rtfhe_sync returns RTFHE_ERR_INVALID once, as for rtfhe_cmux_tree_batch_dev.
 *
 * Keys, backends and devices.  It needs no key at all and runs on every rtfhe_backend; on an rtfhe_ctx_create_multi context on the primary
 * device.  Lifetime is rtfhe_trgsw's: the spectra (8 N bytes per polynomial) live on the primary device and go with the context if it is
 * destroyed first; a call then returns RTFHE_ERR_STATE and rtfhe_plain_destroy only frees the handle.
 *
 * Scratch and captures.  The _dev form allocates nothing and is ONE launch: it may sit in a caller's stream capture first thing on a fresh
 * stream (rtfhe_plain_create is synchronous and builds what the kernel needs). */
typedef struct rtfhe_plain rtfhe_plain;
int rtfhe_plain_create(rtfhe_ctx *ctx, const int32_t *w /* [n_w][N] */, int32_t n_w, rtfhe_plain **out);
void rtfhe_plain_destroy(rtfhe_plain *w);
int rtfhe_trlwe_mul_plain_batch(rtfhe_ctx *ctx, const rtfhe_plain *w, const int32_t *w_idx /* [count][K] or NULL */, const uint32_t *x /* [n_x][2][N] */,
                                int32_t n_x, const int32_t *x_idx /* [count][K] or NULL */, int32_t K, int32_t accumulate,
                                uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_trlwe_mul_plain_batch_dev(rtfhe_ctx *ctx, const rtfhe_plain *w, const void *d_w_idx /* [count][K] or NULL */, const void *d_x /* [n_x][2][N] */,
                                    int32_t n_x, const void *d_x_idx /* [count][K] or NULL */, int32_t K, int32_t accumulate,
                                    void *d_out /* [count][2][N] */, size_t count, void *stream);
/* ---- TRLWE x TRGSW multiply-accumulate: ciphertext x ciphertext, the linear layer with encrypted weights ----
 * TRGSWRepF::cross (hom_nand/src/trgsw.rs:264-306) on the samples of a selector set (rtfhe_trgsw_create; e.g. encryptions of small-integer
 * polynomials from rtfhe_trgsw_encrypt_polys), with its fold-add carried over K terms.  For g in [0, count), on both polynomials of the row:
 *
 *   sum_c  = 0.0;  for k = 0 .. K-1, for h = b, a, for j = 0 .. l-1:
 *                sum_c = sum_c + hadamard(S[s_idx[g][k]].row(c, h, j), ifft_i32(digit_j(x[x_idx[g][k]].poly_h)))          c = 0, 1
 *   out[g].poly_c = (accumulate ? out[g].poly_c : 0) + fft_u32(sum_c)                                    wrapping u32 add
 *
 * i.e. out[g] = (accumulate ? out[g] : 0) + sum_k S_k (.) x_k with ONE pair of inverse transforms and one truncation for the whole sum.  The
 * blocks are those of rtfhe_external_product_batch on the FP64 mirror backend: the digits of the leveled decomposition in force when the call
 * is made (rtfhe_set_leveled_decomposition), the reference's forward transform, the unfused multiply-add, the inverse transform with
 * truncation toward zero -- exact over the sum's whole range, K * 2l * N * (Bg/2) * 2^31 < 2^53.  K = 1 without accumulate gives the words of
 * rtfhe_external_product_batch on the same TRGSW sample and row.
 *
 * With S_k encrypting mu_k(X) the result decrypts to sum_k mu_k * phase(x_k) plus, per term, the selector rows' noise (which does not scale
 * with mu), the decomposition's rounding through mu_k, and x_k's own noise through mu_k.  One-hot selectors make it a K-way row select.
 *
 * Parameters.
 *   - 1 <= K <= 8.  x is an array of n_x rows.  s_idx NULL means selector g * K + k (it needs n_sel >= count * K); x_idx NULL means row
 *     g * K + k (it needs n_x >= count * K).  Duplicates are allowed.
 *   - accumulate = 1 adds into out (a bias as the trivial TRLWE, more than K terms); accumulate = 0 overwrites out.
 *   - Checked on the host before anything is allocated or launched, RTFHE_ERR_INVALID with a message naming the sample: handles and buffers
 *     non-null; K; n_x >= 1; count * K < 2^31; every host index in range and the NULL-index rules above; out overlaps no part of x (in-place
 *     products are not supported).  count == 0 returns 0.
 *   - The _dev form takes the index arrays on the device and checks them in the kernel: a sample with a bad index is skipped, its output row
 *     untouched, and the next rtfhe_sync returns RTFHE_ERR_INVALID once, as for rtfhe_cmux_tree_batch_dev.
 *
 * Keys, backends and devices.  It needs no key of the context.  FP64 mirror backend only: on an exact backend the call returns
 * RTFHE_ERR_INVALID and the context stays usable, as for every other call over a selector set.  On an rtfhe_ctx_create_multi context it runs
 * on the primary device.  A destroyed context gives RTFHE_ERR_STATE.
 *
 * Scratch and captures.  The _dev form allocates nothing and is ONE launch, counted by rtfhe_timer_end: it may sit in a caller's stream
 * capture first thing on a fresh stream (rtfhe_trgsw_create grants the kernel what it needs). */
int rtfhe_trlwe_mul_trgsw_batch(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const int32_t *s_idx /* [count][K] or NULL */, const uint32_t *x /* [n_x][2][N] */,
                                int32_t n_x, const int32_t *x_idx /* [count][K] or NULL */, int32_t K, int accumulate,
                                uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_trlwe_mul_trgsw_batch_dev(rtfhe_ctx *ctx, const rtfhe_trgsw *sel, const void *d_s_idx /* [count][K] or NULL */, const void *d_x /* [n_x][2][N] */,
                                    int32_t n_x, const void *d_x_idx /* [count][K] or NULL */, int32_t K, int accumulate,
                                    void *d_out /* [count][2][N] */, size_t count, void *stream);
/* ---- TRLWE key switching: automorphisms X -> X^t and re-keying ----
 * The automorphism sigma_t : X -> X^t (t odd) permutes a polynomial's coefficients with signs: coefficient j goes to j t mod 2N and is negated
 * past N.  sigma_t(ct) decrypts under sigma_t(s); a TRLWE -> TRLWE key switch brings it back under s -- or, with t = 1 and two different keys,
 * moves a row from one key to another.  Both are one primitive.
 *
 * A SWITCHING KEY for the exponents t[0 .. n_t) is u32[n_t][l][2][N]: row (e, j) is a TRLWE (b then a) under key_to whose phase is
 * -sigma_{t[e]}(key_from) * 2^(32 - (j+1) bgbit), with noise alpha = 2^-25 (rtfhe_trlwe_ksk_keygen below).  key_from == key_to gives
 * automorphism keys; t = 1 with two different keys gives a re-keying key; both at once is allowed.
 *
 * One STEP with entry e on a row x = (b, a), t = t[e]:
 *
 *   a' = sigma_t(a),  b' = sigma_t(b)                    sigma_t(p)[j t mod 2N mod N] = +-p[j], negated when j t mod 2N >= N; wrapping
 *   sum_c = 0.0;  for j = 0 .. l-1:  sum_c = sum_c + hadamard(K[e].row(c, j), ifft_i32(digit_j(a')))          c = 0 (b), 1 (a)
 *   y = (b' + fft_u32(sum_0),  fft_u32(sum_1))
 *   x <- y   (replace)      or      x <- x + y   (add; wrapping)
 *
 * The blocks are those of rtfhe_external_product_batch on the FP64 mirror backend: the digits of the leveled decomposition in force when the
 * call is made (rtfhe_set_leveled_decomposition), the reference's transforms, the unfused multiply-add with the rows in order j = 0 .. l-1, one
 * inverse transform per polynomial with truncation toward zero -- exact, a single product stays below l * N * (Bg/2) * 2^31 < 2^49.  Both
 * decompositions give the digits 0 for the word 0, so a step equals, word for word,
 *
 *   (sigma_t b, 0) + rtfhe_external_product_batch(T, (b := sigma_t a, a := 0))
 *
 * with T the TRGSW whose rows (c, h = b, j) are K[e]'s rows and whose rows (c, h = a, j) are zero.  If x decrypts to mu under key_from, a replace
 * step decrypts to sigma_t(mu) under key_to, plus one gadget level of noise.  sigma_{N / 2^i + 1} added to the identity is the
 * partial trace: it keeps every 2^(i+1)-th coefficient, doubled, and cancels the others.
 *
 * A call runs a PROGRAM of 1 .. 16 steps on every row of a batch: entry[k] and add[k] (NULL: every step replaces) are HOST arrays in both forms,
 * shared by the batch and read before the call returns (they ride in the launch's arguments, as rot does for rtfhe_trgsw_rotate_batch).
 *
 * Parameters.
 *   - Checked on the host before anything is allocated or launched, RTFHE_ERR_INVALID with a message: handle, entry and buffers non-null;
 *     1 <= n_steps <= 16; every entry[k] in [0, n_t); every add[k] 0 or 1; count < 2^31; out is exactly x (in place) or shares no byte with it.
 *     count == 0 returns 0.  At creation: words and t non-null, 1 <= n_t <= 64, every t odd and in [1, 2N), no exponent twice.
 *
 * Keys, backends and devices.  It needs no key of the context.  FP64 mirror backend only: on an exact backend the call returns
 * RTFHE_ERR_INVALID and the context stays usable.  On an rtfhe_ctx_create_multi context it runs on the primary device.  Lifetime is
 * rtfhe_trgsw's: the spectra (8 N bytes per polynomial) live on the primary device and go with the context if it is destroyed first; a call
 * then returns RTFHE_ERR_STATE and rtfhe_trlwe_ksk_destroy only frees the handle.
 *
 * Scratch and captures.  The _dev form allocates nothing and is ONE launch, counted by rtfhe_timer_end: it may sit in a caller's stream
 * capture first thing on a fresh stream (rtfhe_trlwe_ksk_create is synchronous and grants the kernel what it needs). */
typedef struct rtfhe_trlwe_ksk rtfhe_trlwe_ksk;
int rtfhe_trlwe_ksk_create(rtfhe_ctx *ctx, const uint32_t *words /* [n_t][l][2][N] */, const int32_t *t /* [n_t] */, int32_t n_t, rtfhe_trlwe_ksk **out);
void rtfhe_trlwe_ksk_destroy(rtfhe_trlwe_ksk *key);
int rtfhe_trlwe_auto_batch(rtfhe_ctx *ctx, const rtfhe_trlwe_ksk *key, const int32_t *entry /* [n_steps] */, const int32_t *add /* [n_steps] or NULL */,
                           int32_t n_steps, const uint32_t *x /* [count][2][N] */, uint32_t *out /* [count][2][N], may be x */, size_t count);
int rtfhe_trlwe_auto_batch_dev(rtfhe_ctx *ctx, const rtfhe_trlwe_ksk *key, const int32_t *entry /* HOST [n_steps] */,
                               const int32_t *add /* HOST [n_steps] or NULL */, int32_t n_steps, const void *d_x /* [count][2][N] */,
                               void *d_out /* [count][2][N], may be d_x */, size_t count, void *stream);
/* ---- lvl0 dense layers: integer matrix x TLWE batch, the linear layer of the bootstrapped mode ----
 * A dense layer holds an integer matrix W, int32[O][I] with every entry in [-128, 127], as signed bytes in the matrix pipe's operand order,
 * built once at creation together with one correction word per output.  A call computes, for g in [0, count), o in [0, O), c = 0 .. n:
 *
 *   out[g][o][c] = (accumulate ? out[g][o][c] : 0) + [c == n] * bias[o] + sum_{i < I} W[o][i] * x[g][i][c]        mod 2^32
 *
 * on all n + 1 words of the lvl0 rows (mask words 0 .. n-1, then b): sample g's I input ciphertexts in, its O weighted sums out.  The result is
 * EXACT word for word: the ciphertext words are split into signed byte limbs, the products are summed in i32 on the i8 matrix pipe
 * (|sum| <= I * 2^14 <= 2^30) and recombined mod 2^32, so it equals the row-by-row wrapping sum, does not depend on the backend and adds no noise
 * of its own.  The output noise is the inputs' scaled by the weights: variance sum_i W[o][i]^2 sigma_i^2.  A bias is a torus word added to b
 * (word n) of every sample's output o.
 *
 * Parameters.
 *   - Limits: 1 <= O <= 65,536, 1 <= I <= 65,536, count * max(I, O) * (n + 1) < 2^31 words.  Rows are n + 1 words at 4-byte alignment; any n the
 *     context accepts works.  accumulate = 1 adds into out (residual sums, more than one matrix into one output), accumulate = 0 overwrites it.
 *   - Checked on the host before anything is allocated or launched, RTFHE_ERR_INVALID: at creation W and out non-null, O, I, every entry's range
 *     (the first offender is named); per call handle and buffers non-null, the limits above, out overlaps no part of x.  count == 0 returns 0.
 *   - bias is a HOST array in both forms and is read before the call returns (it rides in the launch's arguments).
 *
 * Keys, backends and devices.  It needs no key at all and runs on every rtfhe_backend; on an rtfhe_ctx_create_multi context on the primary
 * device.  Lifetime is rtfhe_trgsw's: the matrix (O x I bytes, padded to 16 x 64) lives on the primary device and goes with the context if
 * it is destroyed first; a call then returns RTFHE_ERR_STATE and rtfhe_dense_destroy only frees the handle.
 *
 * Scratch and captures.  The _dev form allocates nothing: it may sit in a caller's stream capture first thing on a fresh stream
 * (rtfhe_dense_create is synchronous and builds what the kernel needs).  Without a bias it is ONE kernel launch, counted by rtfhe_timer_end;
 * with a bias ceil(O / 512) launches (one for O <= 512; up to 128 at O = 65,536, each reading x again), back to back on the stream.  A
 * small launch (fewer than two workgroups per CU) shares I among workgroups whose parts meet as wrapping atomic adds; if any launch of a
 * call that does not accumulate does so, the whole output is cleared once, before the call's first launch, by a memset on the same stream
 * (no kernel). */
typedef struct rtfhe_dense rtfhe_dense;
int rtfhe_dense_create(rtfhe_ctx *ctx, const int32_t *W /* [O][I], every entry in [-128, 127] */, int32_t O, int32_t I, rtfhe_dense **out);
void rtfhe_dense_destroy(rtfhe_dense *w);
int rtfhe_tlwe_dense_batch(rtfhe_ctx *ctx, const rtfhe_dense *w, const uint32_t *x /* [count][I][n+1] */, const uint32_t *bias /* [O] or NULL */,
                           int32_t accumulate, uint32_t *out /* [count][O][n+1] */, size_t count);
int rtfhe_tlwe_dense_batch_dev(rtfhe_ctx *ctx, const rtfhe_dense *w, const void *d_x /* [count][I][n+1] */, const uint32_t *bias /* HOST [O] or NULL */,
                               int32_t accumulate, void *d_out /* [count][O][n+1] */, size_t count, void *stream);
/* waits for `stream`; also reports (once) a netlist gate skipped since the previous call */
int rtfhe_sync(rtfhe_ctx *ctx, void *stream);
/* device-side timing of the launches enqueued by the *_dev calls between begin and end (HIP events on
 * `stream`); end returns total milliseconds and the number of kernel launches */
int rtfhe_timer_begin(rtfhe_ctx *ctx, void *stream);
int rtfhe_timer_end(rtfhe_ctx *ctx, void *stream, double *ms, int64_t *launches);
/* the same, and of the total the device time spent in the batch key switches of the split path.  Every batch of at least
 * RTFHE_KS_MM_MIN gates (environment, default 1: every batch -- any size, netlist waves, N = 1024 and 2048, both backends) runs as two
 * launches: blind rotation + sample extract (which also zeroes the gates' output rows), then the key switch of the whole batch as one
 * exact i8 contraction (k_key_switch_mm).  RTFHE_KS_MM_MIN=0 keeps the key switch fused into the bootstrap kernel; so does a batch
 * enqueued inside a caller's own stream capture (the split path's scratch buffer belongs to the stream, not to the caller's graph) --
 * key_switch_ms is 0 when all were fused, and the launches of an rtfhe_circuit are never bracketed. */
int rtfhe_timer_end_detail(rtfhe_ctx *ctx, void *stream, double *ms, double *key_switch_ms, int64_t *launches);

/* ---- stage-level entry points (parity tests; same kernels' building blocks) ---- */
int rtfhe_blind_rotate_batch(rtfhe_ctx *ctx, const uint32_t *tlwe /* [count][n+1] */, int32_t steps,
                             uint32_t *acc /* [count][2][N] */, size_t count);
int rtfhe_external_product_batch(rtfhe_ctx *ctx, const int32_t *bk_index /* [count] */,
                                 const uint32_t *trlwe /* [count][2][N] */, uint32_t *out, size_t count);
int rtfhe_key_switch_batch(rtfhe_ctx *ctx, const uint32_t *tlwe1 /* [count][N+1] */,
                           uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_ifft_i32_batch(rtfhe_ctx *ctx, const int32_t *src /* [count][N] */, double *res /* [count][N] */, size_t count);
int rtfhe_fft_u32_batch(rtfhe_ctx *ctx, const double *src /* [count][N] */, uint32_t *res /* [count][N] */, size_t count);
/* the rest of the reference's FFT FFI (off the gate path; utils/src/spqlios.rs:18-32, only its N = 16 unit test uses poly_mul) */
int rtfhe_ifft_f64_batch(rtfhe_ctx *ctx, const double *src /* [count][N] */, double *res /* [count][N] */, size_t count);
int rtfhe_fft_f64_batch(rtfhe_ctx *ctx, const double *src /* [count][N] */, double *res /* [count][N], no truncation */, size_t count);
int rtfhe_poly_mul_batch(rtfhe_ctx *ctx, const uint32_t *a, const uint32_t *b, uint32_t *res /* [count][N] each */, size_t count);

/* ---- the reference's transforms at ANY power of two 16 <= N <= 2048 ----
 * The reference's FFT FFI takes every such N (Spqlios::new, utils/src/spqlios.rs:40-50; FFT_Processor_Spqlios, fft_processor_spqlios.cpp:7-14)
 * and its own unit test runs at N = 16 (spqlios.rs:243-276); a context exists for the gate path's N = 1024 / 2048 only.  A plan holds
 * the twiddle tables of one N on one device and runs the same butterfly networks (ifft_model / fft_model, spqlios-fft-impl.cpp:469-641 /
 * 204-397) on the GPU, one workgroup per polynomial: the same bytes as the reference for every N, with no claim of speed.  Not
 * thread-safe (one plan per host thread, as the reference's thread_local FFT_MAP, math.rs:349-351); host pointers in and out; errors
 * through rtfhe_last_error(NULL).  The Spqlios_* symbols of rtfhe_spqlios.h use a plan for every N other than 1024 / 2048. */
typedef struct rtfhe_fft_plan rtfhe_fft_plan;
int rtfhe_fft_plan_create(int32_t N, int device_id, rtfhe_fft_plan **out);      /* FFT_Processor_Spqlios(N), fft_processor_spqlios.cpp:7-14 */
void rtfhe_fft_plan_destroy(rtfhe_fft_plan *plan);
int32_t rtfhe_fft_plan_degree(const rtfhe_fft_plan *plan);
int rtfhe_fft_plan_get_twiddles(const rtfhe_fft_plan *plan, double *ifft_table /* [2N] */, double *fft_table /* [2N] */);   /* reference layout */
int rtfhe_fft_plan_set_twiddles(rtfhe_fft_plan *plan, const double *ifft_table, const double *fft_table);
int rtfhe_fft_plan_ifft_i32(rtfhe_fft_plan *plan, const int32_t *src, double *res, size_t count);    /* execute_reverse_int / _torus32 */
int rtfhe_fft_plan_ifft_f64(rtfhe_fft_plan *plan, const double *src, double *res, size_t count);     /* execute_reverse */
int rtfhe_fft_plan_fft_u32(rtfhe_fft_plan *plan, const double *src, uint32_t *res, size_t count);    /* execute_direct_torus32 */
int rtfhe_fft_plan_fft_f64(rtfhe_fft_plan *plan, const double *src, double *res, size_t count);      /* execute_direct */
int rtfhe_fft_plan_poly_mul(rtfhe_fft_plan *plan, const uint32_t *a, const uint32_t *b, uint32_t *res, size_t count);   /* spqlios-wrapper.cpp:38-53 */

/* ---- key generation / encryption (host side) ----
 * Production entry points draw every key bit, mask and noise sample from the OS CSPRNG (getrandom(2), expanded with ChaCha20),
 * as the reference draws from rand::thread_rng (utils/src/math.rs:417-479).  They fail with RTFHE_ERR_STATE if the OS gives
 * no entropy.  rtfhe_keygen_with_keys is TFHE::new for caller-supplied secret keys (hom_nand/src/tfhe.rs:21-25). */
int rtfhe_keygen(const rtfhe_params *p, int32_t *key0 /* [n] */, int32_t *key1 /* [N] */,
                 uint32_t *bk /* [n][2][2l][N] */, uint32_t *ksk /* [N][t][base-1][n+1] */);
int rtfhe_keygen_with_keys(const rtfhe_params *p, const int32_t *key0, const int32_t *key1, uint32_t *bk, uint32_t *ksk);
int rtfhe_tlwe_encrypt_bits(const rtfhe_params *p, const int32_t *key0, const uint8_t *bits, uint32_t *out /* [count][n+1] */,
                            size_t count);
/* rtfhe_tlwe_encrypt_bits with the plaintext torus words mu[count] given directly (same CSPRNG, same noise alpha = 2^-15): multi-bit
 * messages for rtfhe_pbs_batch */
int rtfhe_tlwe_encrypt_torus(const rtfhe_params *p, const int32_t *key0, const uint32_t *mu, uint32_t *out /* [count][n+1] */,
                             size_t count);
/* TRLWE encryptions under key1 [N] of the polynomials mu[count][N] (OS CSPRNG, noise alpha = 2^-25 as the bootstrapping key's rows,
 * TRLWERep::encrypt / trlwe_zero, hom_nand/src/trlwe.rs:127-137): the rows of an encrypted table (rtfhe_lut_create_encrypted).
 * rtfhe_trlwe_phase gives b - a·s, i.e. mu plus the noise. */
int rtfhe_trlwe_encrypt_torus(const rtfhe_params *p, const int32_t *key1, const uint32_t *mu /* [count][N] */,
                              uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_trlwe_phase(const rtfhe_params *p, const int32_t *key1, const uint32_t *ct /* [count][2][N] */,
                      uint32_t *phase /* [count][N] */, size_t count);
/* TRGSW encryptions under key1 [N] of the bits[count] (OS CSPRNG): what rtfhe_keygen does for every bit of key0 to make the bootstrapping key
 * (Crypto<i32> for TRGSW, hom_nand/src/trgsw.rs:118-138, 217-229; noise alpha = 2^-25), each in the layout of one key entry, u32[2][2l][N]: the
 * encrypted address bits of a CMUX tree (rtfhe_trgsw_create). */
int rtfhe_trgsw_encrypt_bits(const rtfhe_params *p, const int32_t *key1, const uint8_t *bits /* [count] */,
                             uint32_t *out /* [count][2][2l][N] */, size_t count);
/* TRGSW encryptions under key1 [N] of the small-integer polynomials mu[count][N] (OS CSPRNG): rtfhe_trgsw_encrypt_bits (Crypto<i32> for TRGSW,
 * hom_nand/src/trgsw.rs:118-138; the product they feed is trgsw.rs:264-306) with mu(X) * 2^(32 - (j+1) bgbit), wrapping, added over all N
 * coefficients of gadget position j where that adds bit * 2^(32 - (j+1) bgbit) at coefficient 0.  Same layout, same noise alpha = 2^-25, same
 * order of the mask and noise draws: the encrypted weights of rtfhe_trlwe_mul_trgsw_batch, uploaded through rtfhe_trgsw_create. */
int rtfhe_trgsw_encrypt_polys(const rtfhe_params *p, const int32_t *key1, const int32_t *mu /* [count][N] */,
                              uint32_t *out /* [count][2][2l][N] */, size_t count);
/* The switching key of rtfhe_trlwe_auto_batch for the exponents t[n_t] (OS CSPRNG): row (e, j) a TRLWE under key_to [N] of the polynomial
 * -sigma_{t[e]}(key_from) * 2^(32 - (j+1) bgbit), a zero encryption as the bootstrapping key's rows (noise alpha = 2^-25) plus that message.
 * Refused with RTFHE_ERR_INVALID: a null argument, a key that is not binary, n_t outside [1, 64], a t that is even or outside [1, 2N), an
 * exponent given twice.  key_from == key_to: automorphism keys; t = 1 and two keys: a re-keying key. */
int rtfhe_trlwe_ksk_keygen(const rtfhe_params *p, const int32_t *key_from /* [N] */, const int32_t *key_to /* [N] */, const int32_t *t /* [n_t] */,
                           int32_t n_t, uint32_t *out /* [n_t][l][2][N] */);
/* sigma_t : X -> X^t on count polynomials of u32 coefficients, on the CPU: x[j] goes to out[j t mod 2N mod N], negated when j t mod 2N >= N.
 * N a power of two, t odd and in [1, 2N); out may be exactly x.  For clients (sigma_t of a plaintext, of a key) and tests. */
int rtfhe_trlwe_automorphism(int32_t N, int32_t t, const uint32_t *x /* [count][N] */, uint32_t *out /* [count][N] */, size_t count);
/* the reference's KeySwitchingKey shape from the compact one: entries t = 1 .. base-1 of every level copied, entry t = base =
 * TLWE(base * s_i / 2^(basebit (l+1))) freshly encrypted as KeySwitchingKey::new fills it (hom_nand/src/tlwe.rs:252-274) */
int rtfhe_ksk_expand_ref(const rtfhe_params *p, const int32_t *key0, const int32_t *key1,
                         const uint32_t *ksk /* [N][t][base-1][n+1] */, uint32_t *ksk_ref /* [N][t][base][n+1] */);
/* TEST ONLY -- NOT SECURE: the same, reproducible from a 64-bit seed expanded through xoshiro256** (not a CSPRNG: whoever knows
 * the seed regenerates every mask and noise sample and recovers the secret key from the key-switching key; a reused seed
 * reuses mask and noise).  For fixtures, parity tests and benchmarks only; never for keys or ciphertexts that protect data. */
int rtfhe_keygen_deterministic(const rtfhe_params *p, uint64_t seed, int32_t *key0, int32_t *key1, uint32_t *bk, uint32_t *ksk);
int rtfhe_keygen_with_keys_deterministic(const rtfhe_params *p, uint64_t seed, const int32_t *key0, const int32_t *key1,
                                         uint32_t *bk, uint32_t *ksk);
int rtfhe_ksk_expand_ref_deterministic(const rtfhe_params *p, uint64_t seed, const int32_t *key0, const int32_t *key1,
                                       const uint32_t *ksk, uint32_t *ksk_ref);
int rtfhe_tlwe_encrypt_bits_deterministic(const rtfhe_params *p, const int32_t *key0, uint64_t seed,
                                          const uint8_t *bits, uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_tlwe_encrypt_torus_deterministic(const rtfhe_params *p, const int32_t *key0, uint64_t seed,
                                            const uint32_t *mu, uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_trlwe_encrypt_torus_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t seed,
                                            const uint32_t *mu /* [count][N] */, uint32_t *out /* [count][2][N] */, size_t count);
int rtfhe_trgsw_encrypt_bits_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t seed, const uint8_t *bits /* [count] */,
                                           uint32_t *out /* [count][2][2l][N] */, size_t count);
/* (with a constant polynomial mu = bit and the same seed: the words of rtfhe_trgsw_encrypt_bits_deterministic; trgsw.rs:118-138, 264-306) */
int rtfhe_trgsw_encrypt_polys_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t seed, const int32_t *mu /* [count][N] */,
                                            uint32_t *out /* [count][2][2l][N] */, size_t count);
int rtfhe_trlwe_ksk_keygen_deterministic(const rtfhe_params *p, const int32_t *key_from, const int32_t *key_to, uint64_t seed,
                                         const int32_t *t /* [n_t] */, int32_t n_t, uint32_t *out /* [n_t][l][2][N] */);
int rtfhe_tlwe_decrypt_bits(const rtfhe_params *p, const int32_t *key0, const uint32_t *in,
                            uint8_t *bits, size_t count);
int rtfhe_tlwe_phase(const rtfhe_params *p, const int32_t *key0, const uint32_t *in, uint32_t *phase, size_t count);

/* ---- seeded ciphertexts: TRLWE masks regenerated from a public seed (no reference counterpart) ----
 * Half of every TRLWE row is a uniformly random mask that carries no information.  A seeded object ships a 32-byte seed and the b polynomials
 * only, and the receiver regenerates the a polynomials: half the bytes on the wire and over PCIe.
 *
 * THE MASK RULE.  A mask seed is a ChaCha20 key, u32[8].  Rows are numbered by a uint64_t.  Row R of length N has
 *     a[16 c + i] = word i of the ChaCha20 block (RFC 8439 2.3) with key = seed, the 64-bit block counter c in state words 12-13 and R in state
 *                   words 14-15, for c = 0 .. N/16 - 1
 * -- the RFC's keystream with a 32-bit counter from 0 and the nonce words (0, R lo, R hi), and the generator of the production encryptors above
 * read word by word.  The mask word is the keystream word itself, all 32 bits (the unseeded encryptors draw 24-bit masks, as the reference does).
 *
 * A seeded object is (seed, first_row, b): b is u32[rows][N] in the object's row order, row r masked by row first_row + r of the seed, and `group`
 * says how rows interleave in the full layout u32[rows / group][2][group][N] (the b polynomials of a group, then its a polynomials):
 *     TRLWE tables and rows u32[count][2][N]                      group 1
 *     TRGSW sets and the bootstrapping key u32[count][2][2l][N]   group 2l
 *     the packing key u32[n][t][base-1][2][N]                     group 1
 *
 * SECURITY RULES.  The seed is public.  The noise never comes from the seed: the production encryptors draw it from a separate OS-seeded ChaCha
 * key, as the unseeded ones do, and the test-only forms from xoshiro256**.  A (seed, row) pair must never mask two ciphertexts under one key:
 * that reveals the difference of their phases.  The production encryptors therefore draw a fresh seed from the OS on every call, write it to
 * `seed` and number rows from 0; only the *_deterministic forms take a seed and a first_row (TEST ONLY -- NOT SECURE, as the ones above).
 *
 * Noise, message words and their placement are the unseeded encryptors'.  Where those add the message to an a polynomial (gadget rows l .. 2l-1
 * of a TRGSW sample) the seeded row is the zero encryption under (mask - message), so that the expanded row (b, mask) is one the unseeded
 * encryptor could have produced.  A seeded bootstrapping key needs no function of its own: it is rtfhe_trgsw_encrypt_bits_seeded with bits =
 * key0 (count = n), loaded by rtfhe_load_bk_seeded.
 *
 * Every call returns RTFHE_ERR_INVALID before anything else happens for: a null pointer; N not a power of two in 16 .. 2048; group < 1; rows not a
 * multiple of group; first_row + rows beyond 2^64; (encryptors) a non-binary key. */
int rtfhe_mask_expand(int32_t N, const uint32_t *seed /* [8] */, uint64_t first_row, uint32_t *a /* [rows][N] */, size_t rows);
/* the full layout on the CPU: the oracle of the device form below and the path of a server without this library's GPU side; b and out must not overlap */
int rtfhe_seeded_expand(const rtfhe_params *p, const uint32_t *seed /* [8] */, uint64_t first_row, const uint32_t *b /* [rows][N] */, int32_t group,
                        uint32_t *out /* [rows/group][2][group][N] */, size_t rows);
/* the seeded forms of rtfhe_trlwe_encrypt_torus, rtfhe_trgsw_encrypt_bits, rtfhe_trgsw_encrypt_polys and rtfhe_packing_keygen (centred noise):
 * each writes the b halves only, and the fresh seed */
int rtfhe_trlwe_encrypt_torus_seeded(const rtfhe_params *p, const int32_t *key1, const uint32_t *mu /* [count][N] */, uint32_t *seed /* out [8] */,
                                     uint32_t *b /* [count][N] */, size_t count);
int rtfhe_trgsw_encrypt_bits_seeded(const rtfhe_params *p, const int32_t *key1, const uint8_t *bits /* [count] */, uint32_t *seed /* out [8] */,
                                    uint32_t *b /* [count][2l][N] */, size_t count);
int rtfhe_trgsw_encrypt_polys_seeded(const rtfhe_params *p, const int32_t *key1, const int32_t *mu /* [count][N] */, uint32_t *seed /* out [8] */,
                                     uint32_t *b /* [count][2l][N] */, size_t count);
int rtfhe_packing_keygen_seeded(const rtfhe_params *p, const int32_t *key0, const int32_t *key1, uint32_t *seed /* out [8] */,
                                uint32_t *b /* [n][t][base-1][N] */);
/* TEST ONLY -- NOT SECURE: the noise reproducible from noise_seed through xoshiro256**, the mask seed and its first row the caller's */
int rtfhe_trlwe_encrypt_torus_seeded_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t noise_seed, const uint32_t *seed /* [8] */,
                                                   uint64_t first_row, const uint32_t *mu, uint32_t *b, size_t count);
int rtfhe_trgsw_encrypt_bits_seeded_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t noise_seed, const uint32_t *seed /* [8] */,
                                                  uint64_t first_row, const uint8_t *bits, uint32_t *b, size_t count);
int rtfhe_trgsw_encrypt_polys_seeded_deterministic(const rtfhe_params *p, const int32_t *key1, uint64_t noise_seed, const uint32_t *seed /* [8] */,
                                                   uint64_t first_row, const int32_t *mu, uint32_t *b, size_t count);
int rtfhe_packing_keygen_seeded_deterministic(const rtfhe_params *p, uint64_t noise_seed, const int32_t *key0, const int32_t *key1,
                                              const uint32_t *seed /* [8] */, uint64_t first_row, uint32_t *b);
/* On the device (every backend, no key, the primary device of a multi-device context): one launch of k_seeded_expand writes the whole full-layout
 * object from d_b, which stays as it is.  Asynchronous and ordered on `stream`; nothing is allocated and the seed travels in the launch itself, so
 * the call may be captured first thing on a fresh stream.  d_b and d_out must be 16-byte aligned and must not overlap, and rows * N / 16 stays
 * below 2^31.  This is how compact input rows for rtfhe_trlwe_mul_plain_batch_dev, rtfhe_trlwe_mul_trgsw_batch_dev, rtfhe_demux_tree_batch_dev and
 * rtfhe_lut_update_dev become full rows on the device. */
int rtfhe_seeded_expand_dev(rtfhe_ctx *ctx, const uint32_t *seed /* host [8] */, uint64_t first_row, const void *d_b /* [rows][N] */, int32_t group,
                            void *d_out /* [rows/group][2][group][N] */, size_t rows, void *stream);
/* The upload calls' seeded forms.  Each uploads b (half the bytes of its twin), expands it on the device into the buffer the twin copies the full words
 * into, and from there on IS the twin: same conversion, same handle, lifetime, error codes and memory accounting (the b halves pass through the
 * context's staging). */
int rtfhe_trgsw_create_seeded(rtfhe_ctx *ctx, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [n_sel][2l][N] */, int32_t n_sel,
                              rtfhe_trgsw **out);
int rtfhe_trgsw_update_seeded(rtfhe_trgsw *sel, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [n][2l][N] */, int32_t first, int32_t n);
int rtfhe_lut_create_encrypted_seeded(rtfhe_ctx *ctx, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [n_lut][N] */, int32_t n_lut,
                                      rtfhe_lut **out);
/* (the derived exact-backend keys and the peers' replicas follow as in rtfhe_load_bk_torus) */
int rtfhe_load_bk_seeded(rtfhe_ctx *ctx, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [n][2l][N] */);
int rtfhe_packing_key_create_seeded(rtfhe_ctx *ctx, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [n][t][base-1][N] */,
                                    rtfhe_packing_key **out);

/* ---- seeded lvl0 ciphertexts and the seeded key-switching key (no reference counterpart) ----
 * A lvl0 row is n mask words and ONE word of information: gate, MUX, PBS and circuit inputs u32[n+1], and the 24,576 rows of the key-switching
 * key.  A seeded lvl0 object ships a 32-byte seed and one word per row.
 *
 * THE MASK RULE FOR ROWS OF LENGTH n.  The stream is the one of the rule above, cut at n words.  Row R of a lvl0 object has
 *     a[16 c + i] = word i of the ChaCha20 block (RFC 8439 2.3) with key = seed, the 64-bit block counter c in state words 12-13 and R in state
 *                   words 14-15, for c = 0 .. ceil(n / 16) - 1; the words with 16 c + i >= n are discarded
 * so for n a multiple of 16 the masks are rtfhe_mask_expand(N = n, ...)'s.  The mask word is the keystream word itself, all 32 bits.
 *
 * A seeded lvl0 object is (seed, first_row, b): b is u32[rows], row r masked by row first_row + r of the seed; the full layout is u32[rows][n+1],
 * a[0 .. n) then b -- the layout of every lvl0 batch and of the key-switching key u32[N][t][base-1][n+1], whose row (i, l, d) is row
 * (i t + l)(base - 1) + d.
 *
 * SECURITY RULES: those of the seeded ciphertexts above.  The seed is public; the noise never comes from it; the production encryptors draw a fresh
 * seed per call, write it to `seed` and number rows from 0; only the *_deterministic forms take a seed and a first_row (TEST ONLY -- NOT SECURE).
 * b = <a, key0> + message + e with the unseeded encryptors' message word and noise sampler (sigma = 2^-15).
 *
 * Every call returns RTFHE_ERR_INVALID before anything else happens for: a null pointer; n < 1 (a context's calls: n <= 767 by construction);
 * rows = 0; first_row + rows beyond 2^64; b overlapping out; (encryptors, key generation) a non-binary key. */
int rtfhe_tlwe_mask_expand(int32_t n, const uint32_t *seed /* [8] */, uint64_t first_row, uint32_t *a /* [rows][n] */, size_t rows);
/* the full layout on the CPU: the oracle of the device form below and the path of a server without this library's GPU side */
int rtfhe_tlwe_seeded_expand(const rtfhe_params *p, const uint32_t *seed /* [8] */, uint64_t first_row, const uint32_t *b /* [rows] */,
                             uint32_t *out /* [rows][n+1] */, size_t rows);
/* the seeded forms of rtfhe_tlwe_encrypt_bits and rtfhe_tlwe_encrypt_torus: each writes one b word per message, and the fresh seed */
int rtfhe_tlwe_encrypt_bits_seeded(const rtfhe_params *p, const int32_t *key0, const uint8_t *bits /* [count] */, uint32_t *seed /* out [8] */,
                                   uint32_t *b /* [count] */, size_t count);
int rtfhe_tlwe_encrypt_torus_seeded(const rtfhe_params *p, const int32_t *key0, const uint32_t *mu /* [count] */, uint32_t *seed /* out [8] */,
                                    uint32_t *b /* [count] */, size_t count);
/* the key-switching key of rtfhe_keygen in seeded form: row (i, l, d) encrypts (d + 1) key1[i] 2^(32 - basebit (l + 1)) under key0 */
int rtfhe_ksk_keygen_seeded(const rtfhe_params *p, const int32_t *key0, const int32_t *key1, uint32_t *seed /* out [8] */,
                            uint32_t *b /* [N][t][base-1] */);
/* TEST ONLY -- NOT SECURE: the noise reproducible from noise_seed through xoshiro256**, the mask seed and its first row the caller's */
int rtfhe_tlwe_encrypt_bits_seeded_deterministic(const rtfhe_params *p, const int32_t *key0, uint64_t noise_seed, const uint32_t *seed /* [8] */,
                                                 uint64_t first_row, const uint8_t *bits, uint32_t *b, size_t count);
int rtfhe_tlwe_encrypt_torus_seeded_deterministic(const rtfhe_params *p, const int32_t *key0, uint64_t noise_seed, const uint32_t *seed /* [8] */,
                                                  uint64_t first_row, const uint32_t *mu, uint32_t *b, size_t count);
int rtfhe_ksk_keygen_seeded_deterministic(const rtfhe_params *p, uint64_t noise_seed, const int32_t *key0, const int32_t *key1,
                                          const uint32_t *seed /* [8] */, uint64_t first_row, uint32_t *b);
/* On the device (every backend, no key, the primary device of a multi-device context): one launch of k_tlwe_seeded_expand writes rows * (n + 1)
 * words at d_out, the masks to columns 0 .. n - 1 and d_b[r] to column n; d_b stays as it is.  Asynchronous and ordered on `stream`; nothing is
 * allocated and the seed travels in the launch itself, so the call may be captured first thing on a fresh stream.  d_b and d_out need 4-byte
 * alignment only -- d_out may be a range of rows inside a larger wire table u32[..][n+1] -- and must not overlap; rows * ceil(n / 16) stays below
 * 2^31.  This is how seeded inputs become the rows the *_dev batch calls read. */
int rtfhe_tlwe_seeded_expand_dev(rtfhe_ctx *ctx, const uint32_t *seed /* host [8] */, uint64_t first_row, const void *d_b /* [rows] */,
                                 void *d_out /* [rows][n+1] */, size_t rows, void *stream);
/* rtfhe_load_ksk from the key's seeded form: uploads b (one word per row), makes the masks on the device in the staging buffer rtfhe_load_ksk copies
 * its words into, and from there on IS rtfhe_load_ksk: same device layouts, peers' replicas, error codes and memory accounting. */
int rtfhe_load_ksk_seeded(rtfhe_ctx *ctx, const uint32_t *seed, uint64_t first_row, const uint32_t *b /* [N][t][base-1] */);

/* ---- compressed results: k-bit, bit-packed ciphertexts off the GPU ----
 * The seeded forms above cut what a client sends; this cuts what comes back.  A result's mask is computed, so no seed stands for it -- but its low
 * bits are noise (a bootstrapped lvl0 ciphertext has sigma ~ 0.0116 of the torus in reference mode, 0.0028 in rounded mode, on messages spaced
 * 1/8 .. 1/32 apart).  Keeping the top k bits of every word and packing them densely is modulus switching plus bit packing: a lvl0 result is 795
 * bytes at k = 10 instead of 2,544, and 1,024 results packed into one TRLWE (rtfhe_pack_batch) are 3 KB at k = 12.  The rounding and packing run
 * on the GPU, in the stream or captured graph of the computation, so only the small buffer crosses the bus; the key holder expands on the CPU, and a
 * server that takes stored or forwarded rows up again expands them on the GPU (rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev below).
 *
 * One row.  A row of L torus words v[0 .. L) and a width k, 2 <= k <= 32:
 *   - rounding: r[i] = ((v[i] + 2^(31-k)) mod 2^32) >> (32 - k), a k-bit value: round to nearest, ties up, wrapping -- a word that rounds up to
 *     2^k becomes 0.  For k = 32, r[i] = v[i].
 *   - packing: the row is a little-endian bit stream of L k bits.  Bit j of r[i] is stream bit i k + j; stream bit s is bit s mod 32 of output
 *     word s / 32.
 *   - size: a row occupies W(L, k) = ceil(L k / 32) u32 words (rtfhe_compressed_words); the unused high bits of the last word are ZERO; every row
 *     starts on a word boundary: the output is u32[count][W].
 *   - expansion: v'[i] = r[i] << (32 - k), so |v' - v| <= 2^(31-k) on every word, mod 2^32.
 *
 * Noise, and choosing k.  Under a binary key with h ones the phase of the expanded ciphertext differs from the original's by at most
 * (h + 1) 2^-(k+1) of the torus; the spread is about sqrt((h + 1) / 12) 2^-k.  At k = 12, N = 1024 and a random binary key that is a spread of
 * 0.0015 (measured; worst case seen 0.0054 against the bound 0.062).  The bound is a worst case no real row comes near; size k by the spread,
 * against the distance between messages and the noise the result already has.  Choosing k is the caller's job: nothing here knows the message space.
 *
 * lvl0 form.  The input is [count][n+1]; the row is the whole sample, L = n + 1.
 * TRLWE form.  The input is [count][2][N], b then a, with a coefficient list exactly as rtfhe_trlwe_extract_batch takes it: a host coef[P], or
 * NULL for p * stride; 1 <= P <= N; duplicates allowed; copied into the launch arguments when the call is enqueued (a stream capture bakes it
 * in).  The row is a[0 .. N) followed by b[coef[0]], .., b[coef[P-1]], so L = N + P: the key holder only needs the b coefficients that carry a
 * result (P = N, k = 12 at N = 1024: 768 words instead of 2,048).  Expansion gives a full [2][N] row whose b is zero at the coefficients that
 * were not kept -- rtfhe_trlwe_phase and the extract calls read it as it stands; with duplicate coefficients the later entry wins.
 *
 * On the device: asynchronous and ordered on `stream`, on the context's primary device, on every backend, with no key loaded.  Nothing is
 * allocated, so a call may be captured first thing on a fresh stream.  One launch of k_compress_rows, one more per further 512 coefficients.
 * Checked before anything is launched, RTFHE_ERR_INVALID with a message: null handles or buffers; k outside 2 .. 32; the coefficient list's
 * rules; count * L < 2^31; the output overlapping the input.  count == 0 returns 0. */
int rtfhe_tlwe_compress_batch_dev(rtfhe_ctx *ctx, int32_t k, const void *d_tlwe /* [count][n+1] */, void *d_out /* u32[count][W(n+1,k)] */,
                                  size_t count, void *stream);
int rtfhe_trlwe_compress_batch_dev(rtfhe_ctx *ctx, int32_t k, const void *d_trlwe /* [count][2][N] */, int32_t P,
                                   const int32_t *coef /* HOST [P] or NULL */, int32_t stride, void *d_out /* u32[count][W(N+P,k)] */, size_t count,
                                   void *stream);
/* The other direction on the device: packed rows that came up from the host -- results kept at rest, handed over by another server, read from an
 * "RTFHECZ1" file -- become full rows in the computation's own stream, so the packed bytes are all that cross the bus (lvl0, k = 10: 796 bytes
 * instead of 2,544).  Word for word the CPU twins below: value i of a row is the k-bit field at stream bits [i k, i k + k) of its W words and
 * the expanded word is value << (32 - k) (k = 32: the word itself).  lvl0 form: d_tlwe[g][i] = value i, i = 0 .. n.  TRLWE form: the a
 * polynomial d_trlwe[g][1][i] = value i, i < N; b[j] = value N + p for the LAST p with coef[p] = j (the later entry wins) and 0 at every other
 * j.  The list follows the compress call's rules (a host coef[P], or NULL for p * stride) and is copied into the launch arguments when the call is
 * enqueued.  Bits of a row's last word past L k reach no result; no packed word outside a row's W words is read.
 *   Each call writes exactly count * (n + 1), or count * 2 N, words, each once by a plain store, whatever the buffer held; rows past `count` keep
 * their bytes.  d_words and the output need 4-byte alignment only: d_tlwe may be a range of rows of a wire table.  The contract is the compress
 * calls': asynchronous and ordered on `stream`, primary device, every backend, no key, nothing allocated, capturable first thing on a fresh
 * stream; the same checks before anything is launched (the full rows are now the output), RTFHE_ERR_INVALID with a message; count == 0 returns 0.
 *   Launches of k_expand_rows: one for lvl0 rows and for coef == NULL.  With a list the kept coefficients travel as an inverse map (for each
 * j, -1 or the last p) in the launch arguments, 1,024 entries a launch: ceil(N / 1024) launches -- one at N = 1024, two at N = 2048. */
int rtfhe_tlwe_expand_batch_dev(rtfhe_ctx *ctx, int32_t k, const void *d_words /* u32[count][W(n+1,k)] */, void *d_tlwe /* [count][n+1] */,
                                size_t count, void *stream);
int rtfhe_trlwe_expand_batch_dev(rtfhe_ctx *ctx, int32_t k, const void *d_words /* u32[count][W(N+P,k)] */, int32_t P,
                                 const int32_t *coef /* HOST [P] or NULL */, int32_t stride, void *d_trlwe /* [count][2][N] */, size_t count,
                                 void *stream);
/* The key holder's side, and the host-buffer form of this feature: the same words on the CPU and their inverses, from a plain n or N, with no
 * context and no GPU (there is no upload-compress-download call: rows that are already on the host are compressed here).  Same checks, returned as
 * RTFHE_ERR_INVALID; in and out must not overlap. */
size_t rtfhe_compressed_words(size_t L, int32_t k);            /* W(L, k); 0 for k outside 2 .. 32 */
int rtfhe_tlwe_compress(int32_t n, int32_t k, const uint32_t *in /* [count][n+1] */, uint32_t *out /* [count][W] */, size_t count);
int rtfhe_tlwe_expand(int32_t n, int32_t k, const uint32_t *in /* [count][W] */, uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_trlwe_compress(int32_t N, int32_t k, int32_t P, const int32_t *coef /* [P] or NULL */, int32_t stride, const uint32_t *in /* [count][2][N] */,
                         uint32_t *out /* [count][W] */, size_t count);
int rtfhe_trlwe_expand(int32_t N, int32_t k, int32_t P, const int32_t *coef /* [P] or NULL */, int32_t stride, const uint32_t *in /* [count][W] */,
                       uint32_t *out /* [count][2][N] */, size_t count);

/* ---- wire format (flat little-endian files with an FNV-1a checksum; the reference has no serialization) ----
 * key file   "RTFHEKY1" | rtfhe_params | u32 flags (1 bk, 2 ksk, 4 secret keys) | u32 0 | [key0 | key1] | [bk] | [ksk] | u64 fnv
 * batch file "RTFHECT1" | i32 n | i32 0 | u64 count | u32[count][n+1] | u64 fnv */
int rtfhe_keys_write(const char *path, const rtfhe_params *p, const int32_t *key0, const int32_t *key1,
                     const uint32_t *bk, const uint32_t *ksk);          /* null sections are left out */
int rtfhe_keys_read_header(const char *path, rtfhe_params *p, uint32_t *flags);
/* Buffers are sized for the parameter set rtfhe_keys_read_header returns (call it first); null = skip that section; asking for a
 * section the file does not hold (see flags) fails. */
int rtfhe_keys_read(const char *path, int32_t *key0, int32_t *key1, uint32_t *bk, uint32_t *ksk);
int rtfhe_tlwe_write(const char *path, int32_t n, const uint32_t *cts, size_t count);
int rtfhe_tlwe_read(const char *path, int32_t *n, uint64_t *count, uint32_t *cts /* NULL: header only */, size_t capacity);
/* compressed file "RTFHECZ1" | i32 kind | i32 n or N | i32 k | i32 P (lvl0: 0) | u64 count | i32 coef[P] | u32[count][W] | u64 fnv
 * Compressed results (above) with what it takes to expand them.  dim is n for lvl0 rows and N for TRLWE rows; coef is the resolved list of kept
 * coefficients (rows compressed with coef NULL: p * stride), NULL with P = 0 for lvl0 rows.  Read the header first and size coef [P] and words
 * [count][W] from it; capacity is in rows.  A bad header field, a flipped bit or a short file is RTFHE_ERR_INVALID. */
#define RTFHE_COMPRESSED_TLWE 0
#define RTFHE_COMPRESSED_TRLWE 1
int rtfhe_compressed_write(const char *path, int32_t kind, int32_t dim, int32_t k, int32_t P, const int32_t *coef /* [P] or NULL */,
                           const uint32_t *words /* [count][W] */, size_t count);
int rtfhe_compressed_read_header(const char *path, int32_t *kind, int32_t *dim, int32_t *k, int32_t *P, uint64_t *count);
int rtfhe_compressed_read(const char *path, int32_t *coef /* [P] */, uint32_t *words /* [capacity][W] */, size_t capacity);

/* ---- multi-bit blind rotation: a programmable bootstrap in ceil(n / g) dependent steps instead of n ----
 * The key bits are cut into groups of g = 2 or 3: group t covers bits [t g, min(n, t g + g)), the last one ragged when g does not divide n.
 * With abar_i, bbar, the table row tv and the starting accumulator acc = X^{-bbar} (tv, 0) exactly as in rtfhe_pbs_batch, one step per group:
 *
 *     acc = acc + (Sum_{j = 1 .. J} F_{e_j} . BK_{t,j}) [.] acc            J = 2^g' - 1, g' the bits of the group
 *     e_j = Sum_{q in j} abar_{t g + q}  mod 2N                            bit q of the subset number j = bit t g + q of the key
 *     out[g] = identity_key_switch(sample_extract_0(acc))                  after the last group
 *
 * BK_{t,j} is a TRGSW sample under key1 of the constant  prod_{q in j} s_q  prod_{q not in j} (1 - s_q)  -- 1 exactly when the set bits of the
 * group are those of j -- with the bootstrapping key's gadget and noise, and [.] the external product of rtfhe_external_product_batch in the
 * decomposition rtfhe_set_decomposition selects.  F_e is the spectrum of X^e - 1 in the transform's own point order:
 * F_e[p] = W[(e q_p) mod 2N] - 1, W[t] = exp(i pi t / N) (rtfhe_mb_roots: double[2N][2], cos then sin of the double pi * t / N, W[0] = 1 exactly)
 * and q_p the odd exponent at which the forward transform leaves its value at point p = m * 64 + lane of the device layout
 * (rtfhe_mb_point_exponents: int32[N/2]).  Both tables are plain functions of N and need no context.
 * Every product and sum is rounded on its own, in this order per digit row, output component and point: K = F_{e_1} B_1, then
 * K = K + F_{e_j} B_j for j = 2 .. J, each complex product as (re re - im im, im re + re im); K then stands where the single-bit step has its
 * key row; the truncated product is added into acc.  No subset is left out when e_j = 0.
 * The output decrypts like rtfhe_pbs_batch's; its words differ (another key, another order of roundings).
 *
 * The key.  rtfhe_mbk_words gives its size in words (0 for bad arguments): n_trgsw * 4 l N, n_trgsw = floor(n / g) (2^g - 1) + 2^(n mod g) - 1,
 * i.e. 1.5 x the bootstrapping key at g = 2 and 2.33 x at g = 3.  rtfhe_mbk_keygen fills u32[n_trgsw][2][2l][N], every sample in the layout
 * of one bootstrapping-key entry, groups in order, j ascending, from the OS CSPRNG; rtfhe_mbk_keygen_deterministic (TEST ONLY) from a seed.
 * Both refuse g outside {2, 3} and non-binary keys (RTFHE_ERR_INVALID).
 * rtfhe_mbk_create converts it to spectra on the primary device (as rtfhe_load_bk_torus converts the bootstrapping key; 93.6 MB at the default
 * parameters and g = 2, 145.5 MB at g = 3, counted by rtfhe_ctx_memory_bytes) under the lifetime rule of every handle: normally destroyed before
 * its context; if the context goes first, the device copy goes with it, a later call with the key fails with RTFHE_ERR_STATE and
 * rtfhe_mbk_destroy only frees the handle.  The bootstrapping key itself is not needed; the key-switching key is.
 *
 * The calls follow rtfhe_pbs_batch[_dev]: plain tables from rtfhe_lut_create (an encrypted one: RTFHE_ERR_INVALID), lut_idx NULL = table 0,
 * indices checked on the host before anything is launched / on the device (a gate with a bad index is skipped, its output row keeps the
 * bytes it had on both routes to the key switch, and the next rtfhe_sync returns RTFHE_ERR_INVALID once); every check happens before any launch; the FP64 mirror backend only
 * (the exact backends: RTFHE_ERR_INVALID, the context stays usable); N = 1024 and 2048.  On a multi-device context the batch runs on the primary.
 * Inside a stream capture rtfhe_pbs_mb_batch_dev allocates nothing and needs no earlier call on the stream: there, and in a context without
 * the matrix form of the key-switching key (RTFHE_KS_MM_MIN=0), the kernel switches keys itself; otherwise the samples go through the stream's
 * sample buffer into the batch key switch, as a many-LUT PBS's do.  Both routes give the same words.
 * Two kernel shapes: a wave per gate (any count, both N; what N = 2048 runs on) and, at N = 1024, a workgroup of six waves per gate, which
 * every N = 1024 batch takes; they give the same words.  RTFHE_MB_SHAPE=wave|wg in the environment forces one (wg at N = 2048:
 * RTFHE_ERR_INVALID). */
typedef struct rtfhe_mbk rtfhe_mbk;
size_t rtfhe_mbk_words(const rtfhe_params *p, int32_t g);
int rtfhe_mbk_keygen(const rtfhe_params *p, int32_t g, const int32_t *key0, const int32_t *key1, uint32_t *out /* [n_trgsw][2][2l][N] */);
/* TEST ONLY (deterministic from a seed; NOT secure) */
int rtfhe_mbk_keygen_deterministic(const rtfhe_params *p, uint64_t seed, int32_t g, const int32_t *key0, const int32_t *key1, uint32_t *out);
int rtfhe_mb_roots(int32_t N, double *out /* [2N][2] */);
int rtfhe_mb_point_exponents(int32_t N, int32_t *out /* [N/2] */);
int rtfhe_mbk_create(rtfhe_ctx *ctx, const uint32_t *words, int32_t g, rtfhe_mbk **out);
void rtfhe_mbk_destroy(rtfhe_mbk *k);
int rtfhe_pbs_mb_batch(rtfhe_ctx *ctx, const rtfhe_mbk *mbk, const rtfhe_lut *lut, const int32_t *lut_idx /* [count] or NULL */,
                       const uint32_t *tlwe /* [count][n+1] */, uint32_t *out /* [count][n+1] */, size_t count);
int rtfhe_pbs_mb_batch_dev(rtfhe_ctx *ctx, const rtfhe_mbk *mbk, const rtfhe_lut *lut, const void *d_lut_idx /* int32[count] or NULL */,
                           const void *d_tlwe, void *d_out, size_t count, void *stream);

#ifdef __cplusplus
}
#endif
#endif
