/* playsnark_hip.h -- C ABI of the MI355X-native prover hot path for nikkolasg/playsnark.
 *
 * The reference is a single Go package with no FFI; this header is the boundary a cgo shim
 * binds (INTEGRATION.md shows the shim).  Each entry point names the reference function it
 * replaces (file:line under /root/reference).  Plain pointers and sizes only; all host
 * buffers are caller-owned and never retained past return (cgo pointer rules); handles are
 * opaque, library-owned and explicitly destroyed.  Functions return 0 or a negative
 * PS_ERR_*; nothing aborts or throws across the boundary.  A ps_ctx is not thread-safe;
 * distinct contexts are.
 *
 * Byte formats (big-endian, what kyber's MarshalBinary produces [upstream]):
 *   scalar      32 B canonical Fr element
 *   PS_FMT_AFFINE      G1 96 B  x||y ;  G2 192 B  x_c1||x_c0||y_c1||y_c0 ; identity = 0x40,0,0,...
 *   PS_FMT_COMPRESSED  G1 48 B / G2 96 B ZCash compressed (flags 0x80 | 0x40 inf | 0x20 sign)
 * Outputs are always PS_FMT_AFFINE unless stated.
 */
#ifndef PLAYSNARK_HIP_H
#define PLAYSNARK_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_OK 0
#define PS_ERR_LENGTH (-1)        /* algebra.go:350-352 panic "mismatch of length between poly ..." */
#define PS_ERR_NOT_DIVISIBLE (-2) /* qap.go:158-160, pinochio.go:214-216 panic("apocalypse")        */
#define PS_ERR_ENCODING (-3)      /* non-canonical field element / point not on the curve           */
#define PS_ERR_HIP (-4)           /* HIP runtime failure; see ps_last_error()                        */
#define PS_ERR_ARG (-5)           /* NULL handle, unsupported size, sanityCheck (qap.go:177-189)    */
#define PS_ERR_NO_DEVICE (-6)     /* no gfx950 device visible: the library has no CPU fallback      */

#define PS_FMT_AFFINE 0
#define PS_FMT_COMPRESSED 1

#define PS_G1 1
#define PS_G2 2

typedef struct ps_ctx ps_ctx;         /* one device + stream + workspace                       */
typedef struct ps_points ps_points;   /* device-resident point vector (a CRS array)            */
typedef struct ps_scalars ps_scalars; /* device-resident Fr vector                             */
typedef struct ps_qap ps_qap;         /* device-resident sparse QAP + per-n tables             */

/* ABI revision of this header.  Structs only ever grow at the tail, and only together with this number; a caller checks
 * ps_abi_version() == PS_ABI_VERSION once after loading the library.  Key / device structs (ps_groth16_pk, ps_phgr13_ek,
 * ps_groth16_device, ..) MUST be zero-initialised by the caller (memset or `= {0}`): an optional array that is NULL is
 * "not present", and garbage in a member added by a later revision would be dereferenced.
 *   1  round 1;  2  Lagrange-form key arrays (lxi / lxi2 / lxi_t / lgsi), multi-device entries;
 *   3  ps_msm_info.window_table, ps_msm_set_tail, ps_ctx_set_table_budget, ps_qap_is_valid, ps_microbench_mad;
 *   4  ps_points_monomial_to_lagrange; index-range views build window tables of their own; PS_MSM_QUEUE 3 -> 4 (no struct changed);
 *   5  ps_phgr13_prove_shard, ps_phgr13_prove_multi and its ps_phgr13_device (no existing struct changed);
 *      later within 5: ps_groth16_prove_local, and ps_groth16_prove_multi reads the optional lxi / lxi2 / lxi_t of
 *      ps_groth16_device.pk.  No struct changed, so the number stays: an entry point added within a revision is detected by
 *      its symbol (dlsym), not by ps_abi_version().  Likewise ps_qap_column_sums, ps_groth16_setup_from_srs (with the new
 *      ps_groth16_srs), ps_groth16_crs_contribute and ps_groth16_crs_check_update; then ps_scalars_powers,
 *      ps_groth16_srs_contribute (with the new ps_groth16_srs_share), ps_groth16_srs_check and ps_groth16_srs_check_update;
 *      then ps_points_lagrange_check and ps_groth16_crs_check_from_srs; then ps_qap_create_fr (with the new
 *      ps_csr_fr) and ps_qap_wide_entries; then ps_msm_batch, ps_msm_batch_set_chunk and ps_groth16_prove_batch;
 *      then ps_msm_batch_multi and ps_phgr13_prove_batch; then ps_msm_batch_set_table;
 *      then ps_phgr13_verify_batch and ps_phgr13_verify_batch_info (with the new ps_phgr13_batch_info);
 *      then ps_msm_prediction_counts; then ps_phgr13_verify_batch_locate and ps_phgr13_verify_batch_locate_info (with the
 *      new ps_phgr13_locate_info).  Then ps_poly_scan_tile, ps_poly_eval, ps_poly_div_linear, ps_kzg_commit, ps_kzg_open,
 *      ps_kzg_verify and ps_kzg_verify_batch (no struct at all).  Then ps_scalars_lincomb, ps_kzg_open_multi and
 *      ps_kzg_verify_multi (no struct either).  Then ps_poly_scan_set_group, ps_poly_div_roots, ps_kzg_open_set and
 *      ps_kzg_verify_set (no struct either).  Then ps_poly_lagrange_tile, ps_qap_gate_values, ps_poly_eval_lagrange,
 *      ps_poly_div_linear_lagrange, ps_kzg_commit_lagrange and ps_kzg_open_lagrange (no struct either).  Then
 *      ps_poly_lagrange_set_group, ps_poly_div_roots_lagrange and ps_kzg_open_set_lagrange (no struct either).  Then
 *      ps_kzg_all_key_lagrange and ps_kzg_open_all_lagrange (no struct either). */
#define PS_ABI_VERSION 5
int ps_abi_version(void);
const char* ps_last_error(void);
const char* ps_version(void);
int ps_device_count(void);

/* ---- context ---- */
/* Thread safety: a ps_ctx (and the ps_qap made on it) belongs to one host thread at a time; distinct contexts may run
 * on distinct threads concurrently, ALSO over the same ps_points / ps_scalars arrays (a key uploaded once, proved with
 * from several threads): the arrays are read-only to the sums, their reference counts are atomic, and a window table a
 * prover attaches on first use is built once under the array's own lock.  ps_points_precompute with another window
 * size or -1 (release), and ps_*_free, must not race with sums over the same array. */
int ps_ctx_create(int device, ps_ctx** out);
void ps_ctx_destroy(ps_ctx* ctx);
int ps_ctx_sync(ps_ctx* ctx);
/* Raw HIP stream of the context (hipStream_t as void*), for callers that time with events. */
void* ps_ctx_stream(ps_ctx* ctx);

/* ---- CRS / evaluation-key arrays: the []G1 / []G2 slices of Groth16Setup
 *      (groth16.go:30-61: Xi, Xi2, NioLP, XiT) and PHGR13EvalKey (pinochio.go:37-62) ---- */
/* Encodings are validated (canonical field elements, curve equation, identity = 0x40 then zeros / 0xC0 then
 * zeros): PS_ERR_ENCODING otherwise.  Membership in the order-r subgroup is NOT tested here (it costs a
 * scalar multiplication per point); arrays that come from an untrusted source go through
 * ps_points_check_subgroup, as kyber's UnmarshalBinary would have rejected such points [upstream]. */
int ps_points_upload(ps_ctx* ctx, int group /*PS_G1|PS_G2*/, const uint8_t* pts, size_t n, int fmt,
                     ps_points** out);
/* Window table of a resident array: T[w][i] = 2^(c w) P[i] for every window w of a c-bit signed-digit
 * decomposition (c = window_bits; 0 picks it from the array length: 20 at 2^20 points, 13 windows).  CRS arrays are
 * fixed across proofs (groth16.go:30-61, pinochio.go:37-62), so the table is built once; every later sum over
 * the array -- or over a ps_points_slice of it -- then lets all its windows share ONE bucket set: 13 instead of
 * 16 bucket additions per 255-bit scalar and a sixteenth of the buckets to reduce.  Results are the same group
 * elements, bit for bit.  Costs (255 / c + 1) rows of 128 B (G1) / 256 B (G2) per point in device memory (1.7 GB for
 * 2^20 G1 points at c = 20);
 * at most 2^26 - 1 points.  Sums take the plain path when a table is absent, when ps_msm_set_window
 * forces a window size, when the arrays of a ps_msm_multi call do not all carry tables of one window size, or when the
 * cost model prefers it (short scalars: an int64 witness).  window_bits = -1 releases the table (after waiting for the
 * device: sums may still read it). */
int ps_points_precompute(ps_ctx* ctx, ps_points* p, int window_bits);
int ps_points_table_window(const ps_points* p); /* window bits of the table, 0 = none */
/* ps_groth16_prove / ps_phgr13_prove build the tables of their CRS arrays themselves on first use (keys of at least
 * 32 points; cached per key; about 9 GB for a 2^20-constraint Groth16 key, 15 GB for a PHGR13 one).
 * enable = 0 keeps the provers on the plain plan. */
int ps_ctx_set_tables(ps_ctx* ctx, int enable);
/* Memory policy of those tables.  A prover builds a table only when it fits: `bytes` >= 0 caps ONE table (0: none fit),
 * negative (the default) = what hipMemGetInfo reports as free, less a sixteenth of the device (at least 2 GiB) kept for
 * the sums' own workspaces.  A table that does not fit -- or whose allocation fails -- is not an error: the sums over that
 * array take the plain plan, which needs no memory beyond the array (ps_msm_info.window_table tells which ran).  The array
 * is marked with what the asking context had to offer, and it IS asked again: by a later request with a larger budget, or
 * once a quarter more device memory is free than at the time; ps_points_precompute(p, -1) clears the mark at once.  An
 * explicit ps_points_precompute still fails with PS_ERR_HIP when the allocation fails. */
int ps_ctx_set_table_budget(ps_ctx* ctx, long long bytes);
/* *ok = 1 iff [r]P = O for every point of the array (GPU, ~400 group operations per point). */
int ps_points_check_subgroup(ps_ctx* ctx, const ps_points* p, int* ok);
/* out[i] = scalars[i] * G (fixed base).  GeneratePowersCommit (algebra.go:371-384) and the
 * commit loops of fullLinearPoly (groth16.go:254-264) / generateEvalCommit (pinochio.go:381-388)
 * reduce to this once the exponents are known. */
int ps_points_from_scalars(ps_ctx* ctx, int group, const ps_scalars* k, ps_points** out);
int ps_points_download(ps_ctx* ctx, const ps_points* p, size_t first, size_t n, uint8_t* out);
/* Same with the output format chosen: PS_FMT_COMPRESSED gives the 48 / 96-byte form of MarshalBinary
 * (pinochio.go:258-272), compressed on the GPU -- the at-rest form of key files. */
int ps_points_download_fmt(ps_ctx* ctx, const ps_points* p, size_t first, size_t n, int fmt, uint8_t* out);
size_t ps_points_len(const ps_points* p);
int ps_points_group(const ps_points* p);
/* A view of [first, first+n) sharing storage with `p` (index-range sharding, multi-GPU). */
int ps_points_slice(const ps_points* p, size_t first, size_t n, ps_points** out);
void ps_points_free(ps_points* p);

/* ---- scalar vectors: Poly = []Element (algebra.go:89) / Vector = []Value (algebra.go:13) ---- */
int ps_scalars_upload(ps_ctx* ctx, const uint8_t* be32, size_t n, ps_scalars** out);
/* Value.ToFieldElement = SetInt64 (curve.go:17-19): negatives map to r - |v|.  Sums over such a vector use
 * the short scalar |v| (64 bits: a quarter of the windows) and, for a negative value, the negated point --
 * the same group element for points of order r, which every CRS point is. */
int ps_scalars_upload_i64(ps_ctx* ctx, const int64_t* v, size_t n, ps_scalars** out);
/* Wrap n big-endian 32-byte scalars already resident in device memory (e.g. a torch tensor's
 * data_ptr()); the bytes are converted into a library-owned vector. */
int ps_scalars_from_device_be32(ps_ctx* ctx, const void* d_be32, size_t n, ps_scalars** out);
int ps_scalars_download(ps_ctx* ctx, const ps_scalars* s, size_t first, size_t n, uint8_t* out_be32);
size_t ps_scalars_len(const ps_scalars* s);
int ps_scalars_slice(const ps_scalars* s, size_t first, size_t n, ps_scalars** out);
void ps_scalars_free(ps_scalars* s);

/* ---- MSM: Poly.BlindEval (algebra.go:348-359), sumBlind (groth16.go:134-141), the NioLP loop
 *      (groth16.go:173-179), computeSolCommit (pinochio.go:222-229) ----
 * out = sum_i scalars[i] * points[i].  len(scalars) != len(points) returns PS_ERR_LENGTH, the
 * reference's panic at algebra.go:350-352.  `out` is 96 B (G1) or 192 B (G2), affine.
 * Size limit: windows x length < 2^32 digits (32-bit sort offsets): 2^28 full-width scalars per call,
 * PS_ERR_ARG beyond (split with ps_points_slice / ps_scalars_slice and add the parts with ps_points_sum).
 * Ordering: arrays returned by the asynchronous producers (ps_points_from_scalars,
 * ps_scalars_from_device_be32) may be passed on at once -- every sum waits for its own inputs. */
int ps_msm(ps_ctx* ctx, const ps_points* points, const ps_scalars* scalars, uint8_t* out);
/* Host-buffer convenience forms (upload + ps_msm). */
int ps_msm_be32(ps_ctx* ctx, const ps_points* points, const uint8_t* scalars_be32, size_t n, uint8_t* out);
int ps_msm_i64(ps_ctx* ctx, const ps_points* points, const int64_t* scalars, size_t n, uint8_t* out);
/* Asynchronous form: ps_msm_launch enqueues the sum and leaves the per-window sums on the device;
 * ps_msm_finish() waits for the OLDEST pending sum and folds it on the host.  Up to PS_MSM_QUEUE sums
 * may be pending on a context (PS_ERR_ARG beyond that): each runs on its own internal stream and
 * workspace, the accumulations chained in launch order, so a caller that keeps the queue full
 * (launch i+3, then finish i) hides each sum's sort and its latency-bound tail -- bucket fix-up,
 * reduction, host fold -- under its neighbours' accumulations.  Four is the measured optimum for 2^20-point sums
 * (2.70 ms per sum with three pending, 2.63 with four, 2.9 with five or six: the tail of the oldest sum is starved by
 * the accumulations queued behind it).  The one-call forms (ps_msm, ps_msm_be32, ps_msm_i64, ps_msm_multi, the provers)
 * need an empty queue (PS_ERR_ARG otherwise). */
#ifndef PS_MSM_QUEUE
#define PS_MSM_QUEUE 4
#endif
int ps_msm_launch(ps_ctx* ctx, const ps_points* points, const ps_scalars* scalars);
int ps_msm_finish(ps_ctx* ctx, uint8_t* out);
/* k sums over ONE scalar vector: out[i] = sum_j scalars[j] * points[i][j].  The digit sort runs once and
 * is shared; the arrays may mix G1 and G2.  This is the shape of computeSolCommit called nine times on
 * solution[diff:] (pinochio.go:231-241).  k <= PS_MSM_MULTI_MAX; every array must have the scalars'
 * length (PS_ERR_LENGTH otherwise, algebra.go:350-352). */
#define PS_MSM_MULTI_MAX 16
int ps_msm_multi(ps_ctx* ctx, const ps_points* const* points, size_t k, const ps_scalars* scalars, uint8_t* const* out);
/* The dual: k scalar vectors over ONE point array, one sort / accumulation / tail over k * W bucket sets and a fold per
 * member on the device.
 * out[k] = sum_i scalars[k*n + i] * points[i],  n = ps_points_len(points),  ps_scalars_len(scalars) == k*n (PS_ERR_LENGTH
 * otherwise).  out: k * 96 (G1) / k * 192 (G2) bytes, the encoding ps_msm writes.  Byte-identical to k calls of ps_msm over
 * slices of `scalars`.  k == 0 or n == 0: PS_OK, identities.  (algebra.go:348-359, k times over one blindedPoint.)
 * A window table on `points` changes the route, never the bytes (ps_msm_batch_set_table); ps_msm_set_window is honoured and
 * means the plain plan with that window.  Needs an empty MSM queue (PS_ERR_ARG otherwise).  A batch too large for one pass
 * runs as several, invisibly; ps_msm_batch_set_chunk bounds the members of a pass (0 = automatic).  A batch of which not
 * even one member fits a pass is summed by ps_msm per member. */
int ps_msm_batch(ps_ctx* ctx, const ps_points* points, const ps_scalars* scalars, size_t k, uint8_t* out);
int ps_msm_batch_set_chunk(ps_ctx* ctx, int members /* sums per pass; 0 = automatic */);
/* Whether ps_msm_batch, ps_msm_batch_multi and the batch provers sum over the window tables of their points
 * (ps_points_precompute; the provers' cached keys): all windows of a member then share ONE bucket set -- a pass has k sets
 * instead of k * W, wider windows, fewer digits, and the set sum is the member's result with no fold behind it.
 *   0  automatic (the default): every array of the call carries a usable table of one window size (a table whose windows
 *      cover the scalars, no forced window, n < 2^26), a member has at least 512 points, and the plain plan is not cheaper by
 *      the margin ps_msm applies (an int64 witness over a 20-bit table stays plain)
 *   1  never: the plain pass, k * W bucket sets and a fold per member
 *   2  wherever the tables are usable and one member fits a pass (tests, A/B runs)
 * The bytes are the same on every route.  ps_msm_last_info reports window_table = 1, the table's window_bits and windows, and
 * buckets = (members of the last pass) * 2^(window_bits - 1) after a tabled pass.  Another mode: PS_ERR_ARG.
 * Added within revision 5 (found by symbol, no existing struct changed). */
int ps_msm_batch_set_table(ps_ctx* ctx, int mode);
/* The product of the two: k scalar vectors over `a` point arrays, ONE digit sort per pass shared by all arrays (as in
 * ps_msm_multi) and one bucket problem of k * W bucket sets per array (as in ps_msm_batch).
 * out[i][j] = sum_{t<n} scalars[j*stride + first + t] * points[i][t],  i < a, j < k,  n = the common length of the arrays.
 * out[i]: k * 96 (G1) / k * 192 (G2) bytes.  Arrays may mix groups.  Entry (i, j) is byte-identical to ps_msm over points[i]
 * and the slice [j*stride + first, +n) of `scalars`; with a == 1, stride == n, first == 0 the call is ps_msm_batch.  This is
 * the shape of computeSolCommit on solution[diff:] (pinochio.go:222-241) for k solutions stored back to back: stride = the
 * number of variables, first = diff.  Scalars outside the members' ranges -- the IO part of a witness, the gaps between
 * members -- are never read.
 * a <= PS_MSM_MULTI_MAX; a NULL array or a NULL out[i] is PS_ERR_ARG.  Arrays of different lengths: PS_ERR_LENGTH
 * (algebra.go:350-352); so are first + n > stride and ps_scalars_len(scalars) != k*stride.  a == 0 or k == 0: PS_OK;
 * n == 0: PS_OK, identities.  Needs an empty MSM queue (PS_ERR_ARG otherwise).  Window tables are summed over when every
 * array carries a usable one of the same window size (ps_msm_batch_set_table); ps_msm_set_window, ps_msm_set_slice,
 * ps_msm_set_tail and ps_msm_batch_set_chunk are honoured as in ps_msm_batch, and a batch of which not even one member fits
 * a pass is summed by ps_msm per (array, member).
 * Each array's point pass, fold and encoding run on a workspace of their own (four rotate), so the folds of different arrays
 * -- serial chains of ~250 doublings each -- run side by side; every workspace is idle again when the call returns, on every
 * path.  Added within revision 5 (found by symbol, no existing struct changed). */
int ps_msm_batch_multi(ps_ctx* ctx, const ps_points* const* points, size_t a, const ps_scalars* scalars, size_t k,
                       size_t stride, size_t first, uint8_t* const* out);
/* Host-side conversion of ONE point between PS_FMT_AFFINE and PS_FMT_COMPRESSED (what the shim
 * needs to feed proof elements back to kyber's UnmarshalBinary).  Validates the encoding. */
int ps_point_convert(int group, int in_fmt, int out_fmt, const uint8_t* in, uint8_t* out);
/* Sum of k affine points (the per-GPU partial sums of a sharded MSM, after the RCCL gather). */
int ps_points_sum(int group, const uint8_t* pts, size_t k, uint8_t* out);
/* sum_i scalars[i] * points[i] for a handful of points (k <= 64) on the host: the fixed-point terms of a proof
 * (r Delta + Alpha ...) and the weighting of partial sums computed elsewhere.  Affine in, affine out. */
int ps_points_lincomb(int group, const uint8_t* pts, const uint8_t* scalars_be32, size_t k, uint8_t* out);
/* One sum over index-range shards held by several devices of THIS process: shard d is summed on ctxs[d] (the devices
 * work side by side), the partial sums are folded on the host.  The in-process form of the sharded MSM of SURVEY 8e
 * (a cgo caller cannot wrap a function call in one process per GPU). */
int ps_msm_multi_device(ps_ctx* const* ctxs, const ps_points* const* pts, const ps_scalars* const* scalars, size_t ndev, uint8_t* out);
/* Tuning / introspection of the last MSM on this context. */
typedef struct {
    int window_bits;   /* c */
    int windows;       /* W */
    uint64_t entries;  /* non-zero digits = bucket additions issued */
    uint64_t buckets;  /* W * 2^(c-1) */
    int slice;         /* sorted entries per accumulation thread */
    int window_table;  /* 1: the sum ran over the array's window table (ps_points_precompute), 0: the plain plan */
} ps_msm_info;
int ps_msm_last_info(ps_ctx* ctx, ps_msm_info* out);
int ps_msm_set_window(ps_ctx* ctx, int window_bits /* 0 = automatic, else 4..20 */);
int ps_msm_set_slice(ps_ctx* ctx, int entries /* sorted entries per accumulation thread; 0 = automatic */);
/* The tail of a sum (fix-up of cut buckets, bucket reduction): 0 = automatic (short sums -- fewer than 2^21 digits --
 * take shallow trees of lane-cooperative point additions, long ones the work-efficient chains), 1 = chains, 2 = trees.
 * Same group element, same bytes, either way (A/B runs and tests). */
int ps_msm_set_tail(ps_ctx* ctx, int mode);
/* The point pass of a sum: 1 = fixed slices of the sorted entry list (cut buckets are mended by the fix-up kernels),
 * 2 = whole buckets, one lane each, taken in order of size (no partial sums, no fix-up; correct for every input, slow when
 * a few buckets hold most of the entries), 0 = automatic: slices, unless the sum is long, its scalars are wider than an
 * int64 witness's, it has at least 2^18 buckets of at most 64 entries on average AND the sort finds them evenly filled -- that
 * last part is decided on the device, without a host wait, and ps_msm_last_accumulate reports what the sum finished last
 * took (1 or 2; 0 before the first sum).
 * ps_msm_batch always takes slices.  Same group element, same bytes, either way.  Added within revision 5 (found by
 * symbol, no existing struct changed). */
int ps_msm_set_accumulate(ps_ctx* ctx, int mode);
int ps_msm_last_accumulate(ps_ctx* ctx, int* path);
/* In the automatic mode a sum does not enqueue both point passes every time: the context remembers, per kind of sum (the
 * array and its table, the length, the window, the width of the scalars, the number of arrays over one sort), which pass the
 * device chose last and launches only that one -- ps_msm_launch / ps_msm_finish, ps_msm, ps_msm_be32, ps_msm_i64,
 * ps_msm_multi and the provers' sums.  The device still decides: when it chooses the other pass -- the distribution of the
 * scalars changed -- the call that returns the result (ps_msm_finish, ps_msm_multi, the prover) runs the point pass a second
 * time first, so SUCH A SUM IS SUMMED TWICE (about one lone point pass of extra latency), and the next four sums of that
 * kind enqueue both passes again.  Results and ps_msm_last_accumulate never depend on the guess.  ps_msm_batch keeps the slices.
 * ps_msm_prediction_counts: out[0] admitted sums of this context launched with both passes, out[1] with one, out[2] how
 * many of the latter were summed twice.  The sums over one sort (ps_msm_multi) share one verdict and count as one.  Sums
 * that are not admitted, and forced modes, count nowhere.  Added within revision 5 (found by symbol, no existing struct
 * changed). */
int ps_msm_prediction_counts(ps_ctx* ctx, uint64_t* out /* [3] */);
/* Per-stage device time of the sum finished last, measured with HIP events on the streams its kernels
 * run on.  Stages: 0 digits (+counter memset), 1 scan, 2 scatter (+ the buckets' order by size where whole buckets are
 * considered, ps_msm_set_accumulate), 3 queue (bucket memset, and with
 * several sums in flight the wait for the previous sum's accumulation), 4 accumulate (the dominant
 * kernel, bracketed tightly), 5 fix-up, 6 bucket reduction. */
/* Measured issue rate of v_mad_u64_u32 (lane-operations per second, two waves per SIMD on every CU; ~1 ms): the
 * integer roofline the bucket additions are priced against, measured on the chip and at the clocks of the run. */
int ps_microbench_mad(ps_ctx* ctx, double* lane_mads_per_s);
#define PS_MSM_STAGES 7
int ps_ctx_set_timing(ps_ctx* ctx, int enable);
int ps_msm_last_stage_ms(ps_ctx* ctx, float ms[PS_MSM_STAGES]);

/* ---- QAP quotient: QAP.Quotient (qap.go:151-162) + computeAggregatePoly (qap.go:164-175) ----
 * The R1CS matrices (r1cs.go:78-101: rows = gates, columns = variables) are given in CSR, with
 * int64 coefficients (the reference's Value = int, algebra.go:11; ps_csr) or with field elements
 * (ps_csr_fr, below).  The QAP domain is the
 * reference's {1..n} (qap.go:42-55, algebra.go:256-258). */
typedef struct {
    const uint32_t* row_ptr; /* n+1 */
    const uint32_t* col;     /* nnz */
    const int64_t* val;      /* nnz */
} ps_csr;
int ps_qap_create(ps_ctx* ctx, size_t n_gates, size_t n_vars, size_t n_io, const ps_csr* L, const ps_csr* R,
                  const ps_csr* O, ps_qap** out);
void ps_qap_free(ps_qap* q);
/* The same, with coefficients that are field elements -- a hash's round constants, MDS entries, weights 2^k for k >= 64, or
 * r - 1 written out instead of -1: 32-byte canonical big-endian values, the format of ps_scalars_upload.  Checks, codes and
 * texts are ps_qap_create's; in addition a coefficient not below r is PS_ERR_ENCODING.  An explicit zero is allowed.  Both
 * entries make the same ps_qap from the same circuit: every result is the same bytes.  Added within revision 5 (found by
 * symbol). */
typedef struct {
    const uint32_t* row_ptr; /* n+1 */
    const uint32_t* col;     /* nnz */
    const uint8_t* val_be32; /* nnz x 32 B */
} ps_csr_fr;
int ps_qap_create_fr(ps_ctx* ctx, size_t n_gates, size_t n_vars, size_t n_io, const ps_csr_fr* L, const ps_csr_fr* R,
                     const ps_csr_fr* O, ps_qap** out);
/* out[0..2]: the entries of L, R, O that are WIDE.  A canonical value v counts with the signed magnitude min(v, r - v)
 * (negative above (r - 1) / 2), and is wide iff that magnitude is >= 2^64.  Always 0 for a ps_qap made by ps_qap_create.
 * Only ps_qap_column_sums depends on it. */
int ps_qap_wide_entries(const ps_qap* q, size_t out[3]);
/* sol: n_vars scalars.  Outputs (any may be NULL): A, B, C aggregate polynomials (n coefficients
 * each) and h (n-1 coefficients), all device-resident.  PS_ERR_NOT_DIVISIBLE <=> "apocalypse". */
int ps_qap_quotient(ps_ctx* ctx, const ps_qap* q, const ps_scalars* sol, ps_scalars** A, ps_scalars** B,
                    ps_scalars** C, ps_scalars** h);
/* (*QAP).IsValid (qap.go:107-148): *valid = 1 iff left(x) right(x) - out(x) is divisible by z(x), i.e. iff the solution
 * satisfies every gate.  PS_ERR_ARG <=> sanityCheck's panic (qap.go:177-189). */
int ps_qap_is_valid(ps_ctx* ctx, const ps_qap* q, const ps_scalars* sol, int* valid);

/* computeAggregatePoly (qap.go:164-175) for ONE of the three polynomials: which = 0 left (A), 1 right (B), 2 out (C);
 * n coefficients.  No divisibility test (that needs all three: ps_qap_quotient).  The three parts of the quotient --
 * A, B and h through the h-only route -- are independent, so three GPUs can compute them side by side. */
int ps_qap_interpolate(ps_ctx* ctx, const ps_qap* q, const ps_scalars* sol, int which, ps_scalars** out);

/* Poly.Mul (algebra.go:92-105): out = a * b, len(a)+len(b)-1 coefficients (NTT product). */
int ps_poly_mul(ps_ctx* ctx, const ps_scalars* a, const ps_scalars* b, ps_scalars** out);

/* ---- whole-function drivers ---- */
typedef struct { /* the prover's part of Groth16Setup (groth16.go:30-61) */
    uint8_t alpha[96], beta[96], delta[96]; /* G1 */
    uint8_t beta2[192], delta2[192];        /* G2 */
    const ps_points* xi;                    /* n   G1 */
    const ps_points* xi2;                   /* n   G2 (declared []G1 at groth16.go:60) */
    const ps_points* nio_lp;                /* n_vars - (n_vars - n_io) ... see `diff` note */
    const ps_points* xi_t;                  /* n-1 G1 */
    /* Optional (NULL = absent): the same CRS in LAGRANGE form, as ps_groth16_setup also emits it --
     *   lxi[j-1]  = l_j(x) G1,  lxi2[j-1] = l_j(x) G2         l_j the Lagrange basis of the QAP domain {1..n} (qap.go:42-55)
     *   lxi_t[k-1] = lambda_k(x) t(x)/delta G1                 lambda_k the Lagrange basis of the nodes n+1..2n-1
     * With all three present the prover needs no polynomial in coefficient form: A(x) G = sum_j (L.s)_j lxi_j, likewise B,
     * and h(x) t(x)/delta G = sum_k h(n+k) lxi_t_k -- the interpolations and the division of the quotient (three quarters of
     * it) disappear, the proof is the same group elements.  A key made by the reference's NewGroth16TrustedSetup has only
     * the monomial arrays above; then the coefficients are computed as QAP.Quotient does. */
    const ps_points* lxi;                   /* n   G1 */
    const ps_points* lxi2;                  /* n   G2 */
    const ps_points* lxi_t;                 /* n-1 G1 */
} ps_groth16_pk;
/* Groth16Prove (groth16.go:122-211).  r, s are inputs (the reference draws them at :148,:158 and
 * keeps them in the proof, :203-206).  diff = n_vars - n_io is used as the first non-IO index
 * exactly as the reference does (groth16.go:175-177).
 * Internal forms, all giving the same group elements: C as one sum with the scalars s a_j + r b_j, or -- Lagrange-form keys
 * of >= 2^19 constraints -- B in G1 as a sum of its own over the wire values and s A + r B1 added on the host (DESIGN.md
 * section 5; PS_G16_B1_MIN_N in the environment of ps_ctx_create moves that threshold: a knob for tests and measurements). */
int ps_groth16_prove(ps_ctx* ctx, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol,
                     const uint8_t r_be32[32], const uint8_t s_be32[32], uint8_t A[96], uint8_t B[192],
                     uint8_t C[96]);

/* k proofs under one key: sols holds k solution vectors of q's m variables back to back; r_be32 / s_be32 k*32 bytes; A, C
 * k*96, B k*192.  Proof j is byte-identical to ps_groth16_prove(ctx, pk, q, sols[j*m .. (j+1)*m), r_j, s_j, ..).
 * (groth16.go:122-211, k times.)  One pass of wire values and gate checks over all witnesses, the h values witness by
 * witness without a host synchronisation between them, then three ps_msm_batch sums.
 * Needs a Lagrange-form key (lxi, lxi2, lxi_t): PS_ERR_ARG otherwise, naming ps_points_monomial_to_lagrange.
 * valid == NULL: a witness that violates a gate fails the call with PS_ERR_NOT_DIVISIBLE ("apocalypse", qap.go:158-160; the
 * message names the first such index).  valid != NULL: PS_OK, valid[j] = 0 and the 384 bytes of proof j are zero, every
 * other proof as above.  k == 0: PS_OK.  Needs an empty MSM queue; ps_msm_batch_set_chunk bounds the members per pass.
 * Measured against a loop of ps_groth16_prove on the same key (profiles/prove_batch.txt): a call costs ~13 ms whatever k is (each
 * of the three sums ends in a serial fold of ~250 doublings per member, 3.3-3.9 ms), so the batch is slower than the loop
 * below ~32 proofs (k = 1: 0.06-0.14x, k = 8: 0.35-0.54x) and wins beyond: 1.9x at 2^10 constraints and k = 64, 3.0x at
 * k = 256, 2.0-2.2x at 2^12.  At 2^14 constraints it only draws level (0.97x at 64, 1.15x at 256) and at 2^16 it loses at
 * every k measured (0.55x): there the single prover's window tables and its three sums in flight are worth more. */
int ps_groth16_prove_batch(ps_ctx* ctx, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sols, size_t k,
                           const uint8_t* r_be32, const uint8_t* s_be32, uint8_t* A, uint8_t* B, uint8_t* C, int* valid);

/* One rank's share of Groth16Prove when the sums are sharded over `world` GPUs (one process each): rank g
 * takes its index range of every CRS array, the LAST rank also the fixed points; A_part / B_part / C_part of all
 * ranks add up (ps_points_sum, after an all_gather) to the A, B, C of ps_groth16_prove.  Every rank
 * computes the quotient itself (beside its sums: the quotient runs on a stream of its own). */
int ps_groth16_prove_shard(ps_ctx* ctx, const ps_groth16_pk* pk, const ps_qap* q, const ps_scalars* sol,
                           const uint8_t r_be32[32], const uint8_t s_be32[32], int rank, int world, uint8_t A_part[96],
                           uint8_t B_part[192], uint8_t C_part[96]);

/* Groth16Prove over the devices of one process, every device holding only ITS index range of the CRS arrays: device d
 * of ndev holds Xi[range(n)], Xi2[range(n)], NioLP[range(nbIO)], XiT[range(n-1)] with range = the d-th of ndev
 * contiguous parts whose sizes differ by at most one (PS_ERR_LENGTH, naming the device, otherwise); the fixed points are
 * read from dev[0].pk.  Each device has its own context, its own ps_qap of the circuit and its own copy of the solution;
 * 1 <= ndev <= 64.  Same proof bytes as ps_groth16_prove.
 *
 * The optional arrays of dev[d].pk select the route, as in ps_groth16_prove:
 *   - lxi[range(n)], lxi2[range(n)], lxi_t[range(n-1)] on EVERY device (xi / xi2 / xi_t may then be NULL, and are not read):
 *     the route without coefficient vectors.  The scalars of A, B and of B in G1 are the wire values of the device's OWN rows
 *     of L.s and R.s -- computed, gate-checked and converted by one kernel on that device, no exchange at all; the four sums
 *     that need no h start at once.  Only the values h(n+k) depend on the whole circuit: their three convolutions run on
 *     devices 0, 1, 2 side by side (one each; ndev < 3: all on dev[0]), and every device copies its ranges of the three
 *     results device to device -- 3 x 40 bytes per node of its range -- and finishes h there.  Nothing of A, B or h crosses
 *     host memory, nothing is allocated once the contexts are warm.  The contexts must be distinct (PS_ERR_ARG).  The
 *     divisibility test is the union of the devices' own-row checks: PS_ERR_NOT_DIVISIBLE from any of them fails the call,
 *     and every device has drained what it launched when the call returns.  ps_prove_last_phase_ms on each context gives
 *     that device's share.  PS_G16_MULTI_HSPLIT=0 in the environment of ps_ctx_create (read from dev[0].ctx; default 1) keeps
 *     the three convolutions on dev[0] whatever ndev is: a knob for tests and measurements, as PS_G16_B1_MIN_N is.
 *   - on some devices but not on all: PS_ERR_ARG.
 *   - on none: the monomial arrays are required; with three or more devices the parts of the quotient (A, B, h) are
 *     computed side by side on devices 0, 1, 2 and cross through host memory. */
typedef struct {
    ps_ctx* ctx;
    const ps_qap* qap;
    const ps_scalars* sol;
    ps_groth16_pk pk; /* rank-local arrays */
} ps_groth16_device;
int ps_groth16_prove_multi(const ps_groth16_device* dev, size_t ndev, const uint8_t r_be32[32], const uint8_t s_be32[32],
                           uint8_t A[96], uint8_t B[192], uint8_t C[96]);

/* One rank's share of Groth16Prove when the rank holds ONLY its index ranges of a Lagrange-form key (one process per GPU):
 * pk_local has lxi[range(n)], lxi2[range(n)], lxi_t[range(n-1)], nio_lp[range(nbIO)] for (rank, world) -- PS_ERR_LENGTH
 * otherwise; a key without all three L-arrays is PS_ERR_ARG (xi / xi2 / xi_t are not read) -- and the fixed points, which
 * the LAST rank adds.  The share of ps_groth16_prove_multi's Lagrange route, with the values of h computed on this device
 * (processes cannot copy peer to peer, and 2 ms replicated beats three broadcasts); the gate check covers all rows, so every
 * rank reports an unsatisfied witness.  The element-wise ps_points_sum of all ranks' parts is the proof of
 * ps_groth16_prove, byte for byte. */
int ps_groth16_prove_local(ps_ctx* ctx, const ps_groth16_pk* pk_local, const ps_qap* q, const ps_scalars* sol,
                           const uint8_t r_be32[32], const uint8_t s_be32[32], int rank, int world, uint8_t A_part[96],
                           uint8_t B_part[192], uint8_t C_part[96]);

typedef struct { /* PHGR13EvalKey (pinochio.go:37-62); ws is G2, every other array is G1 */
    const ps_points *vs, *ws, *ys, *vas, *was, *yas, *gsi, *vbs, *wbs, *ybs;
    /* Optional (NULL = absent): lgsi[k-1] = lambda_k(s) G1, the Lagrange form of gsi on the nodes n+1..2n-1 (n-1 points, as
     * ps_phgr13_setup emits it): hs = sum_k h(n+k) lgsi_k without interpolating h. */
    const ps_points* lgsi;
} ps_phgr13_ek;
typedef struct { /* PHGR13Proof (pinochio.go:180-203) */
    uint8_t vss[96], vass[96], wss[192], wass[96], yss[96], yass[96], hs[96], gz[96];
} ps_phgr13_proof;
/* PHGR13Prove (pinochio.go:207-254). */
int ps_phgr13_prove(ps_ctx* ctx, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sol,
                    ps_phgr13_proof* out);

/* k proofs under one evaluation key: sols holds k solution vectors of q's m variables back to back; out: k proofs.
 * Proof j is byte-identical to ps_phgr13_prove(ctx, ek, q, sols[j*m .. (j+1)*m), &out[j]).  (pinochio.go:207-254, k times.)
 * One pass of wire values and gate checks over all witnesses, the h values witness by witness without a host
 * synchronisation between them, hs as one ps_msm_batch over lgsi, and the other seven elements as ONE ps_msm_batch_multi
 * over vs, ws, ys, vas, was, yas and the pointwise sum of the three beta arrays, reading solution[diff:] of every witness in
 * place.
 * Needs lgsi in the key: PS_ERR_ARG otherwise, naming ps_points_monomial_to_lagrange.  The nine solution arrays must have one
 * length nn with diff + nn <= m, and gsi / lgsi n - 1 points (PS_ERR_LENGTH otherwise); ps_scalars_len(sols) == k*m and
 * n >= 2 (PS_ERR_ARG); k*m and k*(n-1) below 2^31 (PS_ERR_ARG: split the batch).
 * valid == NULL: a witness that violates a gate fails the call with PS_ERR_NOT_DIVISIBLE ("apocalypse", qap.go:158-160; the
 * message names the first such index).  valid != NULL: PS_OK, valid[j] = 0 and all 864 bytes of proof j are zero, every
 * other proof as above.  k == 0: PS_OK.  Needs an empty MSM queue; ps_msm_batch_set_chunk bounds the members per pass.
 * ps_prove_last_phase_ms: [0] wire values, gate check and h values, [1] the h sum, [2] the solution sums, [3] total.
 * Added within revision 5 (found by symbol, no existing struct changed). */
int ps_phgr13_prove_batch(ps_ctx* ctx, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sols, size_t k,
                          ps_phgr13_proof* out, int* valid);

/* One rank's share of PHGR13Prove when the sums are sharded over `world` GPUs (one process each), the twin of
 * ps_groth16_prove_shard: every rank holds the WHOLE key and computes the quotient itself; rank g sums its index range of
 * every array -- range(len(vs)) of the nine solution arrays (one digit sort), range(n-1) of gsi, or of lgsi when the key has
 * it.  PHGR13 has no fixed points: `part` holds partial sums only (the identity for an empty range), and the element-wise
 * ps_points_sum of all ranks' parts is the proof of ps_phgr13_prove, byte for byte.  The nine arrays must have one length
 * (as ps_phgr13_setup / NewPHGR13TrustedSetup make them; PS_ERR_LENGTH otherwise). */
int ps_phgr13_prove_shard(ps_ctx* ctx, const ps_phgr13_ek* ek, const ps_qap* q, const ps_scalars* sol, int rank, int world,
                          ps_phgr13_proof* part);

/* PHGR13Prove over the devices of one process, every device holding only ITS index ranges of the evaluation key: device d
 * of ndev holds vs .. ybs[range(nn)] (nn = len(vs) of the whole key) and gsi[range(n-1)], and lgsi[range(n-1)] if the key
 * has the Lagrange form -- on every device or on none (PS_ERR_ARG); range = the d-th of ndev contiguous parts whose sizes
 * differ by at most one (PS_ERR_LENGTH, naming the device, otherwise).  Each device has its own context (distinct), its own
 * ps_qap of the circuit and its own copy of the solution; 1 <= ndev <= 64.  The quotient runs once, on dev[0]; every
 * other device starts its solution sums at once and copies its range of h device to device when h exists.  Same proof
 * bytes as ps_phgr13_prove.  ps_prove_last_phase_ms on each context gives that device's share. */
typedef struct {
    ps_ctx* ctx;
    const ps_qap* qap;
    const ps_scalars* sol;
    ps_phgr13_ek ek; /* rank-local arrays */
} ps_phgr13_device;
int ps_phgr13_prove_multi(const ps_phgr13_device* dev, size_t ndev, ps_phgr13_proof* out);

/* Host wall-clock split of the last ps_groth16_prove / ps_phgr13_prove on this context, in ms:
 * [0] quotient h(x) (SpMV, gate check, interpolations, division), [1] scalar preparation (Groth16) or
 * the h(s) sum (PHGR13), [2] the remaining sums incl. host folds, [3] total.  For reports only.
 * ps_phgr13_prove_shard / ps_phgr13_prove_multi set it for the context's own share: [0] computing h -- or, on a device of
 * ps_phgr13_prove_multi other than dev[0], waiting for h including the copy of its range --, [1] the h(s) sum, [2] the
 * solution sums (what is left of them after [1]), [3] total.
 * ps_groth16_prove_local, and ps_groth16_prove_multi over Lagrange-form local keys, likewise for the context's share: [0] the
 * own rows (and whatever of the values route ran on this device) plus the wait for h, [1] the h sum, [2] the other sums and
 * the host's weighting, [3] total. */
#define PS_PROVE_PHASES 4
int ps_prove_last_phase_ms(ps_ctx* ctx, float ms[PS_PROVE_PHASES]);

/* ---- trusted setup on the device ---- */
typedef struct { uint8_t alpha[32], beta[32], delta[32], x[32], gamma[32]; } ps_groth16_toxic; /* groth16.go:15-26 */
typedef struct { /* type Groth16Setup (groth16.go:30-61) without the toxic waste */
    uint8_t alpha[96], beta[96], delta[96];        /* G1 */
    uint8_t beta2[192], delta2[192], gamma[192];   /* G2 */
    ps_points *xi, *xi2, *io_lp, *nio_lp, *xi_t;    /* caller frees with ps_points_free */
    ps_points *lxi, *lxi2, *lxi_t;                  /* the Lagrange form (see ps_groth16_pk); caller frees */
} ps_groth16_crs;
/* NewGroth16TrustedSetup (groth16.go:64-101) with the toxic waste supplied by the caller. */
int ps_groth16_setup(ps_ctx* ctx, const ps_qap* q, const ps_groth16_toxic* tw, ps_groth16_crs* out);

typedef struct { uint8_t s[32], av[32], aw[32], ay[32], rv[32], rw[32], beta[32], gamma[32]; } ps_phgr13_toxic; /* draw order of pinochio.go:99-138 */
typedef struct { /* PHGR13Setup (pinochio.go:28-35) without the toxic waste */
    ps_points *gsi, *vs, *ws, *ys, *vas, *was, *yas, *vbs, *wbs, *ybs;                  /* PHGR13EvalKey, pinochio.go:37-62 */
    uint8_t av[192], aw[96], ay[192], gamma[192], bgamma[96], bgamma2[192], yts[192]; /* PHGR13VerifKey, pinochio.go:64-91 */
    ps_points *vk_vs, *vk_ws, *vk_ys; /* vk.vs, vk.ws (G2), vk.ys over ALL variables; vs/ws/ys above are their [diff:] views */
    ps_points* lgsi;                  /* the Lagrange form of gsi (see ps_phgr13_ek) */
} ps_phgr13_crs;
/* NewPHGR13TrustedSetup (pinochio.go:93-176) with the toxic waste supplied by the caller. */
int ps_phgr13_setup(ps_ctx* ctx, const ps_qap* q, const ps_phgr13_toxic* tw, ps_phgr13_crs* out);
void ps_phgr13_crs_free(ps_phgr13_crs* crs); /* frees the 14 arrays */

/* ---- a reference-made key onto the fast route, without the toxic waste ----
 * The reference's setups emit the monomial arrays only -- Xi, Xi2, XiT (groth16.go:79-97), gsi (pinochio.go:101) -- and a prover
 * given those interpolates and divides (28 ms per Groth16 proof at 2^20 constraints where the Lagrange form of the same key
 * takes 18).  ps_groth16_setup emits both forms but needs the toxic waste, which "must be delete[d] after a trusted setup"
 * (groth16.go:13-14).  This is the one-time conversion of an array {x^i P}, i < cnt, into {l_j(x) P}, j < cnt, over the
 * group elements alone (the transposed interpolation of csrc/lagrange.hpp: ~230 cnt scalar multiplications of points; seconds
 * at 2^16 gates, under a minute at 2^20).  nodes = 0: the QAP domain 1..n, cnt = n (Xi -> lxi, Xi2 -> lxi2);
 * nodes = 1: the nodes n+1..2n-1, cnt = n-1 (XiT -> lxi_t, gsi -> lgsi).  Either group.  The result is byte-identical to the
 * array ps_groth16_setup / ps_phgr13_setup emit from the toxic waste; the caller frees it.  PS_ERR_LENGTH when the array is
 * not exactly cnt points long.  The points must lie in the subgroup of order r, as the points of a key do (the scalar
 * multiplications split their scalars with the curve's endomorphism, which acts as a scalar only there). */
int ps_points_monomial_to_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_points* mono, int nodes, ps_points** out);

/* ---- a circuit's key from a powers-of-tau string, without the toxic waste ----
 * NewGroth16TrustedSetup (groth16.go:64-101) computes every key element from alpha, beta, delta, x, gamma in the clear, values
 * that "must be delete[d] after a trusted setup" (groth16.go:13-14).  A deployment instead starts from a universal string
 * {x^i G} that no single party knows (phase 1), derives the circuit's key from it with delta = gamma = 1, and lets every party
 * fold a delta / gamma share of its own into that key (phase 2); anybody can check a fold.  Entry points added within
 * revision 5 (found by symbol, no existing struct changed).
 *
 * Column sums of an R1CS matrix over points: out[i] = sum_j M[j][i] p[j], i < n_vars; M = L, R, O for which = 0, 1, 2; p has
 * n_gates points (PS_ERR_LENGTH otherwise), either group.  The per-variable sums of fullLinearPoly (groth16.go:254-264) when
 * only {l_j(x) G} is known, not x: the sparse matrix applied to a vector of points.  A coefficient enters as the signed
 * magnitude min(v, r - v), and a column costs one doubling per bit of its own largest magnitude plus one addition per set
 * coefficient bit: at most 64 doublings while the matrix has no wide entry (ps_qap_wide_entries; every ps_csr matrix), at
 * most 254 for a column that holds one, and additions only for a column of +-1 in either case.  Identity points, repeated
 * points and terms that cancel are handled; a variable that occurs in no gate gives the identity.  Canonical affine output (the bytes ps_points_from_scalars gives for the same group element); caller frees. */
int ps_qap_column_sums(ps_ctx* ctx, const ps_qap* q, int which, const ps_points* p, ps_points** out);

typedef struct {                   /* phase-1 output, the layout public ceremonies publish; n = n_gates */
    const ps_points* tau_g1;       /* x^i G1,        i < 2n-1 */
    const ps_points* tau_g2;       /* x^i G2,        i < n    */
    const ps_points* alpha_tau_g1; /* alpha x^i G1,  i < n    */
    const ps_points* beta_tau_g1;  /* beta  x^i G1,  i < n    */
    uint8_t beta_g2[192];          /* beta G2                 */
} ps_groth16_srs;
/* The key of ps_groth16_setup for the same alpha, beta, x and delta = gamma = 1, byte for byte, from the string alone:
 * alpha, beta = the first points of the scaled arrays, beta2 copied, delta = G1, delta2 = gamma = G2; xi, xi2 = the first n
 * powers, lxi / lxi2 their ps_points_monomial_to_lagrange; io_lp | nio_lp = ps_qap_column_sums of L over the Lagrange form of
 * beta_tau_g1, plus R over that of alpha_tau_g1, plus O over lxi, split at diff = n_vars - n_io; xi_t[i] = sum_k z_k tau_g1[i+k]
 * with z = prod_{j=1..n} (X - j) (one NTT over points: the correlation of lagrange.hpp); lxi_t its conversion on the nodes
 * n+1..2n-1.  Five conversions dominate the cost (seconds each at 2^16 gates).  An array of another length than the comment
 * above says: PS_ERR_LENGTH; n < 2: PS_ERR_ARG.  `out` is overwritten; the caller frees its eight arrays with ps_points_free.
 * The caller is responsible for the string being well formed and for its points lying in the subgroup of order r --
 * ps_groth16_srs_check (below) tests both: the scalar multiplications split their scalars with the curve's endomorphism, which
 * acts as a scalar only there. */
int ps_groth16_setup_from_srs(ps_ctx* ctx, const ps_qap* q, const ps_groth16_srs* srs, ps_groth16_crs* out);
/* out = in with delta *= d and gamma *= g: nio_lp, xi_t and lxi_t scaled by 1/d, io_lp by 1/g (groth16.go:86-97), delta and
 * delta2 by d, gamma by g -- the key ps_groth16_setup makes for (delta d, gamma g), byte for byte.  d or g zero (mod r):
 * PS_ERR_ARG.  The drawing of d and g, and their deletion, are the caller's.  out != in.  The four scaled arrays of `out` are
 * new; its xi, xi2, lxi, lxi2 are views of in's storage (ps_points_slice: reference counted), so BOTH keys are freed as
 * usual, each of its eight handles with ps_points_free, in either order. */
int ps_groth16_crs_contribute(ps_ctx* ctx, const ps_groth16_crs* in, const uint8_t d_be32[32], const uint8_t g_be32[32],
                              ps_groth16_crs* out);
/* *ok = 1 iff `after` is `before` with SOME (d, g) folded in -- one fold or several:
 *   e(delta', G2) = e(G1, delta2');   e(sum rho_i N'_i, delta2') = e(sum rho_i N_i, delta2) for N = nio_lp, xi_t, lxi_t;
 *   e(sum rho_i I'_i, gamma') = e(sum rho_i I_i, gamma) for io_lp;   alpha, beta, beta2, xi, xi2, lxi, lxi2 byte-equal.
 * rho: nrho weights of 32 B, canonical (PS_ERR_ENCODING), drawn by the caller AFTER both keys are fixed, as for
 * ps_groth16_verify_batch (128 random bits each are enough); nrho at least the longest scaled array (PS_ERR_LENGTH).  A key
 * that was not made by a fold passes with probability <= 2^-bits(rho) per array.  Arrays of different lengths: *ok = 0.
 * The fixed points are tested for the subgroup; the arrays of an untrusted `after` go through ps_points_check_subgroup
 * first.  Needs an empty MSM queue. */
int ps_groth16_crs_check_update(ps_ctx* ctx, const ps_groth16_crs* before, const ps_groth16_crs* after, const uint8_t* rho_be32,
                                size_t nrho, int* ok);

/* ---- phase 1: making and checking the powers-of-tau string itself ----
 * The string ps_groth16_setup_from_srs starts from is the work of a ceremony: it begins as the trivial string (tau = alpha =
 * beta = 1: every point a generator), every party folds a share (t, a, b) of its own into it and publishes (t G2, a G2, b G2),
 * and anybody checks every fold.  Nobody knows tau, alpha, beta of the result unless ALL parties collude.  Entry points added
 * within revision 5 (found by symbol, no existing struct changed).
 *
 * out[i] = c s^i, i < n (s^0 = 1 also for s = 0): the exponents of a fold.  s or c not below r: PS_ERR_ENCODING; n = 0: an
 * empty vector; n >= 2^32: PS_ERR_ARG.  Caller frees. */
int ps_scalars_powers(ps_ctx* ctx, const uint8_t s_be32[32], const uint8_t c_be32[32], size_t n, ps_scalars** out);

typedef struct { uint8_t t_g2[192], a_g2[192], b_g2[192]; } ps_groth16_srs_share; /* t G2, a G2, b G2 */
/* out = in with tau *= t, alpha *= a, beta *= b:  tau_g1[i], tau_g2[i] scaled by t^i, alpha_tau_g1[i] by a t^i, beta_tau_g1[i] by
 * b t^i, beta_g2 by b; share = (t G2, a G2, b G2), the contributor's public values.  Canonical affine output: the bytes
 * ps_points_from_scalars gives for the same group elements.  Arrays of any lengths (a ceremony string is longer than any one
 * circuit needs; ps_points_slice cuts it); the four arrays of `out` are as long as in's, new, and freed by the caller with
 * ps_points_free.  out != in.  t, a or b zero (mod r): PS_ERR_ARG; not below r: PS_ERR_ENCODING.  The drawing of t, a and b, and
 * their deletion, are the caller's; so is the subgroup membership of in's points, as in ps_groth16_setup_from_srs. */
int ps_groth16_srs_contribute(ps_ctx* ctx, const ps_groth16_srs* in, const uint8_t t_be32[32], const uint8_t a_be32[32],
                              const uint8_t b_be32[32], ps_groth16_srs* out, ps_groth16_srs_share* share);
/* *ok = 1 iff the string is well formed -- {x^i G1}, {x^i G2}, {alpha x^i G1}, {beta x^i G1}, beta G2 for SOME non-zero x, alpha,
 * beta.  With T1, T2, A, B the four arrays of m1, m2, ma, mb points:
 *   T1[0] = G1, T2[0] = G2 (bytes);  T1[1], A[0], B[0], beta_g2 are not the identity;
 *   e(sum rho_i X[i], T2[1]) = e(sum rho_i X[i+1], G2), i < m - 1, for X = T1, A, B;
 *   e(T1[1], sum rho_i T2[i]) = e(G1, sum rho_i T2[i+1]), i < m2 - 1;     e(B[0], G2) = e(G1, beta_g2)
 * -- every point of every array is in a tested pair (i, i+1); each equation is a pairing product of its own.  m1, m2 >= 2,
 * ma, mb >= 1 (PS_ERR_ARG otherwise; an array of one point has no pair to test).  rho: nrho weights of 32 B, canonical
 * (PS_ERR_ENCODING), drawn by the caller AFTER the string is fixed (128 random bits each are enough), nrho >= max(m) - 1
 * (PS_ERR_LENGTH).  A string that is not well formed passes with probability <= 2^-bits(rho) per equation.  check_subgroup != 0:
 * the four arrays go through ps_points_check_subgroup and beta_g2 is tested likewise; a point outside the subgroup gives
 * *ok = 0 (0 only for a string the caller made itself).  A beta_g2 that is no canonical point on the curve: PS_ERR_ENCODING.
 * Needs an empty MSM queue. */
int ps_groth16_srs_check(ps_ctx* ctx, const ps_groth16_srs* srs, const uint8_t* rho_be32, size_t nrho, int check_subgroup, int* ok);
/* *ok = 1 iff `after` passes ps_groth16_srs_check with the subgroup tests on, each of its arrays is as long as before's, and
 *   e(after.T1[1], G2) = e(before.T1[1], share.t_g2);   e(after.A[0], G2) = e(before.A[0], share.a_g2);
 *   e(after.B[0], G2) = e(before.B[0], share.b_g2);     e(G1, after.beta_g2) = e(before.B[0], share.b_g2)
 * i.e. `after` is `before` with the (t, a, b) behind the share folded in.  `before` is taken as already checked.  The share is
 * untrusted: an encoding that is no canonical point on the curve is PS_ERR_ENCODING, the identity or a point outside the
 * subgroup gives *ok = 0.  rho as above.  A proof that the contributor KNOWS t, a and b (so that it could not derive its share
 * from earlier ones) belongs to the ceremony protocol and is not part of this call.  Needs an empty MSM queue. */
int ps_groth16_srs_check_update(ps_ctx* ctx, const ps_groth16_srs* before, const ps_groth16_srs* after, const ps_groth16_srs_share* share,
                                const uint8_t* rho_be32, size_t nrho, int* ok);

/* ---- the last link: is a key what its string makes of it? ----
 * Every other step of the chain -- ps_groth16_srs_contribute -> ps_groth16_srs_check / _check_update -> ps_groth16_setup_from_srs
 * -> ps_groth16_crs_contribute -> ps_groth16_crs_check_update -> prove -> verify -- has a cheap public check; that a circuit's key
 * IS what ps_groth16_setup_from_srs makes from this string could only be known by deriving it again (five conversions over group
 * elements) and comparing bytes.  But every key element is a fixed linear function of the string's points: a random linear
 * combination of a key array equals ONE sum over the monomial string, with coefficients from an interpolation over scalars.
 * Entry points added within revision 5 (found by symbol, no existing struct changed).
 *
 * *ok = 1 iff `lagr` is the Lagrange form of `mono` as ps_points_monomial_to_lagrange makes it (nodes = 0: the domain 1..n,
 * cnt = n points; nodes = 1: the nodes n+1..2n-1, cnt = n-1), either group:
 *   sum_j rho_j lagr[j] = sum_i c_i mono[i],   c = the coefficients of the polynomial with the values rho on those nodes
 * -- one interpolation of cnt scalars, two sums, the results compared as canonical affine bytes.  An array of another length
 * than cnt: PS_ERR_LENGTH; arrays of different groups, or sums pending on the context: PS_ERR_ARG.  rho: nrho >= cnt weights of
 * 32 B (PS_ERR_LENGTH), canonical (PS_ERR_ENCODING), drawn by the caller AFTER both arrays are fixed (128 random bits each are
 * enough); a wrong array passes with probability <= 2^-bits(rho). */
int ps_points_lagrange_check(ps_ctx* ctx, const ps_qap* q, const ps_points* mono, const ps_points* lagr, int nodes,
                             const uint8_t* rho_be32, size_t nrho, int* ok);
/* *ok = 1 iff `key` is ps_groth16_setup_from_srs(q, srs) with SOME non-zero (delta, gamma) folded in -- the fresh key
 * (delta = gamma = 1) and a ceremony's final key alike.  With T1, T2, A, B the string's arrays, diff = n_vars - n_io and
 * z = prod_{j=1..n} (X - j):
 *   alpha = A[0], beta = B[0], beta2 = srs.beta_g2 (bytes);  delta, delta2, gamma are not the identity and lie in the subgroup;
 *   e(delta, G2) = e(G1, delta2);
 *   xi = T1[:n], xi2 = T2[:n] (bytes, compared on the device: no array crosses PCIe);
 *   lxi against xi, lxi2 against xi2 (nodes = 0) and lxi_t against xi_t (nodes = 1): the equation of ps_points_lagrange_check;
 *     the three are optional (NULL: skipped, a monomial-only key has none);
 *   e(sum_{i<n-1} rho_i xi_t[i], delta2) = e(sum_{m<2n-1} (rho * z)_m T1[m], G2),   rho * z the polynomial product;
 *   for S = the IO variables (i < diff) and S = the rest, rho_S = rho[:n_vars] with the entries outside S zeroed, and cU, cV, cW
 *   the interpolants on 1..n of L rho_S, R rho_S, O rho_S (ps_qap_interpolate with rho_S for the solution),
 *   E_S = <cU, B> + <cV, A> + <cW, T1[:n]>:
 *     e(sum_{i<diff} rho_i io_lp[i], gamma) = e(E_io, G2),     e(sum_{i>=diff} rho_i nio_lp[i-diff], delta2) = e(E_nio, G2).
 * Each array enters exactly one equation that is linear in rho, so a key that differs from the derived one in any point passes
 * with probability <= 2^-bits(rho) per equation.  About sixteen sums, eight scalar interpolations and four pairing equalities
 * (each a product of its own, on host threads beside the device's work) where the derivation runs five conversions over group
 * elements: 28 ms against 4.05 s at 2^16 gates, 105 ms with the subgroup tests (profiles/crs_check_from_srs.txt).
 * The string's lengths as for ps_groth16_setup_from_srs (PS_ERR_LENGTH; n < 2: PS_ERR_ARG); the string itself is taken as
 * checked (ps_groth16_srs_check).  rho: nrho >= max(n_vars, n) weights of 32 B (PS_ERR_LENGTH), canonical (PS_ERR_ENCODING),
 * drawn by the caller AFTER string and key are fixed.  A key array of another length than this circuit's gives *ok = 0, not an
 * error; a key without xi, xi2, io_lp, nio_lp or xi_t: PS_ERR_ARG.  check_subgroup != 0: the key's arrays go through
 * ps_points_check_subgroup first, a point outside the subgroup gives *ok = 0 (0 only for a key the caller made itself).  A
 * delta, delta2 or gamma that is no canonical point on the curve: PS_ERR_ENCODING.  Needs an empty MSM queue. */
int ps_groth16_crs_check_from_srs(ps_ctx* ctx, const ps_qap* q, const ps_groth16_srs* srs, const ps_groth16_crs* key,
                                  const uint8_t* rho_be32, size_t nrho, int check_subgroup, int* ok);

/* ---- verifiers (host-side ate pairing; the IO commitments go through the GPU MSM) ---- */
typedef struct { /* the verifier's part of Groth16Setup (groth16.go:30-61) */
    uint8_t alpha[96];                        /* G1 */
    uint8_t beta2[192], gamma[192], delta2[192]; /* G2 */
    const ps_points* io_lp;                   /* IoLP, nbVars - nbIO G1 points (`diff` convention) */
} ps_groth16_vk;
/* Groth16Verify (groth16.go:214-233); io = sol[:diff] as in groth16_test.go:29.  *ok = 1/0.
 * Both verifiers and ps_pairing_equal treat every point they are given as untrusted: canonical encoding, on
 * the curve and in the order-r subgroup ([r]P = O), PS_ERR_ENCODING otherwise -- the checks the reference gets
 * from kyber's UnmarshalBinary before its Verify functions ever see a point [upstream]. */
int ps_groth16_verify(ps_ctx* ctx, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t A[96], const uint8_t B[192],
                      const uint8_t C[96], int* ok);
typedef struct { /* PHGR13VerifKey (pinochio.go:64-91); the *_io arrays are vk.vs[:diff], vk.ws[:diff], vk.ys[:diff] */
    uint8_t av[192], aw[96], ay[192], gamma[192], bgamma[96], bgamma2[192], yts[192];
    const ps_points *vs_io, *ws_io, *ys_io; /* G1, G2, G1 */
} ps_phgr13_vk;
/* PHGR13Verify (pinochio.go:281-378).  *ok = 1/0. */
int ps_phgr13_verify(ps_ctx* ctx, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proof, int* ok);
/* e(a1, b1) == e(a2, b2) ?  (Pair, curve.go:36-38; host only) */
int ps_pairing_equal(const uint8_t a1_g1[96], const uint8_t b1_g2[192], const uint8_t a2_g1[96], const uint8_t b2_g2[192],
                     int* equal);

/* prod_i e(g1[i], g2[i]) == 1 ?  Miller loops and their product on the device, one final exponentiation on the host.
 * Arrays of equal length (PS_ERR_LENGTH otherwise), n = 0 gives 1.  check != 0: both arrays go through
 * ps_points_check_subgroup first (PS_ERR_ENCODING outside the subgroup); 0 for arrays the caller made itself.
 * At most 2^24 pairs (PS_ERR_ARG beyond). */
int ps_pairing_product_is_one(ps_ctx* ctx, const ps_points* g1, const ps_points* g2, int check, int* is_one);

/* Groth16Verify (groth16.go:214-233) for nproofs proofs under ONE key, by random linear combination: for weights rho_i
 *     prod_i e(rho_i A_i, B_i) * e(-(sum rho_i) alpha, beta2) * e(-X, gamma) * e(-sum rho_i C_i, delta2) == 1,
 *     X = sum_j (sum_i rho_i io_ij) IoLP_j
 * -- nproofs Miller loops on the device, ONE sum over IoLP, one over the C_i, three host Miller loops, one final
 * exponentiation.  proofs: nproofs x (A 96 B || B 192 B || C 96 B), PS_FMT_AFFINE.  io: nproofs x diff scalars, proof-major
 * (len(io) != nproofs * len(vk->io_lp): PS_ERR_LENGTH).  rho_be32: nproofs x 32 B, canonical (PS_ERR_ENCODING), non-zero
 * (PS_ERR_ARG: a zero weight would skip a proof); drawn by the caller AFTER the proofs are fixed, as r and s are drawn
 * by the caller elsewhere in this header; 128 random bits each are enough.
 * *ok = 1 iff the combined equation holds: every proof valid => 1 for every rho; some proof invalid => 0 except with
 * probability <= nproofs / 2^bits(rho) over the choice of rho.  Every point is untrusted, as in ps_groth16_verify
 * (encoding, curve, subgroup: PS_ERR_ENCODING; ps_last_error() names the proof of a bad encoding).  nproofs = 0: *ok = 1.
 * nproofs = 1 with rho = 1 is exactly ps_groth16_verify.  nproofs <= 2^24 (PS_ERR_ARG beyond).  Needs an empty MSM
 * queue, like every one-call form.  The call costs ~50 ms up to ~1 000 proofs (subgroup tests, scaling and Miller loops
 * are latency chains of one lane each): a lone proof is 14 times slower than ps_groth16_verify (49.7 against 3.6 ms), the
 * batch wins from ~16 proofs on and is 155 times faster per proof at 4 096 (20 us; profiles/verify_batch.txt). */
int ps_groth16_verify_batch(ps_ctx* ctx, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t* proofs, size_t nproofs,
                            const uint8_t* rho_be32, int* ok);

/* WHICH proofs of a batch are invalid.  Arguments, validation and error codes are exactly those of
 * ps_groth16_verify_batch (lengths; canonical, non-zero rho; encoding, curve and subgroup of every point, ps_last_error()
 * naming the proof of a bad encoding -- a malformed or off-subgroup proof fails the CALL with PS_ERR_ENCODING, there is no
 * per-proof "malformed" verdict; an empty MSM queue), except the cap: nproofs <= 2^20 (PS_ERR_ARG beyond).
 * valid[i] = 1 / 0 for proof i, *ninvalid = the number of zeros.  nproofs = 0: *ninvalid = 0 and nothing is written.  On an
 * error *ninvalid = 0 and the contents of valid are unspecified.
 * How: the batch equation restricted to a set S of proofs,
 *     check(S): final_exp(prod_{i in S} miller(rho_i A_i, B_i) * miller(-(sum_S rho_i) alpha, beta2) * miller(-X_S, gamma)
 *                         * miller(-sum_S rho_i C_i, delta2)) == 1,   X_S = sum_j (sum_S rho_i io_ij) IoLP_j,
 * is multiplicative over disjoint unions.  The whole batch is checked exactly as ps_groth16_verify_batch checks it; if it
 * is rejected, the sets of a binary tree over the proofs are checked from the root down, both halves of every failing set,
 * from partial results kept on the device (no step passes over the proofs of a set again).
 * Soundness: check({i}) is proof i's own equation (Groth16Verify, groth16.go:214-233) raised to rho_i != 0, and GT has prime
 * order, so a verdict "invalid" is always exact; a verdict "valid" is wrong only if a set that passed hid a cancellation:
 * probability <= nproofs / 2^bits(rho) per passed check, over the choice of rho (drawn after the proofs are fixed).
 * Cost: an accepted batch costs what ps_groth16_verify_batch costs (one check, nothing else is launched); b invalid proofs
 * among N cost at most 1 + 2 b ceil(log2 N) checks, each three host Miller loops and one final exponentiation, the sets of a
 * level side by side on at most 16 host threads (profiles/verify_locate.txt).
 * Device memory, kept by the context: 1 344 B per proof for the levels of the product tree; for a rejected batch also
 * 448 B per proof for the sums of rho_i C_i and 64 B per proof and per (public input + 1) for the scalar sums; a batch that
 * cannot get them fails with PS_ERR_HIP and a message that says so. */
typedef struct {
    uint32_t checks;   /* sets whose equation was evaluated, the whole batch included */
    uint32_t levels;   /* depth reached below the root (0: batch accepted, or nproofs <= 1) */
    uint32_t invalid;  /* proofs reported invalid */
    uint32_t reserved;
} ps_verify_locate_info;
int ps_groth16_verify_batch_locate(ps_ctx* ctx, const ps_groth16_vk* vk, const ps_scalars* io, const uint8_t* proofs,
                                   size_t nproofs, const uint8_t* rho_be32, uint8_t* valid /* nproofs bytes: 1 / 0 */,
                                   size_t* ninvalid);
int ps_groth16_verify_batch_locate_info(ps_ctx* ctx, ps_verify_locate_info* out); /* of the last locate call on ctx */

/* PHGR13Verify (pinochio.go:281-378) for nproofs proofs under ONE key, by random linear combination.  With diff =
 * len(vk->vs_io), io proof-major (io_ij, len(io) != nproofs * diff: PS_ERR_LENGTH), gv_i = sum_j io_ij vs_j + vss_i and
 * S_X = sum_i rho_i X_i for a proof element X, the five products of ps_phgr13_verify become
 *     E0 division  prod_i e(rho_i gv_i, wss_i) * prod_k e(P_k, ws_k) * e(-S_hs, yts) * e(-(S_yss + sum_j t_j ys_j), G2) == 1
 *                  P_k = sum_i io_ik (rho_i gv_i),  t_j = sum_i rho_i io_ij
 *     E1 v         e(S_vass, G2) * e(-S_vss, av) == 1
 *     E2 w         e(S_wass, G2) * e(-aw, S_wss) == 1
 *     E3 y         e(S_yass, G2) * e(-S_yss, ay) == 1
 *     E4 linear    e(S_gz, gamma) * e(-(S_vss + S_yss), bgamma2) * e(-bgamma, S_wss) == 1
 * -- nproofs + diff Miller loops on the device (E0 with the G2 commitment of the inputs expanded by bilinearity: no G2
 * arithmetic per proof), the eight S_X as one ps_msm_multi, eleven host Miller loops, and FIVE final exponentiations: each
 * product is checked on its own.  *ok = 1 iff all five hold; all five are always evaluated.
 * Soundness: each E_c is linear in rho and GT has prime order, so if some proof violates equation c, E_c still holds only
 * with probability <= nproofs / 2^bits(rho) over the choice of rho, as for ps_groth16_verify_batch.  rho_be32: nproofs x
 * 32 B, canonical (PS_ERR_ENCODING), non-zero (PS_ERR_ARG), drawn by the caller AFTER the proofs are fixed; 128 random bits
 * each are enough.  The five are NOT merged into one product: under equal weights the errors of two equations of one proof
 * could cancel (vass + D with wass - D).
 * Every point is untrusted, as in ps_phgr13_verify: encoding, curve and subgroup, PS_ERR_ENCODING otherwise, and
 * ps_last_error() names the proof index and the element of a bad proof point.  A malformed proof fails the CALL: there is
 * no per-proof verdict (ps_phgr13_verify_batch_locate names the invalid proofs of a rejected batch).  vs_io, ws_io, ys_io of different lengths:
 * PS_ERR_LENGTH.  diff = 0 is legal.  nproofs = 0: *ok = 1.  nproofs = 1 with rho = 1 gives the verdict of ps_phgr13_verify.
 * Needs an empty MSM queue (PS_ERR_ARG), like every one-call form.
 * Caps, checked before any device work: nproofs <= 2^20 and nproofs * (diff + 1) < 2^24; PS_ERR_ARG beyond, with a message
 * that says to split the batch (the verdicts of the parts AND together).
 * Device memory, kept by the context: per proof 1 008 B of Miller values and 800 B of points and weights, and per proof and
 * per public input 448 B for the two XYZZ buffers of the scaled key points and 104 B of scalars (7.5 GB + 1.7 GB at the
 * second cap); for the duration of the call also the proofs and both sides of the device's loops (1 344 B per proof) and
 * the transposed inputs (32 B per proof and input).  A context that cannot get them fails with PS_ERR_HIP.
 * Cost: a call costs 45-55 ms up to ~256 proofs (subgroup tests, scaling and Miller loops are latency chains of one lane each): a lone proof is
 * 10 times slower than ps_phgr13_verify (53 against 4.6 ms at diff = 6), the batch wins from 16 proofs on (the crossover lies between 1 and 16), is 70 times
 * faster at 1 024 and costs 21.3 us per proof at 4 096 with diff = 6, 15.1 us with diff = 63 (225 and 701 times the loop;
 * profiles/phgr13_verify_batch.txt). */
typedef struct {
    uint32_t failed;        /* bit c set: equation E_c did not hold (0 division, 1 v, 2 w, 3 y, 4 linear); 0 after *ok = 1 */
    uint32_t device_loops;  /* Miller loops run on the device: nproofs + diff */
    uint32_t reserved[2];
} ps_phgr13_batch_info;
int ps_phgr13_verify_batch(ps_ctx* ctx, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proofs,
                           size_t nproofs, const uint8_t* rho_be32, int* ok);
int ps_phgr13_verify_batch_info(ps_ctx* ctx, ps_phgr13_batch_info* out); /* of the last batch call on ctx */

/* WHICH proofs of a PHGR13 batch are invalid, and which of the five equations each of them violates.  Arguments,
 * validation, error codes, messages and caps are exactly those of ps_phgr13_verify_batch (lengths; canonical, non-zero rho;
 * encoding, curve and subgroup of every point, ps_last_error() naming the proof and the element -- a malformed or
 * off-subgroup proof fails the CALL with PS_ERR_ENCODING, there is no per-proof "malformed" verdict; an empty MSM queue).
 * valid[i] = 1 / 0 for proof i, failed[i] (may be NULL) = the mask of the equations proof i violates (bit c = E_c, 0 for a
 * valid proof), *ninvalid = the number of zeros in valid.  nproofs = 0: *ninvalid = 0 and nothing is written.  nproofs = 1
 * rejected: valid[0] = 0 and failed[0] = the batch's mask, without a descent.  On an error *ninvalid = 0 and the contents of
 * valid and failed are unspecified.  Afterwards ps_phgr13_verify_batch_info reports the mask of the whole batch, as after
 * the plain call.
 * How: for a set S of proofs the five equations of ps_phgr13_verify_batch restricted to S,
 *     E0(S)  final_exp(F_S * prod_k miller(P_S,k, ws_k) * miller(-hs_S, yts) * miller(-(yss_S + sum_j t_S,j ys_j), G2)) == 1
 *     E1(S)  final_exp(miller(vass_S, G2) * miller(-vss_S, av)) == 1
 *     E2(S)  final_exp(miller(wass_S, G2) * miller(-aw, wss_S)) == 1
 *     E3(S)  final_exp(miller(yass_S, G2) * miller(-yss_S, ay)) == 1
 *     E4(S)  final_exp(miller(gz_S, gamma) * miller(-(vss_S + yss_S), bgamma2) * miller(-bgamma, wss_S)) == 1
 * with X_S = sum_{i in S} rho_i X_i, t_S,j = sum_S rho_i io_ij, P_S,k = sum_S io_ik (rho_i gv_i) and F_S = prod_S
 * miller(rho_i gv_i, wss_i), are each multiplicative over disjoint unions.  The whole batch is checked exactly as
 * ps_phgr13_verify_batch checks it; if it is rejected, the sets of a binary tree over the proofs are checked from the root
 * down, both halves of every failing set, each half only on the equations its parent failed, from partial results kept on
 * the device (no step passes over the proofs of a set again; the diff loops of E0 of every set run on the device and one
 * Fp12 value per set comes back).
 * Soundness: E_c({i}) is proof i's own equation c (PHGR13Verify, pinochio.go:281-378) raised to rho_i != 0, and GT has prime
 * order, so a set bit of failed[i] is always exact; valid[i] = 1, or an unset bit of failed[i], is wrong only if a check
 * that passed hid a cancellation: probability <= nproofs / 2^bits(rho) per passed product, over the choice of rho (drawn
 * after the proofs are fixed).
 * Cost: an accepted batch is the work of ps_phgr13_verify_batch (one check, five products, nothing else is launched or
 * allocated beyond the levels of its product tree, kept apart from the key's loops; measured below); b invalid proofs among N cost checks <= 1 + 2 b ceil(log2 N) and
 * products <= 5 + 2 ceil(log2 N) * sum_i popcount(failed[i]), each product two or three host Miller loops and one final
 * exponentiation, the products of a level side by side on at most 16 host threads.
 * Measured (profiles/phgr13_verify_locate.txt; N = 256, 1 024, 4 096, diff = 6 and 63, medians of interleaved runs): an accepted
 * batch costs the plain call plus 0.9 .. 2.6 ms of extra product launches -- inside the plain call's run-to-run spread (0.5 ..
 * 8 ms) at diff = 6 and N <= 1 024, but 1.1 .. 2.1 ms (2 .. 4 %) against a spread of 0.2 .. 1.0 ms at diff = 63: not free there.
 * A rejected batch beats both a loop of ps_phgr13_verify and caller-side halving with ps_phgr13_verify_batch at every
 * measured point: one bad proof among 4 096 at diff = 6 in 112 ms (one equation failed) or 381 ms (three, E0 among them)
 * against 1.5 s of halving and 19.6 s of the loop; sixteen in 137 / 497 ms against 15.8 s and 19.6 s.  The smallest margins:
 * 2.1 x halving (one bad proof, E0 failed, diff = 63, N = 256) and 3.8 x the loop (sixteen, diff = 6, N = 256).
 * Device memory, kept by the context, on top of the plain call's: 1 344 B per proof for the levels of the product tree
 * (2 x sizeof Fp12 = 2 x 672) and 672 B per public input; for a rejected batch also, for the trees its failed equations
 * read, 448 B per proof (2 x sizeof XYZZ G1 = 2 x 224) for each of the up to seven G1 elements and, if E0 failed, for each
 * public input, 896 B per proof (2 x sizeof XYZZ G2) for wss if E2 or E4 failed, 64 B per proof and per (public input + 1)
 * for the scalar sums if E0 failed, and while the trees are built 152 B per proof and element (sizeof affine G1 112 + Fr 40)
 * plus 224 B per proof and 40 B per proof and public input.  A batch that cannot get them fails with PS_ERR_HIP and a
 * message that gives the bytes asked for. */
typedef struct {
    uint32_t checks;    /* sets evaluated, the whole batch included */
    uint32_t products;  /* pairing products evaluated = final exponentiations: 5 for the batch, then one per tested (set, equation) */
    uint32_t levels;    /* depth reached below the root (0: accepted, or nproofs <= 1) */
    uint32_t invalid;   /* proofs reported invalid */
    uint32_t failed;    /* OR of the masks of the invalid proofs = the batch's ps_phgr13_batch_info.failed */
    uint32_t reserved[3];
} ps_phgr13_locate_info;
int ps_phgr13_verify_batch_locate(ps_ctx* ctx, const ps_phgr13_vk* vk, const ps_scalars* io, const ps_phgr13_proof* proofs,
                                  size_t nproofs, const uint8_t* rho_be32, uint8_t* valid /* nproofs bytes: 1 / 0 */,
                                  uint8_t* failed /* nproofs masks, bit c = E_c; may be NULL */, size_t* ninvalid);
int ps_phgr13_verify_batch_locate_info(ps_ctx* ctx, ps_phgr13_locate_info* out); /* of the last locate call on ctx */

/* ---- KZG polynomial commitments over the powers-of-tau string: Poly.Commit / PolyCommit, Poly.Eval (algebra.go:107-115)
 *      and Poly.Div by a linear factor (algebra.go:119-137) ----
 * The commitment of p (n coefficients, lowest degree first) is C = sum_i p_i tau_g1[i] = [p(tau)] G1; the proof that
 * p(z) = y is pi = [q(tau)] G1 with q = (p(X) - y) / (X - z); anybody checks e(C - y G1 + z pi, G2) = e(pi, tau G2).  Entry
 * points added within revision 5 (found by symbol, no struct at all).
 * Shared conventions: z, y and rho are 32-byte big-endian and canonical (PS_ERR_ENCODING otherwise); a NULL argument is
 * PS_ERR_ARG; an empty p is PS_ERR_LENGTH; k = 0 is PS_OK with no output buffer written; k * n >= 2^32 is PS_ERR_ARG (split the
 * points).  p may be a view (ps_scalars_slice).
 *
 * Value and quotient come from ONE recurrence, h_n = 0, h_i = p_i + z h_{i+1}: h_0 = p(z) and q_{i-1} = h_i -- on the device
 * a scan in three launches (tile totals, one carry walk per point, apply), for all k points at once.
 * ps_poly_scan_tile: the coefficients per workgroup of that scan (tests sit on its edges; a constant of the build). */
int ps_poly_scan_tile(void);
/* y[j] = p(z_j), j < k: y_be32 has k * 32 bytes.  (Poly.Eval, algebra.go:107-115.) */
int ps_poly_eval(ps_ctx* ctx, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32);
/* *q: k * (n - 1) scalars, row j = the quotient of p by (X - z_j), lowest degree first -- member-major, the layout
 * ps_msm_batch reads; rem[j] = p(z_j).  Poly.Div (algebra.go:119-137) with the divisor (1, -z) of the reference's
 * highest-first order.  n = 1: PS_ERR_LENGTH (no quotient to hold).  k = 0: *q is an empty vector.  Caller frees *q. */
int ps_poly_div_linear(ps_ctx* ctx, const ps_scalars* p, const uint8_t* z_be32, size_t k, ps_scalars** q, uint8_t* rem_be32);
/* out = sum_i p_i tau_g1[i]: ps_msm over the first n points of the string, which may be longer than p; a shorter string is
 * PS_ERR_LENGTH (algebra.go:350-352), a G2 array PS_ERR_ARG.  Needs an empty MSM queue. */
int ps_kzg_commit(ps_ctx* ctx, const ps_points* tau_g1, const ps_scalars* p, uint8_t out[96]);
/* y[j] = p(z_j) and proofs[j] = [q_j(tau)] G1, j < k (k * 32 and k * 96 bytes): values and quotients on the device, then ONE
 * ps_msm_batch of the k quotient rows over tau_g1[0 .. n-1); the quotients never leave the device.  Proof j is byte-identical
 * to ps_msm over that view and row j of ps_poly_div_linear.  n = 1: y = p_0 and identity proofs, without a division.  The string
 * must hold at least n points (the commitment being opened needs them; PS_ERR_LENGTH).  Needs an empty MSM queue
 * (PS_ERR_ARG otherwise), as the other composite entries do. */
int ps_kzg_open(ps_ctx* ctx, const ps_points* tau_g1, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32,
                uint8_t* proofs /* k x 96 */);
/* *ok = 1 iff e(commit - y G1 + z proof, G2) = e(proof, tau_g2_1), tau_g2_1 being the string's tau_g2[1] = tau G2.  Host only
 * (the ate pairing of the verifiers, two Miller loops and one final exponentiation).  A point that is not canonical or not
 * on the curve: PS_ERR_ENCODING; a point outside the order-r subgroup: *ok = 0. */
int ps_kzg_verify(const uint8_t tau_g2_1[192], const uint8_t commit[96], const uint8_t z_be32[32], const uint8_t y_be32[32],
                  const uint8_t proof[96], int* ok);
/* k openings (C_j, z_j, y_j, pi_j) under ONE string -- polynomials and points may all differ -- by random linear combination:
 *     e(sum_j rho_j (C_j + z_j pi_j) - (sum_j rho_j y_j) G1, G2) * e(-sum_j rho_j pi_j, tau_g2_1) == 1
 * -- two sums over the uploaded points (ps_msm), the scalars rho_j z_j and sum rho_j y_j on the host, one two-pair product.
 * commits, proofs: k * 96 bytes; z, y, rho: k * 32.  rho: canonical (PS_ERR_ENCODING), non-zero (PS_ERR_ARG: a zero weight
 * would skip an opening), drawn by the caller AFTER commitments, points, values and proofs are fixed, as for
 * ps_groth16_verify_batch; 128 random bits each are enough.
 * *ok = 1 iff the combined equation holds.  Every opening valid => 1 for every rho.  Some opening invalid => the left side
 * is the product of the single equations' values raised to rho_j, a non-trivial linear form in the rho_j over a group of
 * prime order, so *ok = 1 with probability <= 1 / (2^bits(rho) - 1) over the choice of rho (the false-accept bound; with
 * equal weights two errors can cancel: y_1 + d with y_2 - d).
 * Encodings and the curve equation are always tested (PS_ERR_ENCODING).  check_subgroup != 0: commitments and proofs go
 * through ps_points_check_subgroup and tau_g2_1 is tested likewise; a point outside the subgroup gives *ok = 0 (0 only for
 * points the caller made itself).  k = 0: *ok = 1.  k <= 2^24 (PS_ERR_ARG beyond).  Needs an empty MSM queue. */
int ps_kzg_verify_batch(ps_ctx* ctx, const uint8_t tau_g2_1[192], const uint8_t* commits, const uint8_t* z_be32, const uint8_t* y_be32,
                        const uint8_t* proofs, const uint8_t* rho_be32, size_t k, int check_subgroup, int* ok);

/* ---- Many polynomials at shared points: Poly.Add / Poly.Sub (algebra.go:161-196) on the device, and ONE proof per point ----
 * *out: t rows of N = max_i len(v_i) scalars, row j = sum_i c_ij v_i with every v_i zero-extended to N -- member-major, the
 * layout ps_msm_batch and the scan read; canonical plain words like any ps_scalars.  coef_be32: m * t canonical scalars, entry
 * [i * t + j] (PS_ERR_ENCODING otherwise).  The inputs may be views (ps_scalars_slice) and may repeat.  A NULL argument or
 * m = 0: PS_ERR_ARG; an empty input: PS_ERR_LENGTH; t = 0: *out is an empty vector.  Limits: t * N < 2^32 (what the scan reads)
 * and m * t <= 2^20 (the coefficients go to the device as one table); PS_ERR_ARG beyond.  A zero coefficient costs no product.
 * Caller frees *out. */
int ps_scalars_lincomb(ps_ctx* ctx, const ps_scalars* const* v, size_t m, const uint8_t* coef_be32 /* m * t, entry [i * t + j] */,
                       size_t t, ps_scalars** out);
/* m polynomials opened at t points with ONE proof per point.  c_ij != 0 means "polynomial i is opened at point j, with this
 * weight":
 *     y[i * t + j] = p_i(z_j) where c_ij != 0, 32 zero bytes elsewhere
 *     proofs[j] = [q_j(tau)] G1,  f_j = sum_i c_ij p_i,  q_j = (f_j - f_j(z_j)) / (X - z_j)
 * The weights are the caller's: powers of a Fiat-Shamir challenge, drawn AFTER the commitments and the values are fixed
 * (weights known beforehand let errors in two values of one point cancel).  Division by (X - z) is linear, so the call costs
 * t rows of ps_msm_batch whatever m is: values by the scan per polynomial, the rows f_j by ps_scalars_lincomb, their quotients
 * by the scan, ONE ps_msm_batch over tau_g1[0 .. N-1), N = max_i len(p_i); nothing leaves the device.  Proof j is byte-identical
 * to ps_msm over that view and row j of ps_poly_div_linear applied to row j of ps_scalars_lincomb; with m = 1 and c = 1 the
 * call returns ps_kzg_open's bytes.  N = 1: the values are the constants and the proofs identities.  A column of c without a
 * non-zero entry: PS_ERR_ARG (nothing would be opened at that point); tau_g1 shorter than N: PS_ERR_LENGTH; t = 0: PS_OK,
 * nothing written; the limits of ps_scalars_lincomb.  Needs an empty MSM queue (PS_ERR_ARG otherwise). */
int ps_kzg_open_multi(ps_ctx* ctx, const ps_points* tau_g1, const ps_scalars* const* polys, size_t m, const uint8_t* z_be32 /* t */,
                      size_t t, const uint8_t* coef_be32 /* m * t */, uint8_t* y_be32 /* m * t */, uint8_t* proofs /* t * 96 */);
/* The check of what ps_kzg_open_multi made.  With w_i = sum_j rho_j c_ij and s = sum_j rho_j sum_i c_ij y_ij (on the host):
 *     e(sum_i w_i C_i + sum_j rho_j z_j pi_j - s G1, G2) * e(-sum_j rho_j pi_j, tau_g2_1) == 1
 * -- ps_kzg_verify_batch's equation with C'_j = sum_i c_ij C_i folded into the scalars: two sums over the uploaded [C | pi]
 * array and one two-pair product.  y entries where c_ij = 0 are ignored (not even decoded).  rho: one weight per POINT, with the
 * rules of ps_kzg_verify_batch (canonical, non-zero, drawn afterwards); the subgroup option, the encoding errors and the
 * false-accept bound are that call's too.  A column of c without a non-zero entry: PS_ERR_ARG.  t = 0: *ok = 1.
 * m + t <= 2^24 (PS_ERR_ARG beyond).  Needs an empty MSM queue.  With m = t and c the identity matrix this is
 * ps_kzg_verify_batch. */
int ps_kzg_verify_multi(ps_ctx* ctx, const uint8_t tau_g2_1[192], const uint8_t* commits /* m * 96 */, size_t m, const uint8_t* z_be32,
                        size_t t, const uint8_t* coef_be32, const uint8_t* y_be32 /* m * t */, const uint8_t* proofs /* t * 96 */,
                        const uint8_t* rho_be32 /* t */, int check_subgroup, int* ok);

/* ---- One polynomial at a SET of points: Poly.Div (algebra.go:119-137) by Z_S = prod_j (X - z_j), and ONE proof for the set ----
 * S = {z_0 .. z_{k-1}}, k distinct canonical points; r = the interpolant of (z_j, p(z_j)), degree < k; q = (p - r) / Z_S, the
 * n - k quotient coefficients.  By partial fractions, with w_j = 1 / prod_{l != j} (z_j - z_l),
 *     q = sum_j w_j (p - p(z_j)) / (X - z_j)
 * -- the rows of the linear scan, folded into ONE row while they are scanned: totals and carry walk of
 * ps_poly_div_linear for the k points, then an apply pass in which a workgroup owns a tile and a group of
 * ps_poly_scan_set_group() points.  Device memory beside the result: ceil(k / G) partial rows of n - k scalars (none for k <= G),
 * where k rows of n - 1 would be needed to compose the same from ps_poly_div_linear and ps_scalars_lincomb.
 * Shared conventions: z and y are 32-byte big-endian and canonical (PS_ERR_ENCODING otherwise); two equal points are PS_ERR_ARG
 * (the message names both indices: the weights do not exist -- the k single-point openings take repeated points); k = 0 is
 * PS_ERR_ARG (division by the constant 1 is a copy and is not offered); k > 1024 (the host work is quadratic in k) or
 * k * n >= 2^32 is PS_ERR_ARG; a NULL argument is PS_ERR_ARG; an empty p is PS_ERR_LENGTH.  p may be a view.
 * ps_poly_scan_set_group: G, the points a workgroup folds (tests sit on its edges; a constant of the build). */
int ps_poly_scan_set_group(void);
/* *q: the n - k coefficients of q, lowest degree first; an empty vector for n <= k.  y[j] = p(z_j) (k * 32 bytes).  rem, unless
 * NULL: the k coefficients of the remainder r, lowest first (k * 32 bytes) -- interpolated on the host from the y_j, O(k^2); for
 * n <= k it is p zero-extended.  Poly.Div with the divisor Z_S of the reference's highest-first order.  Caller frees *q. */
int ps_poly_div_roots(ps_ctx* ctx, const ps_scalars* p, const uint8_t* z_be32, size_t k, ps_scalars** q, uint8_t* y_be32 /* k */,
                      uint8_t* rem_be32 /* k coefficients, lowest first; may be NULL */);
/* y[j] = p(z_j) and proof = [q(tau)] G1 for the whole set: the scan above, then ONE ps_msm (the lone sum, not a row of
 * ps_msm_batch) over tau_g1[0 .. n-k); nothing but values and proof leaves the device.  The proof is byte-identical to ps_msm
 * over that view and ps_poly_div_roots' quotient, equals sum_j w_j proofs_j of ps_kzg_open, and for k = 1 is ps_kzg_open's.
 * n <= k: the proof is the identity and the values are ps_poly_eval's.  The string must hold at least n points (the commitment
 * being opened needs them; PS_ERR_LENGTH, BlindEval's wording, algebra.go:350-352).  Needs an empty MSM queue (PS_ERR_ARG). */
int ps_kzg_open_set(ps_ctx* ctx, const ps_points* tau_g1, const ps_scalars* p, const uint8_t* z_be32, size_t k, uint8_t* y_be32 /* k */,
                    uint8_t proof[96]);
/* *ok = 1 iff  e(commit - [r(tau)] G1, G2) * e(-proof, [Z_S(tau)] G2) == 1.
 * On the host: the coefficients of r (interpolation of the (z_j, y_j)) and of Z_S, both O(k^2).  On the device: [r(tau)] G1 as
 * ps_msm over tau_g1[0 .. k) and [Z_S(tau)] G2 as ps_msm over tau_g2[0 .. k].  Then commit - R by ps_points_lincomb and one
 * two-pair product on the host.  tau_g1 holds at least k points and tau_g2 at least k + 1 (PS_ERR_LENGTH otherwise); they are the
 * caller's own arrays and are not tested here (ps_groth16_srs_check does that).  Encodings and the curve equation of commit and
 * proof are always tested (PS_ERR_ENCODING); check_subgroup != 0: both are tested for the subgroup as ps_kzg_verify tests them,
 * and a point outside gives *ok = 0.  For k = 1 the equation is ps_kzg_verify's.  Needs an empty MSM queue. */
int ps_kzg_verify_set(ps_ctx* ctx, const ps_points* tau_g1 /* >= k */, const ps_points* tau_g2 /* >= k + 1 */, const uint8_t commit[96],
                      const uint8_t* z_be32, const uint8_t* y_be32, size_t k, const uint8_t proof[96], int check_subgroup, int* ok);

/* ---- Polynomials given by their VALUES on the domain 1 .. n (the Lagrange form): no interpolation, no division ----
 * A polynomial of degree < n is the vector v of its values on the nodes 1 .. n of a ps_qap (n = its gate count; the ps_qap also
 * supplies the factorial tables of the barycentric weights w_i = (-1)^(n-i) / ((i-1)! (n-i)!)).  With e_i = 1 / (z - i):
 *     p(z) = prod_i (z - i) * sum_i w_i v_i e_i                      for z off the domain,  p(m) = v_m on it;
 *     q = (p - p(z)) / (X - z) has the values q_i = (p(z) - v_i) e_i at the nodes i != z, and at a node z = m the value the
 *     degree bound deg q <= n - 2 forces: q_m = (sum_{i != m} w_i v_i e_i - v_m sum_{i != m} w_i e_i) / w_m.
 * The n inversions are ONE field inversion per workgroup and a few products per node.  lag_g1 is the
 * Lagrange form of the string on the same nodes -- [l_i(tau)] G1, what ps_points_monomial_to_lagrange makes of tau_g1[0 .. n)
 * and ps_points_lagrange_check tests -- so that sum_i q_i lag_g1[i] = [q(tau)] G1: commitments and proofs are the SAME group
 * elements, hence the same 96 bytes, as ps_kzg_commit and ps_kzg_open give for the interpolated coefficients, and
 * ps_kzg_verify / ps_kzg_verify_batch check them unchanged.
 * Shared conventions: `values` and lag_g1 hold exactly n elements (PS_ERR_LENGTH otherwise); a G2 array, a NULL argument,
 * k * n >= 2^32 or -- where a sum is taken -- a non-empty MSM queue are PS_ERR_ARG; z is 32-byte big-endian and canonical
 * (PS_ERR_ENCODING otherwise); k = 0 is PS_OK with nothing written.  Points may repeat, and points on and off the domain may
 * share a call.  n = 1 is no special case: y = v_1 and q = 0 for every z.
 * ps_poly_lagrange_tile: the nodes a workgroup inverts together (tests sit on its edges; a constant of the build). */
int ps_poly_lagrange_tile(void);
/* *out = the n values of (L|R|O).sol on the domain -- what ps_qap_interpolate interpolates, uninterpolated.  which: 0 left,
 * 1 right, 2 out; the argument rules are ps_qap_interpolate's.  Caller frees *out. */
int ps_qap_gate_values(ps_ctx* ctx, const ps_qap* q, const ps_scalars* sol, int which, ps_scalars** out);
/* y[j] = p(z_j), k * 32 bytes, for the polynomial with the given values: ps_poly_eval of the interpolated coefficients. */
int ps_poly_eval_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, uint8_t* y_be32);
/* *qv: k rows of n scalars, row after row (the layout ps_msm_batch reads): row j = the values on 1 .. n of
 * (p - p(z_j)) / (X - z_j); y[j] = p(z_j).  k = 0: an empty vector.  Caller frees *qv. */
int ps_poly_div_linear_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, ps_scalars** qv,
                                uint8_t* y_be32 /* k */);
/* out = sum_i v_i lag_g1[i] = [p(tau)] G1: ps_msm over arrays of one length (PS_ERR_LENGTH otherwise). */
int ps_kzg_commit_lagrange(ps_ctx* ctx, const ps_points* lag_g1, const ps_scalars* values, uint8_t out[96]);
/* y[j] = p(z_j) and proofs[j] = [q_j(tau)] G1 for k points: the quotient rows above, then the lone ps_msm for k = 1 and ONE
 * ps_msm_batch of the k rows over lag_g1 otherwise; the rows never leave the device. */
int ps_kzg_open_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_points* lag_g1, const ps_scalars* values, const uint8_t* z_be32, size_t k,
                         uint8_t* y_be32 /* k */, uint8_t* proofs /* k * 96 */);

/* ---- A value-form polynomial at a SET of points: ps_poly_div_roots and ps_kzg_open_set from the values, no interpolation ----
 * S = {z_0 .. z_{k-1}}, k distinct canonical points, on the domain or off it; c_j = 1 / prod_{l != j} (z_j - z_l), y_j = p(z_j).
 * The partial fractions of the set section hold value by value on the nodes:
 *     q(i) = sum_j c_j (y_j - v_i) / (z_j - i)     with the term of a point that IS node i replaced by c_j q_m, q_m the value
 *                                                  ps_poly_div_linear_lagrange gives at its own node
 * are the n values on 1 .. n of q = (p - r) / Z_S, of degree <= n - 1 - k, so sum_i q(i) lag_g1[i] = [q(tau)] G1: the proof of
 * ps_kzg_open_set for the interpolated coefficients, the same 96 bytes, and ps_kzg_verify_set checks it unchanged.  The k
 * linear quotients are folded into ONE row while they are computed: a workgroup owns a tile and a group
 * of ps_poly_lagrange_set_group() points, and ONE field inversion serves the whole group.  Device memory beside the result:
 * ceil(k / G) partial rows of n scalars (none for k <= G), never k * n.
 * Conventions, the union of the two sections: two equal points are PS_ERR_ARG (the message names both indices); k = 0 is
 * PS_ERR_ARG; `values` and lag_g1 hold exactly n elements (PS_ERR_LENGTH otherwise); z is canonical (PS_ERR_ENCODING otherwise); a
 * G2 array, a NULL argument, k > 1024 or k * n >= 2^32 are PS_ERR_ARG, and so is a non-empty MSM queue where a sum is taken.
 * Added within revision 5 (found by symbol, no existing struct changed).
 * ps_poly_lagrange_set_group: G, the points that share an inversion (tests sit on its edges; a constant of the build). */
int ps_poly_lagrange_set_group(void);
/* *qv: the n values of q on 1 .. n, all zero for k >= n.  y[j] = p(z_j) as ps_poly_eval_lagrange gives it (k * 32 bytes).  rem,
 * unless NULL: the k coefficients of the remainder r, lowest first, as ps_poly_div_roots gives them.  Caller frees *qv. */
int ps_poly_div_roots_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_scalars* values, const uint8_t* z_be32, size_t k, ps_scalars** qv,
                               uint8_t* y_be32 /* k */, uint8_t* rem_be32 /* k coefficients, lowest first; may be NULL */);
/* y[j] = p(z_j) and proof = [q(tau)] G1 for the whole set: the row above, then ONE ps_msm (the lone sum) over lag_g1; nothing but
 * values and proof leaves the device.  Byte-identical to ps_kzg_open_set on ps_qap_interpolate's coefficients, and for k = 1 to
 * ps_kzg_open_lagrange.  k >= n: the proof is the identity. */
int ps_kzg_open_set_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_points* lag_g1, const ps_scalars* values, const uint8_t* z_be32,
                             size_t k, uint8_t* y_be32 /* k */, uint8_t proof[96]);

/* ---- A value-form polynomial at EVERY node of its domain: the n proofs pi_m, m = 1 .. n, in one call ----
 * What a table prover or a data-availability sampler precomputes.  With kappa(d) = 1 / d for d != 0 and kappa(0) = 0, the
 * quotient of node m has the values (v_m - v_i) kappa(m - i) at the nodes i != m and q_m (above) at m itself, hence
 *     pi_m = v_m K_m - U_m + g_m lag_g1[m-1]
 *     U_m = sum_i kappa(m - i) (v_i lag_g1[i-1])      K_m = sum_i kappa(m - i) lag_g1[i-1]
 *     s_m = sum_i kappa(m - i) w_i v_i                c_m = sum_i kappa(m - i) w_i             g_m = (s_m - v_m c_m) / w_m
 * -- four Toeplitz products with one multiplier, run as cyclic convolutions of size S = 2^p >= 2n - 1: two transforms over
 * points (the NTT over points of the key conversion) and a batch of two over scalars, about (p + 1) S + 3n scalar
 * multiplications of points where n calls of ps_kzg_open_lagrange take n sums over n points.  K_m depends
 * on n and the string alone: ps_kzg_all_key_lagrange computes it once, and a call that is handed it runs one transform pair, not
 * two.  kappa is antisymmetric: K and U read backwards are the NEGATED sums.
 * Conventions, those of the value-form section: `values`, lag_g1 and all_key hold exactly n elements (PS_ERR_LENGTH otherwise); a
 * G2 array or a NULL argument (other than all_key) is PS_ERR_ARG; n > 2^30 is PS_ERR_ARG (the S <= 2^31 points of a transform are
 * indexed with 32 bits).  n = 1 is no special case for the caller: one identity point.  The points of lag_g1 and all_key must lie
 * in the subgroup of order r, as ps_points_monomial_to_lagrange requires of its input (the scalar multiplications split with the
 * endomorphism); identity entries are legal.  The values at the nodes are the input itself: there is no y output.  Each proof is
 * the group element ps_kzg_open_lagrange gives at z = m, hence the same 96 bytes, and ps_kzg_verify / ps_kzg_verify_batch check
 * the proofs unchanged.  Device memory of a call: S points of 224 bytes and 3 S + 2 n scalars of 40, beside the n results.  The
 * calls return with the stream idle.  Added within revision 5 (found by symbol, no existing struct changed). */
/* *out = K_m, m = 1 .. n: n canonical affine points on the device; depends on n and the string only.  Caller frees *out. */
int ps_kzg_all_key_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_points* lag_g1, ps_points** out);
/* (*proofs)[m-1] = [((p - v_m) / (X - m))(tau)] G1 for every node: n canonical affine points on the device; caller frees.
 * all_key = what ps_kzg_all_key_lagrange returned for (q, lag_g1), or NULL: computed inside the call and dropped. */
int ps_kzg_open_all_lagrange(ps_ctx* ctx, const ps_qap* q, const ps_points* lag_g1, const ps_points* all_key, const ps_scalars* values,
                             ps_points** proofs);

#ifdef __cplusplus
}
#endif
#endif
