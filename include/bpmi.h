/*
 * bpmi.h -- C-ABI of libbpmi.so: the MI355X (gfx950) multi-scalar-multiplication +
 * inner-product-argument engine that drops in behind src/pippenger and
 * src/innerproduct of wborgeaud/python-bulletproofs.
 *
 * The reference has no FFI layer of its own: its hot path is a Python call
 * surface that bottoms out in the third-party `fastecdsa` C extension.  Each
 * entry point below names the reference interface it replaces (paths relative to
 * /root/reference); INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross this boundary;
 *   - field elements / scalars: 32 bytes little-endian (= 4 x u64 LE limbs);
 *     affine point: x || y (64 bytes); the identity is 64 zero bytes
 *     ((0,0) is not on y^2 = x^3 + 7);
 *   - scalars of the MSM / scalar-multiplication entry points (bpmi_msm*, bpmi_ec_mul_batch*)
 *     may be any 256-bit value: the kernels reduce them mod q as they load them (the `% order`
 *     of pippenger.py:26; the Python wrapper also does it, with the length check of :23-24).
 *     The mod-q entry points (bpmi_sc_*, the a / b vectors and challenges of bpmi_ipa_*) expect
 *     values in [0, q);
 *   - every function returns 0 on success or a negative BPMI_E_* code, never
 *     throws, never aborts; bpmi_last_error(ctx) gives the message
 *     (ctx == NULL: the message of the last failed bpmi_ctx_create);
 *   - a ctx is for use by one thread at a time; distinct ctxs are independent;
 *   - a ctx, the objects made from it and the library's host worker threads do not survive fork(): a child process creates
 *     its own ctx (the HIP runtime does not survive a fork either);
 *   - points handed in through HOST pointers are checked to be the identity or on the curve (option "validate_points", default 1;
 *     BPMI_E_ARG names the first bad index and no result is written: a 64-byte result is zeroed).  Points behind DEVICE pointers are the caller's
 *     responsibility unless the option is 2: each must be 64 zero bytes or (x, y) with x, y < p and y^2 = x^3 + 7; anything else
 *     gives an unspecified (never out-of-bounds) result;
 *   - `*_dev` variants take DEVICE pointers (hipMalloc'd, or torch tensors'
 *     data_ptr()) on the ctx's device and enqueue on the ctx's stream; results
 *     written to host pointers are complete when the call returns;
 *   - there is NO CPU fallback: without a usable gfx950 device bpmi_ctx_create
 *     fails with BPMI_E_NODEVICE.
 */
#ifndef BPMI_H
#define BPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPMI_OK 0
#define BPMI_E_NODEVICE -1   /* no HIP device / wrong architecture */
#define BPMI_E_HIP -2        /* a HIP runtime call failed (message has the call) */
#define BPMI_E_ARG -3        /* bad argument (NULL pointer, n too large, ...) */
#define BPMI_E_NOMEM -4      /* device or host allocation failed */
#define BPMI_E_STATE -5      /* call not valid in the object's current state */

#define BPMI_MAX_N (1ull << 26) /* largest supported vector length */

typedef struct bpmi_ctx bpmi_ctx;
typedef struct bpmi_ipa bpmi_ipa;
typedef struct bpmi_rp_prover bpmi_rp_prover;
typedef struct bpmi_ipa_batch_prover bpmi_ipa_batch_prover;

/* ---- library / context ---------------------------------------------------- */
int bpmi_version(void);
/* number of visible HIP devices (0 if none); does not initialise a device */
int bpmi_device_count(void);
/* `stream`: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream),
 * or NULL for a stream owned by the ctx.  Returns NULL on failure.
 * One ctx drives ONE device.  A multi-GPU caller creates one ctx per device (one process per GPU is
 * what the Python side and bench.py do; a single C process may equally hold several ctxs, one thread
 * each) and folds the 64-byte partial results itself (bpmi_ec_sum): the library has no multi-device
 * entry point and no collective of its own.
 * Host memory a ctx allocates lazily: a 32 MB page-locked staging ring at the first upload of 4 KB .. 8 MB
 * from pageable memory (uploads from bpmi_host_alloc memory bypass it), 16 KB of page-locked result
 * buffer per pending-MSM slot. */
bpmi_ctx *bpmi_ctx_create(int device, void *stream);
void bpmi_ctx_destroy(bpmi_ctx *ctx);
const char *bpmi_last_error(const bpmi_ctx *ctx);
int bpmi_sync(bpmi_ctx *ctx);

/* tuning knobs (0 = automatic):
 *   "window_bits"  MSM window bits c in [2,16]
 *   "chunk"        sorted entries added per thread in the accumulate kernel
 *   "tail"         where the O(256) sequential window-combine tail runs: 1 device kernel,
 *                  2 host thread (default; the result is consumed on the host anyway)
 *   "small_n"      largest n that runs on the one-launch small-MSM kernel (-1: never; default 4608)
 *   "split"        1: run one MSM as two window groups on the ctx's two lanes (default 0)
 *   "async_lanes"  1: slot s of bpmi_msm_dev_enqueue runs on the ctx's lane s (own stream and workspace; three lanes), so
 *                  the tail stages of one MSM overlap the sort / accumulate of the next (inputs must be complete
 *                  before the first enqueue of a burst; default 0)
 *   "fused_scan"   1 (default): the accumulate kernel folds the partial results of the 64 threads of a wave itself (two
 *                  records per wave go to the segmented scan); 0: two records per thread (round 3; kept for A/B runs and tests)
 *   "rp_lanes"     bpmi_rp_batch_prepare_dev: proofs per 64-lane wave (power of two; 0 = 64, the fastest measured)
 *   "rp_only_role" profiling only: 0..3 runs just that role of the preparation kernel (Protocol-2 hash chain | the other
 *                  transcript checks | inversion and factor tables | inverse-free scalars); such a call reports proof 0 as bad
 *                  whatever it saw, so it can never pass for a verification; -1 (default) all four
 *   "rp_overlap"   0 (measurements only): the point decoding runs BEHIND the preparation kernels instead of beside them, and the
 *                  upload is not sliced: every kernel's duration is then its own; 1 default
 *   "glv"          1: the bucket pipeline runs on GLV-split scalars (2n pairs of 128-bit scalars, half the windows).  An
 *                  experiment that lost (profiles/r03_glv_msm_on_off.txt); default 0 = off
 *   "priority"     the MSM's stages around the accumulation raise their waves' issue priority (s_setprio 3): 0 none, 1 (default from round 6) all of
 *                  them, 16 + mask the stages of the mask (1 sort, 2 segmented scan, 4 stage 1 of the bucket reduction, 8 its finish).  Beside round
 *                  3's one-round accumulation it lost (profiles/r03_wave_priority_ab.txt); beside the multi-round one ("rounds") it gains 2-8 %
 *                  with two MSMs in flight (profiles/r06_wave_priority_and_chunk_ab.txt)
 *   "rounds"       where another MSM's kernels run beside an accumulation (the asynchronous pipeline, the slices of a large MSM, a synchronous
 *                  pair from 2^19 pairs) its chunk length is ceil(W n / (64 x 3072 x rounds)), at least 20: `rounds` rounds of three waves per
 *                  SIMD.  0 (default) 3; 1: rounds 2-5's one-round accumulation (86 entries at 2^20).  "pair_rounds" = 1 keeps one round for pairs
 *   "accum_runs"   the bucket accumulation as ONE whole bucket run per thread, the non-empty buckets in order of their run length (k_accum_runs
 *                  behind a counting sort of the buckets, csrc/msm_kernels.hpp) instead of chunks of equal length with a segmented scan behind:
 *                  0 never, 1 (default) where the LDS sort runs with 16-bit windows on a whole MSM of 2^19 pairs or more, 2 wherever the LDS
 *                  sort runs (tests).  The device decides per MSM: when some run is longer than the cap the chunked accumulation does the work
 *                  (both are queued every time; the one that is not chosen returns at once).  Never with "glv"
 *   "accum_runs_cap"  that cap: 0 (default) twice the mean run length ceil(n W / G) plus 64, which uniform scalars never reach and every skewed
 *                  distribution passes; otherwise the cap itself, 1 .. 2^30 (tests force either side with it)
 *   "pair_sched"   1: a synchronous pair of MSMs of 2^19 pairs or more as both sorts, then the accumulations one after the other.  Measured
 *                  neutral (profiles/r06_C3_pair_sched_ab.txt); default 0
 *   "accum_stream" / "lane_priority" / "accum_chain"   round-6 experiments on WHERE the pipeline's accumulations are queued (a low-priority stream
 *                  of their own; queue priorities of the lanes; unchained lanes): nothing measurable (profiles/r06_accum_stream_and_chunk_ab.txt); off
 *   "spin_wait"    polls of a completion event before the calling thread sleeps in the runtime (per ctx; default 0)
 *   "mul_batch_glv" bpmi_ec_mul_batch[_dev] from 32 768 points: 1 (default) GLV halves on fixed signed three-bit windows over affine
 *                  3P, 5P, 7P (k_ec_odd_multiples + k_ec_mul_batch_glv; workspace 1 080 B per point of a 196 608-point slice);
 *                  0 the bit-serial ladder at every size
 *   "rp_rows"      bpmi_rp_batch_prepare_dev: proofs per kernel launch (0 = as many as fit ~256 MB of scratch cells)
 *   "ipa_big_m"    base length from which the IPA prover folds its generators 16-way at
 *                  once instead of deferring the fold into the MSM scalars (default 2^18)
 *   "ipa_small_m"  logical length at which bases below "ipa_big_m" are folded once more, through per-term products
 *                  (0 = default 4096, 1 = never, else a power of two; the later rounds then run on the one-launch small-MSM kernel)
 *   "pair_phases"  1: bpmi_msm2 on the bucket pipeline queues both MSMs' sorts before either accumulation.  An experiment that came out
 *                  neutral (profiles/r04_C3_pair_phases_ab.txt); default 0
 *   "prover_table_bits" window bits of the fixed-base tables a bpmi_rp_prover builds, read by bpmi_rp_prover_create: 0 = default, else 4 .. 16
 *                  (wider: fewer additions per scalar multiplication, a larger table -- 16 bits: 64 KB x 32 768 entries per (generator, window),
 *                  4.4 GB and 72 ms to build for 64-bit proofs; 12 bits: 378 MB, 17 ms, 22 % slower proving; profiles/r06_batch_prover_table_bits.txt).
 *                  Default: 16 for proofs of up to 128 elements (bits x values); above, the widest width whose table -- (3 + 2 elements) x
 *                  ceil(256 / w) x 2^(w-1) x 64 B -- is no larger than the 8.7 GB of 128 elements at 16 bits: 14 bits at 256 elements (5.1 GB),
 *                  13 at 512, 12 at 1 024 (csrc/rp_prove_plan_host.hpp)
 *   "prover_job_lanes" lanes bpmi_rp_prove_batch gives a multi-scalar multiplication of a proof: 0 (default) automatic -- 16, and a wave of 64 in
 *                  launches of few jobs of proofs of more than 128 elements (profiles/r07_batch_prover_wide.txt) --, 16 or 64 forced
 *   "rp_priority"  the batch preparation's chain kernels (expander, roles, elements) raise their waves' issue priority: 0 never, 1 (default) on wire
 *                  formats 1 and 2, where the point decoding's square roots run beside them (format 2: a batch alone 1.72 -> 1.66 ms, ten in
 *                  flight +2.4-2.8 %), 2 always (format 3: nothing; profiles/r06_C5_preparation_priority_ab.txt)
 *   "rp_slices"    uploads of a batch of >= 4 096 proofs in bpmi_rp_batch_prepare_dev / bpmi_rp_batch_verify_dev: 1 .. 4, 0 (default) = 4 for wire
 *                  formats 1 and 2 (the points of a slice are decoded on the second lane while the next slice is on the link), 1 for format 3
 *                  (its points are checked, not computed; profiles/r06_C5_upload_slices_ab.txt)
 *   "prover_wire_format" 2 (default) or 3: the wire format bpmi_rp_prove_batch writes (3: with the points' y coordinates, see
 *                  bpmi_rp_wire_v2_to_v1; 32 (6 + 2k) bytes more per proof -- bpmi_rp_prove_batch_proof_bytes counts them)
 *   "ipa_fixed_generators" 1: the generator arrays handed to bpmi_ipa_create_dev are deployment constants.  The tables of odd multiples that
 *                  the prover's 16-way generator fold builds from them (1.1 ms at n = 2^20) are then kept between proofs for as long as the
 *                  calls name the same d_g, d_h and n: the caller's promise that the arrays were not modified.  Default 0
 *   "validate_points" on-curve check of input points: 0 never, 1 (default) every entry point that takes HOST pointers to points (bpmi_msm,
 *                  bpmi_msm2, bpmi_ec_mul_batch, bpmi_ec_lincomb2_batch, bpmi_ec_sum, bpmi_ipa_create[_scaled], the extra points of
 *                  bpmi_ipa_verify_dev, the commitments of bpmi_rp_batch_verify_dev, bpmi_rp_prover_create), 2 also the synchronous entry
 *                  points that take DEVICE pointers (bpmi_msm_dev, the generators of bpmi_ipa_verify_dev and bpmi_rp_batch_verify_dev).
 *                  What fastecdsa's Point constructor does for the reference (reached from /root/reference/src/utils/utils.py:119-131).
 *                  Cost: one kernel behind the upload, no extra wait (profiles/r05_validate_points_cost.txt)
 *   "slice_n"      an MSM of more than "slice_min" pairs (the synchronous entry points: bpmi_msm[_dev], bpmi_msm_segs_dev, the one MSM of
 *                  bpmi_ipa_verify_dev and of the batch verifier) runs as ceil(n / (slice_n 17/16)) equal slices, two in flight on the ctx's
 *                  lanes 0 / 1 with their accumulations chained, the slices' results added on the host: the engine peaks at ~2^20 pairs per
 *                  MSM (profiles/r06_msm_big_n.txt).  0 (default) 2^20; 2^16 .. 2^23; -1: one MSM up to the sort's 2^23-pair limit
 *   "slice_min"    ... the size from which it does: 0 (default) 1.625 x slice_n, the measured crossover of one MSM against two slices
 *   "mid_parts"    blocks per window of the one-block-per-window kernel (k_msm_mid: MSMs of 1 536 .. 8 448 pairs in the inner-product rounds,
 *                  2 560 .. 8 448 one at a time): 0 (default) three from 3 000 pairs, else one; 1 .. 4 forced.  Every part leaves its own window
 *                  sum, the host tail adds them (profiles/r05_mid_kernel_parts_ab.txt: C4's argument 4.05 -> 3.2 ms)
 *   "mixed_windows" 1 (default): window bits c = 10 .. 14 as 256 / c windows of which the last 256 - (256 / c) c are c + 1 bits wide with twice
 *                  the buckets -- the windows cover the 256 bit positions exactly: no carry window, no short top window (13 bits: 10 + 9
 *                  windows) --, and the window table that goes with it (12 bits above the one-block kernel's 8 448 pairs, 13 from 19 000, 16 from 185 000);
 *                  0: uniform windows and the earlier table
 *   "top_window_unsigned" 1 (default): the same for window_bits = 15 (16 + 1 windows); 0: every width uniform, with its carry window
 *   "sort_inblock" 1 (default): up to 2^17 pairs the sort's second level handles partitions of any size in one block (two launches fewer)
 *   "reduce_fit"   1 (default): stage 1 of the bucket reduction gives every sum as many lanes (any number up to 64, not only powers of two)
 *                  as keep its waves within the chip's 1 024 SIMDs at one wave each; 0: round 4's rule (total buckets / 2^15 elements
 *                  per lane, power-of-two groups).  "reduce_epl" > 0 forces the elements per lane
 *   "final_spread" the finish of the bucket reduction (12 dependent point additions on quads of lanes): 0 one 16-wave block per (window,
 *                  array) (k_digit_final_quad: the 16 waves share one CU, 49 us); 3 (default) the 16 second-level sums of every array as
 *                  waves of their own, in blocks of four, and a second launch of one wave per array for the last 8 additions (18 + 21 us);
 *                  2 the same with one-wave blocks; 1 one launch, the wave that draws an array's last ticket runs the finish (60 us: the
 *                  tickets' device-scope fences cost more than the launch they save; profiles/r05_bucket_reduction_finish_ab.txt)
 *   "segscan_fused" / "hist_scan_fused" 1: the segmented scan's last level / the scan of the sort's partition counts run in the block that
 *                  finishes the level / the histogram kernel last (one launch fewer each).  Experiments that lost to the cost of the
 *                  device-scope fence every block needs (profiles/r05_last_block_fusions_ab.txt); default 0
 *   "msm_batch_route" bpmi_msm_batch[_dev[_enqueue]]: 0 (default) the route follows the sizes -- the light shape up to 512 pairs per vector, the
 *                  k_msm_mid shape with ceil(pairs / 8 448) blocks per window up to 25 344 pairs, above that a loop of single MSMs, which
 *                  also runs a batch of fewer than 32 vectors (64 with three blocks per window): the measured crossovers,
 *                  profiles/r10_msm_batch.txt --; 1 / 2 / 3 forces the light shape / the k_msm_mid shape (up to 33 792 pairs) / the loop
 *                  (tests, A/B runs: a forced shape that cannot hold the vectors is BPMI_E_ARG)
 *   "msm_batch_vecs" ... vectors per launch: 0 (default) as many as keep a launch's window sums (vectors x 37 x parts x 144 B) within
 *                  256 MB; a larger batch runs as consecutive launches over row ranges
 *   "fold_wnaf"    the ladder of that 16-way fold: 2 (default) width-4 non-adjacent forms of the coefficients' GLV halves over affine
 *                  tables of 3P, 5P, 7P and of beta x (k_ec_multifold_w4g; 792 B of workspace per generator, kept by the ctx after the first fold),
 *                  1 of the whole coefficients (k_ec_multifold_w4), 0 the plain NAF ladder without tables (k_ec_multifold)
 *   "h2c_plain" / "h2c_per_lane"   the launch shapes of the bulk hash to the curve: see bpmi_ec_hash_batch below
 *   "direct_result" 1 (default): the last kernel of an MSM writes its result into the slot's page-locked host buffer; 0: workspace + copy
 *   "graphs"       1: an MSM's launch sequence is replayed as a HIP graph when the same call comes again; default 0
 *   "hist_threads" / "hist_blocks"   launch shape of the sort's k_coarse_hist: threads per block 256, 512 or 1024, blocks up to 8 192 (0 = default)
 *   "quad_final"   1 (default): the bucket reduction's finish with four-lane point additions (k_digit_final_quad); 0: one lane per point
 *   "tail_thread"  1 (default): the host tail of the second MSM of a synchronous pair runs on the ctx's helper thread beside the first
 *                  one's; 0: one after the other
 *   "pair_chain"   1: a synchronous pair of large MSMs with their accumulate kernels chained as in the asynchronous pipeline (A/B; round 3
 *                  measured it slower); default 0
 *   "small_pair"   1 (default): a pair of small MSMs (bpmi_msm2, the L / R of an inner-product round) as one launch sequence on one
 *                  stream; 0: on two lanes
 *   "mid_min"      a pair of MSMs runs as one launch of k_msm_mid from this many pairs in the larger one (0 = default 1 536, -1 = never)
 *   "mid_single_min"  a single MSM runs on k_msm_mid from this many pairs (0 = default 2 560, -1 = never)
 *   "ipa_small_step" 1: short inner-product vectors run fold, coefficient tables and the next round's dots and scalars in one launch
 *                  (k_ipa_small_step).  Measured slower (profiles/r04_C3_small_step_ab.txt); default 0, kept with its tests
 *   "fold_shared"  1 (default): the product fold of a state without per-generator scales uses shared GLV halves, two terms per thread;
 *                  0: per-lane products
 *   "prover_split" bpmi_rp_prove_batch: 1 = a batch of 4 096 proofs or more as two halves on two lanes, N > 1 = from 2 N proofs.  Measured
 *                  slower (profiles/r06_batch_prover_table_bits.txt); default 0
 * What each option accepts, its message and what a set does beyond storing the value: one row each in csrc/options_host.hpp */
int bpmi_set_option(bpmi_ctx *ctx, const char *name, int64_t value);

/* ---- device buffers (so callers need no other GPU runtime) ------------------- */
int bpmi_malloc(bpmi_ctx *ctx, size_t bytes, void **dptr);
int bpmi_free(bpmi_ctx *ctx, void *dptr);
int bpmi_upload(bpmi_ctx *ctx, void *dptr, const void *host, size_t bytes);
int bpmi_download(bpmi_ctx *ctx, void *host, const void *dptr, size_t bytes);
/* device -> device, enqueued on the ctx stream (ordered with the ctx's other work) */
int bpmi_memcpy_dev(bpmi_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);

/* ---- multi-scalar multiplication ------------------------------------------------
 * out = sum_i scalars[i] * pts[i].
 * Replaces Pippenger.multiexp on EC(secp256k1) = the PipSECP256k1 singleton
 * (src/pippenger/pippenger.py:22-61, src/pippenger/__init__.py:5; group law
 * src/pippenger/group.py:27-32), i.e. every call site listed in SURVEY.md
 * section 8b: src/utils/commitments.py:13, src/innerproduct/inner_product_verifier.py:134,140,
 * src/rangeproofs/rangeproof_prover.py:81, rangeproof_verifier.py:92, ...
 * n == 0 gives the identity (pippenger.py:28-29). */
int bpmi_msm(bpmi_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, uint64_t n, uint8_t out[64]);
int bpmi_msm_dev(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]);
/* The same MSM (n <= 2^23, device pointers) split into an asynchronous pair: `enqueue` queues every kernel
 * and the device->host copy of the window sums on the ctx stream and returns; `finish` waits for that
 * MSM only (its own completion event), runs the host part of the tail and writes the result.  Three slots
 * (0, 1, 2) may be in flight: a caller that rotates them overlaps the host tail -- and its own work between
 * two MSMs, e.g. the exchange of per-GPU partial results -- of MSM k with the kernels of MSM k + 1 (and, three
 * deep with "async_lanes", the sort of MSM k + 2).  The
 * inputs must stay valid and unmodified until `finish`; while a slot is pending, a synchronous call that
 * needs it fails with BPMI_E_STATE. */
int bpmi_msm_dev_enqueue(bpmi_ctx *ctx, int slot, const void *d_pts, const void *d_scalars, uint64_t n);
int bpmi_msm_finish(bpmi_ctx *ctx, int slot, uint8_t out[64]);
/* What an MSM of n pairs runs as under the ctx's current options; no GPU work.  pipelined: 1 = as bpmi_msm_dev_enqueue runs it, 0 = as
 * the synchronous entry points do (which slice large inputs: option "slice_n").  geom[0] kernel family (0 the bucket pipeline, 1 the
 * one-launch kernel, 2 one block per window), [1] window bits c, [2] windows W, [3] how many of them are c + 1 bits wide, [4] buckets,
 * [5] sorted entries per thread of the accumulation, [6] slices K, [7] pairs per slice (the other fields describe ONE slice).
 * The bucket additions of the call are K x W x (pairs per slice); bench.py prices its multiply-adds from this, not from a constant. */
int bpmi_msm_geometry(bpmi_ctx *ctx, uint64_t n, int pipelined, uint32_t geom[8]);
/* Tests: which accumulation the last bucket-pipeline MSM queued on lane `lane` (0 .. 2; synchronous calls use lane 0) ran.  Waits for the
 * lane.  state[0] 1 when the accumulation by runs was planned (option "accum_runs"), [1] the device's flag: 1 = some run was longer than
 * the cap and the chunked accumulation did the work, 0 = k_accum_runs did, [2] the runs it added (non-empty buckets; 0 with the flag up). */
int bpmi_debug_msm_runs(bpmi_ctx *ctx, int lane, uint32_t state[3]);
/* One MSM over up to three (points, scalars) arrays in different device buffers (BPMI_MAX_N pairs in total at most):
 * `multiexp(gs + hs + ..., a + b + ...)` without the list concatenation of src/utils/commitments.py:13. */
int bpmi_msm_segs_dev(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const void *const *d_scalars, const uint64_t *n, uint8_t out[64]);
/* Two independent MSMs (n0, n1 <= 2^23) from host buffers, overlapped on the ctx's two lanes: pairs
 * such as A / S (rangeproof_prover.py:52,60) and T1 / T2 (:71-72) cost one round trip instead of two. */
int bpmi_msm2(bpmi_ctx *ctx, const uint8_t *pts0, const uint8_t *scalars0, uint64_t n0, uint8_t out0[64], const uint8_t *pts1,
              const uint8_t *scalars1, uint64_t n1, uint8_t out1[64]);

/* ---- MANY scalar vectors over ONE shared point set: n_vec multi-scalar multiplications in one launch ----------------
 *   out[v] = sum_s sum_{i < n[s]} scalars[s][v][i] * pts[s][i]        v in [0, n_vec)
 * Replaces a LOOP of Pippenger.multiexp over the same gs (src/pippenger/pippenger.py:22-61) -- the Pedersen vector commitments
 * vector_commitment(gs, hs, a_p, b_p) of many vectors (src/utils/commitments.py:13), the statements P_p = <a_p, g> + <b_p, h> + c_p u
 * of a run of inner-product arguments, the columns of a table under one generator set.  Below ~10^4 pairs such a loop is almost all
 * fixed cost per call; here block (vector, window) of ONE launch runs the one-block-per-window method in LDS and a second launch
 * combines every vector's windows, one lane per vector.
 *   nseg        1 .. 3 segments, as in bpmi_msm_segs_dev; d_pts[s]: n[s] points shared by every vector (n[s] = 0 is allowed, the
 *               segment's pointers are then not read)
 *   d_scalars[s] a row-major matrix of n_vec rows x n[s] scalars of 32 bytes: row v starts at byte v * n[s] * 32
 *   out         HOST, n_vec x 64 bytes, complete on return (bpmi_msm_batch_dev, bpmi_msm_batch)
 *   d_out       DEVICE, n_vec x 64 bytes (bpmi_msm_batch_dev_enqueue): the same work without the wait, ordered on the ctx stream; read it
 *               after bpmi_sync, like bpmi_ec_sum_dev_enqueue's.  (Vectors of more than 25 344 pairs, and batches of fewer than 32
 *               vectors, run as a loop of single MSMs whose tails are the host's: that route waits here too.)
 * Conventions of bpmi_msm: scalars are any 256-bit values, reduced mod q as they are loaded; the identity is 64 zero bytes on input
 * and output; no pairs at all gives n_vec identities; n_vec = 0 is BPMI_OK and touches nothing.  bpmi_msm_batch (one segment, HOST
 * pointers) checks its points under "validate_points" >= 1 exactly as bpmi_msm does (BPMI_E_ARG names the first bad index, out is
 * zeroed); level 2 also checks the points of bpmi_msm_batch_dev.
 * Refused with BPMI_E_ARG before anything is read or allocated, the message naming the bound: nseg outside 1 .. 3, a NULL pointer, more
 * than BPMI_MAX_N pairs per vector, n_vec > 2^20, n_vec x pairs > 2^30.  The calls use the workspace of the ctx's first lane: while an
 * asynchronous MSM is pending in a slot that lives there (slot 0; every slot without "async_lanes") they fail with BPMI_E_STATE.
 * Routes and launch shapes: csrc/msm_batch_plan_host.hpp; options "msm_batch_route", "msm_batch_vecs". */
int bpmi_msm_batch(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, const uint8_t *scalars, uint64_t n_vec, uint8_t *out);
int bpmi_msm_batch_dev(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const uint64_t *n, const void *const *d_scalars, uint64_t n_vec, uint8_t *out);
int bpmi_msm_batch_dev_enqueue(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const uint64_t *n, const void *const *d_scalars, uint64_t n_vec,
                               void *d_out);

/* ---- fixed-base MSM: an object that owns a point set and a table of its multiples ------------------------------------
 *   out = sum_{i < n_scalars} scalars[i] * P_i        over the object's points P_0 .. P_{n-1}, n_scalars <= n
 * Replaces Pippenger.multiexp(gs, es) (src/pippenger/pippenger.py:22-61) and vector_commitment(gs, hs, a, b)
 * (src/utils/commitments.py:13) where gs (gs + hs) is a list of generators that never changes: the object keeps
 * T[r][i] = 2^(c Wv r) P_i for r < R, so the W windows of c bits of a scalar become entries for R table points in only
 * Wv = ceil(W / R) windows -- as many bucket additions, and the bucket reduction and the tail over Wv windows instead of W.
 *   bpmi_fixed_base_create[_dev]  pts: n x 64 bytes (HOST / DEVICE), copied: the caller may free them.  window_bits: 0 or 10 .. 16 (W =
 *                           255 / window_bits + 1 uniform signed windows); rows: 0 or 1 .. W, Wv = ceil(W / rows), and the effective row
 *                           count ceil(W / Wv) is what info reports.  rows = 1 keeps a copy of the points and runs as an ordinary MSM of the
 *                           given width.  (0, 0): automatic, by the measured rule of csrc/msm_fixed_plan_host.hpp (one of the two 0: that
 *                           one is chosen around the other); an explicit value is never overridden.  Refused with BPMI_E_ARG before
 *                           anything is read or allocated, the message naming the bound: n = 0, n > BPMI_MAX_N, n x rows > 2^23 (the
 *                           sort's packed entry holds a 23-bit pair index; automatic rows are lowered until it holds), window_bits or rows
 *                           out of range, a NULL pointer.  A table that does not fit the device is BPMI_E_NOMEM.  The points are checked to be
 *                           on the curve under "validate_points" (create at level >= 1, create_dev at level 2): BPMI_E_ARG names the
 *                           first bad index.  The identity, equal and opposite points are legal.
 *   bpmi_fixed_base_info    info[0] n, [1] window bits c, [2] windows W, [3] rows R (effective), [4] virtual windows Wv, [5] table bytes,
 *                           [6] build time in microseconds, [7] 0.  c = W = Wv = 0 with R = 1: the automatic rule chose the ordinary MSM
 *                           under the ctx's own options.
 *   bpmi_fixed_base_table   count entries of row `row` from index `first` to HOST memory, 64 bytes each, affine and canonical, the identity
 *                           64 zero bytes (tests, debugging)
 *   bpmi_msm_fixed[_dev]    scalars: n_scalars x 32 bytes (HOST / DEVICE), any 256-bit values, reduced mod q on load; the missing n -
 *                           n_scalars scalars count as 0 (n_scalars > n: BPMI_E_ARG); n_scalars = 0 gives the identity and runs no GPU work.
 *                           The result is affine and canonical: the bytes of bpmi_msm_dev over the same points and zero-padded scalars.
 *   bpmi_msm_fixed_dev_enqueue   the asynchronous form, finished by bpmi_msm_finish(ctx, slot, out) of the object's ctx.
 * The object uses its ctx's lanes, workspace and pending slots exactly as bpmi_msm_dev / bpmi_msm_dev_enqueue do (the BPMI_E_STATE rules
 * and "async_lanes" included; the scalars stay valid until `finish`).  One thread at a time per ctx; destroy the object before its ctx. */
typedef struct bpmi_fixed_base bpmi_fixed_base;
int bpmi_fixed_base_create(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, uint32_t window_bits, uint32_t rows, bpmi_fixed_base **out);
int bpmi_fixed_base_create_dev(bpmi_ctx *ctx, const void *d_pts, uint64_t n, uint32_t window_bits, uint32_t rows, bpmi_fixed_base **out);
void bpmi_fixed_base_destroy(bpmi_fixed_base *fx);
int bpmi_fixed_base_info(const bpmi_fixed_base *fx, uint64_t info[8]);
int bpmi_fixed_base_table(bpmi_fixed_base *fx, uint32_t row, uint64_t first, uint64_t count, uint8_t *out);
int bpmi_msm_fixed(bpmi_fixed_base *fx, const uint8_t *scalars, uint64_t n_scalars, uint8_t out[64]);
int bpmi_msm_fixed_dev(bpmi_fixed_base *fx, const void *d_scalars, uint64_t n_scalars, uint8_t out[64]);
int bpmi_msm_fixed_dev_enqueue(bpmi_fixed_base *fx, int slot, const void *d_scalars, uint64_t n_scalars);

/* ---- batched point operations ----------------------------------------------------
 * out[i] = scalars[i] * pts[i]      replaces `ModP * Point` / `int * Point`
 * (src/utils/utils.py:43-44), e.g. hsp[i] = y^-i * hs[i]
 * (src/rangeproofs/rangeproof_prover.py:77, rangeproof_verifier.py:72). */
int bpmi_ec_mul_batch(bpmi_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, uint64_t n, uint8_t *out);
int bpmi_ec_mul_batch_dev(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, void *d_out);
/* out[i] = k1 * p1[i] + k2 * p2[i]   replaces the generator fold
 * g' = x^-1 * g_lo + x * g_hi (src/innerproduct/inner_product_prover.py:107-108). */
int bpmi_ec_lincomb2_batch(bpmi_ctx *ctx, const uint8_t *p1, const uint8_t *p2, const uint8_t k1[32],
                           const uint8_t k2[32], uint64_t n, uint8_t *out);
int bpmi_ec_lincomb2_batch_dev(bpmi_ctx *ctx, const void *d_p1, const void *d_p2, const uint8_t k1[32],
                               const uint8_t k2[32], uint64_t n, void *d_out);
/* out = sum_i pts[i]                 replaces chains of `Point + Point`
 * (fastecdsa Point.__add__; e.g. `A + x*S + multiexp(...)`, rangeproof_prover.py:78-87),
 * and folds the per-GPU partial results of a sharded MSM. */
int bpmi_ec_sum(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, uint8_t out[64]);
/* the same for points already in device memory (e.g. the receive buffer of an all_gather) */
int bpmi_ec_sum_dev(bpmi_ctx *ctx, const void *d_pts, uint64_t n, uint8_t out[64]);
/* ... and without the wait: the sum goes to d_out (64 bytes of device memory), ordered on the ctx stream; read it after bpmi_sync */
int bpmi_ec_sum_dev_enqueue(bpmi_ctx *ctx, const void *d_pts, uint64_t n, void *d_out);

/* out[i] = the point encoded by comp[33*i .. 33*i+33) in SEC1 compressed form (0x02 | 0x03,
 * then x big-endian; 33 zero bytes = identity); ok[i] = 1 when the encoding is valid
 * (known tag, x < p, x^3 + 7 a square), else out[i] = identity and ok[i] = 0.
 * Replaces bytes_to_point / b64_to_point (src/utils/utils.py:114-131) in bulk, e.g. for
 * the 19 points of every proof of a batch that arrives as bytes. */
int bpmi_ec_decompress_batch(bpmi_ctx *ctx, const uint8_t *comp, uint64_t n, uint8_t *out, uint8_t *ok);
/* the same with the decoded points left on the device (d_out: n x 64 bytes of device memory), ready to be MSM input */
int bpmi_ec_decompress_batch_dev(bpmi_ctx *ctx, const uint8_t *comp, uint64_t n, void *d_out, uint8_t *ok);

/* ---- bulk hash to the curve: the generators of every protocol, derived on the device ----------------
 * out[i] = elliptic_hash(message i) of the reference (src/utils/elliptic_curve_hash.py:7-23), try and increment: the counters
 * c = 1, 2, ... are tried in turn, pre = str(c) || message (decimal ASCII, no padding), x = SHA-256(pre) read big-endian; x >= p
 * or x^3 + 7 not a square: the next c.  The sign rule: with r = (x^3 + 7)^((p+1)/4) and bit = the low bit of the last byte of
 * MD5(pre), the point is (x, r) when bit = 1, else (x, p - r) -- chosen by MD5 of the same prefixed message and by which root
 * the exponentiation returns, NOT by the parity of y.  Under these generators, and only these, proofs interoperate with the
 * reference's.
 *   batch form   message i = msgs[msg_off[i] .. msg_off[i + 1]), msg_off: n + 1 offsets
 *   range form   message i = str(lo + i) || tail[0 .. tail_len), i in [0, hi - lo): the idiom
 *                [elliptic_hash(str(i).encode() + seed, CURVE) for i in range(n)] of the reference's tests and main; only the tail
 *                is uploaded
 * max_tries: the candidates a message gets at most, 1 .. 255; 0 means 255 (the chance of a message needing more is 2^-255).
 * tries (n bytes, may be NULL): tries[i] = the counter that succeeded, or 0 when none did within max_tries -- out[i] is then 64
 * zero bytes.  With tries == NULL a message without a point fails the call with BPMI_E_STATE naming the first such index (an
 * identity must never pass silently for a generator); with tries given the call is BPMI_OK and the caller reads the flags.
 * Refused with BPMI_E_ARG before any message is read or anything is allocated: n > BPMI_MAX_N, a message of more than 65 535
 * bytes, decreasing offsets, more than 4 GiB of messages, tail_len > 65 535, anything but lo <= hi <= 2^32, max_tries > 255.
 * n = 0 (lo == hi) is BPMI_OK and touches nothing.  out: n x 64 bytes in the point format above; the _dev forms leave the points in
 * device memory (d_out: n x 64 bytes), ready to be the g / h of bpmi_ipa_create_dev, bpmi_ipa_verify_dev, bpmi_msm_dev or the batch
 * verifier.  Ordered on the ctx stream, and complete on return, like bpmi_ec_decompress_batch[_dev].
 * A call of up to 196 608 messages runs one message per lane with a loop per lane; a larger one gives every wave a span of several
 * messages per lane and a lane takes the span's next message when its own is done (profiles/r09_hash_to_curve.txt).  Options for A/B
 * runs and tests: "h2c_plain" = 1 forces the loop per lane at every size; "h2c_per_lane" = 1 .. 64 forces the queue with that many
 * messages per lane (0 = by the call's size). */
int bpmi_ec_hash_batch(bpmi_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint32_t max_tries, uint8_t *out, uint8_t *tries);
int bpmi_ec_hash_batch_dev(bpmi_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint32_t max_tries, void *d_out, uint8_t *tries);
int bpmi_ec_hash_range(bpmi_ctx *ctx, const uint8_t *tail, uint64_t tail_len, uint64_t lo, uint64_t hi, uint32_t max_tries, uint8_t *out, uint8_t *tries);
int bpmi_ec_hash_range_dev(bpmi_ctx *ctx, const uint8_t *tail, uint64_t tail_len, uint64_t lo, uint64_t hi, uint32_t max_tries, void *d_out, uint8_t *tries);

/* ---- bulk scalar (mod q) operations ------------------------------------------------
 * out = sum_i a[i] * b[i] mod q       replaces inner_product (src/utils/utils.py:134-137) */
int bpmi_sc_dot(bpmi_ctx *ctx, const uint8_t *a, const uint8_t *b, uint64_t n, uint8_t out[32]);
int bpmi_sc_dot_dev(bpmi_ctx *ctx, const void *d_a, const void *d_b, uint64_t n, uint8_t out[32]);
/* out[i] = x * lo[i] + y * hi[i] mod q  replaces the a / b fold
 * (src/innerproduct/inner_product_prover.py:109-110) */
int bpmi_sc_fold(bpmi_ctx *ctx, const uint8_t *lo, const uint8_t *hi, const uint8_t x[32], const uint8_t y[32],
                 uint64_t n, uint8_t *out);
int bpmi_sc_fold_dev(bpmi_ctx *ctx, const void *d_lo, const void *d_hi, const uint8_t x[32], const uint8_t y[32],
                     uint64_t n, void *d_out);

/* The verifier's s-vector with the proof's final scalars folded in, n = 2^k entries each:
 *   s_i = prod_j xs[j]^(+1 if bit (k-1-j) of i is set, else -1)   (Verifier2.get_ss,
 *   src/innerproduct/inner_product_verifier.py:91-102),  sa[i] = a s_i,  sb[i] = b s_i^-1 scale[i]
 * (the `a * s_i` / `b * s_i^-1` lists of :131-133; scale: n scalars or NULL -- hsp_i = y^-i hs_i of
 * src/rangeproofs/rangeproof_verifier.py:72 rides in the scalars).  xs, xinvs: k challenges and their
 * inverses.  2-3 multiplications per element on the device instead of the reference's k per element. */
int bpmi_sc_svector(bpmi_ctx *ctx, const uint8_t *xs, const uint8_t *xinvs, uint32_t k, const uint8_t a[32], const uint8_t b[32],
                    const uint8_t *scale, uint8_t *sa, uint8_t *sb);

/* Verifier2.verify's two sides (src/innerproduct/inner_product_verifier.py:127-147) as ONE multi-scalar
 * multiplication over generators that are already in device memory (n = 2^k points each, d_hscale: n scalars or NULL):
 *   out = sum_i sa[i] g_i + sum_i sb[i] h_i + sum_t extra_scalars[t] * extra_pts[t]
 * with sa, sb as in bpmi_sc_svector, computed on the device and consumed there (no host loop over n, no
 * round trip of the 2n scalars).  The caller passes u, the L_j, R_j and P with their scalars
 * (a b, -x_j^2, -x_j^-2, -1) as the extra terms and accepts iff out is the identity (64 zero bytes). */
int bpmi_ipa_verify_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, const uint8_t *xs,
                        const uint8_t *xinvs, uint32_t k, const uint8_t a[32], const uint8_t b[32], const uint8_t *extra_pts,
                        const uint8_t *extra_scalars, uint64_t n_extra, uint8_t out[64]);

/* ---- a BATCH of inner-product proofs over the same generators in one MSM ----------------
 * Verifier2.verify's check (/root/reference/src/innerproduct/inner_product_verifier.py:127-147) is one equation per proof p,
 *   sum_i a_p s_{p,i} g_i + sum_i b_p s_{p,i}^-1 c_i h_i + a_p b_p u_p - P_p - sum_j (x_{p,j}^2 L_{p,j} + x_{p,j}^-2 R_{p,j}) = 0
 * with s_{p,i} as in bpmi_sc_svector (get_ss, :91-102).  Multiplied by a random weight w_p each and added up, the generator terms
 * of all proofs collapse to 2n pairs with the scalars
 *   SA_i = sum_p w_p a_p s_{p,i},   SB_i = c_i sum_p w_p b_p s_{p,i}^-1
 * so n_proofs proofs cost n_proofs x n x 2 multiplications mod q and ONE multi-scalar multiplication instead of one each.  The two
 * equalities of Verifier1 (:44-58: P_new = P + x c u, u_new = x u) are point equations too and can ride along as extra pairs under
 * weights of their own.  The weights must be unpredictable to whoever made the proofs: with known weights the errors of two
 * invalid proofs can be made to cancel.
 * Per call: n = 2^k with k <= 22; 1 <= n_proofs <= 2^16; n_proofs x n <= 2^32; the half tables (n_proofs x 64 (2^(k/2) + 2^(k - k/2))
 * bytes) at most 1 GiB; at most 2^22 extra points.  A call outside these bounds is refused with BPMI_E_ARG before anything is read
 * or allocated.  One call at a time per ctx.
 *
 * SA, SB of a batch, to host memory (the testable half, as bpmi_sc_svector is for bpmi_ipa_verify_dev).  xs, xinvs: n_proofs x k x 32
 * bytes; a, b, weights: n_proofs x 32 bytes, values in [0, q); scale: n x 32 bytes or NULL; sa, sb: n = 2^k scalars each. */
int bpmi_sc_svector_sum(bpmi_ctx *ctx, uint32_t k, uint64_t n_proofs, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a,
                        const uint8_t *b, const uint8_t *weights, const uint8_t *scale, uint8_t *sa, uint8_t *sb);
/* The whole batch over generators in device memory (n points each, d_hscale: n scalars or NULL):
 *   out = sum_i SA_i g_i + sum_i SB_i h_i + sum_t extra_scalars[t] * extra_pts[t]
 * the identity (64 zero bytes) iff every weighted equation holds.  The caller passes every proof's u, L_j, R_j and P as extra points
 * with the scalars (a b, -x_j^2, -x_j^-2, -1) ALREADY multiplied by that proof's weight: the library does not know which extra
 * point belongs to which proof.  Points are checked as in bpmi_ipa_verify_dev (option "validate_points": the extra points at
 * level 1, the generators at level 2); a call refused for a point leaves 0xFF.. in out, never the identity. */
int bpmi_ipa_verify_batch_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, uint64_t n_proofs,
                              const uint8_t *xs, const uint8_t *xinvs, uint32_t k, const uint8_t *a, const uint8_t *b,
                              const uint8_t *weights, const uint8_t *extra_pts, const uint8_t *extra_scalars, uint64_t n_extra,
                              uint8_t out[64]);

/* ---- a batch of inner-product proofs of DIFFERENT lengths over the prefixes of one generator list, in one MSM ----------------
 * A generator list is a capacity: a statement of n_p = 2^k_p elements is made over g[:n_p], h[:n_p] (and c[:n_p]), and its verifier is
 * Verifier2 over those prefixes (src/innerproduct/inner_product_verifier.py:127-147), with s_{p,i} from the proof's own k_p challenges
 * (get_ss, :91-102; MSB first over k_p bits).  Under the weights of bpmi_ipa_verify_batch_dev generator i collects the proofs that
 * reach it:
 *   SA_i = sum_{p : n_p > i} w_p a_p s_{p,i},   SB_i = c_i sum_{p : n_p > i} w_p b_p s_{p,i}^-1,   i < n_top = max_p n_p
 * so proofs of 64, 256 and 4 096 elements are ONE MSM of 2 n_top + (extra pairs) and sum_p n_p x 2 multiplications mod q, not one
 * batch per length.  The MSM reads the first n_top generators only.
 *   n_gens       the capacity: 2^K points in d_g and d_h each (scalars in scale / d_hscale), K <= 22
 *   ks           n_proofs round counts k_p, in any order; every k_p <= K
 *   xs, xinvs    sum_p k_p x 32 bytes: proof after proof in the order of ks, each proof's k_p challenges (NULL allowed when every k_p = 0)
 *   a, b, weights   n_proofs x 32 bytes, values in [0, q), in the order of ks
 * Per call: 1 <= n_proofs <= 2^16; sum_p n_p <= 2^32; the half tables (64 (2^(k_p/2) + 2^(k_p - k_p/2)) bytes per proof) at most 1 GiB; at
 * most 2^22 extra points.  A call outside these bounds is refused with BPMI_E_ARG before anything is allocated.  One call at a time per ctx.
 *
 * SA, SB of a mixed batch, to host memory.  scale: n_gens x 32 bytes (the first n_top are read) or NULL; sa, sb: room for
 * n_top = 2^max(k_p) scalars each; *n_top: that count.  For proofs of ONE length the bytes are those of bpmi_sc_svector_sum. */
int bpmi_sc_svector_sum_mixed(bpmi_ctx *ctx, uint64_t n_gens, uint64_t n_proofs, const uint32_t *ks, const uint8_t *xs, const uint8_t *xinvs,
                              const uint8_t *a, const uint8_t *b, const uint8_t *weights, const uint8_t *scale, uint8_t *sa, uint8_t *sb,
                              uint64_t *n_top);
/* The whole mixed batch over generators in device memory (n_gens points each, d_hscale: n_gens scalars or NULL):
 *   out = sum_{i < n_top} SA_i g_i + sum_{i < n_top} SB_i h_i + sum_t extra_scalars[t] * extra_pts[t]
 * the identity (64 zero bytes) iff every weighted equation holds.  The extra pairs follow the contract of bpmi_ipa_verify_batch_dev:
 * already multiplied by their proof's weight, the library does not know their owner.  Points are checked as there (option
 * "validate_points": the extra points at level 1, the first n_top generators at level 2); a call refused for a point leaves 0xFF.. in
 * out, never the identity. */
int bpmi_ipa_verify_batch_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, uint64_t n_proofs,
                                    const uint32_t *ks, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a, const uint8_t *b,
                                    const uint8_t *weights, const uint8_t *extra_pts, const uint8_t *extra_scalars, uint64_t n_extra,
                                    uint8_t out[64]);

/* ---- inner-product argument prover, split at the Fiat-Shamir edge ----------------------
 * One object = one run of FastNIProver2.prove (src/innerproduct/inner_product_prover.py:70-110).
 * g, h: n points; a, b: n scalars; u: one point; all copied to the device once and kept
 * there.  a and b are halved in place every round; the generator fold is DEFERRED: L and R
 * are MSMs over the unfolded generators with the fold coefficients multiplied into the
 * scalars (the prover's outputs never contain the folded generators), and large bases are
 * materialised 16-way at once.
 *   bpmi_ipa_round_LR : cl, cr, L, R of the current round          (:96-99)
 *   --- host: transcript.add_list_points([L, R]); x = H(transcript) (:102-106) ---
 *   bpmi_ipa_fold     : g, h, a, b <- folded with x, x^-1           (:107-110)
 *   bpmi_ipa_finish   : the final a[0], b[0]                         (:85-94)     */
int bpmi_ipa_create(bpmi_ctx *ctx, const uint8_t *g, const uint8_t *h, const uint8_t *a, const uint8_t *b,
                    uint64_t n, const uint8_t u[64], bpmi_ipa **out);
int bpmi_ipa_create_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_a, const void *d_b,
                        uint64_t n, const uint8_t u[64], bpmi_ipa **out);
/* As bpmi_ipa_create, for the generators h_scale[i] * h[i] (h_scale: n scalars, or NULL):
 * the range-proof provers run the argument over hsp[i] = y^-i * hs[i]
 * (src/rangeproofs/rangeproof_prover.py:77,88); the factors are multiplied into the MSM
 * scalars instead of n point multiplications (large n: one batched multiplication). */
int bpmi_ipa_create_scaled(bpmi_ctx *ctx, const uint8_t *g, const uint8_t *h, const uint8_t *a, const uint8_t *b,
                           uint64_t n, const uint8_t u[64], const uint8_t *h_scale, bpmi_ipa **out);
uint64_t bpmi_ipa_len(const bpmi_ipa *st);
int bpmi_ipa_round_LR(bpmi_ipa *st, uint8_t L[64], uint8_t R[64]);
int bpmi_ipa_fold(bpmi_ipa *st, const uint8_t x[32], const uint8_t xinv[32]);
/* the whole halving loop in one call, Fiat-Shamir included: rounds of (L, R) -> transcript items -> x = mod_hash(transcript, q) -> fold
 * until the state has length 1 (inner_product_prover.py:94-110, utils.py:84-97).  digest: the transcript so far; digest_out
 * (capacity cap): the transcript after the last round; xs / Ls / Rs: 32 / 64 / 64 bytes per round, max_rounds entries each. */
int bpmi_ipa_prove_rounds(bpmi_ipa *st, const uint8_t *digest, uint64_t digest_len, uint8_t *digest_out, uint64_t cap, uint64_t *out_len, uint8_t *xs,
                          uint8_t *Ls, uint8_t *Rs, uint32_t max_rounds, uint32_t *rounds);
int bpmi_ipa_finish(bpmi_ipa *st, uint8_t a[32], uint8_t b[32]);
/* The CURRENT (folded) g, h (len points each) and a, b (len scalars each), len = bpmi_ipa_len:
 * what the reference holds in gp, hp, ap, bp at the top of its loop (:84).  With folds
 * deferred, every generator costs one MSM, so this is meant for short states (len <= 64):
 * a prover sharded over GPUs hands its last element to the other ranks through it. */
int bpmi_ipa_export(bpmi_ipa *st, uint8_t *g, uint8_t *h, uint8_t *a, uint8_t *b);
void bpmi_ipa_destroy(bpmi_ipa *st);

/* ---- batch verification of range proofs: host-side preparation (no GPU work, no ctx) ---------------
 * For n_proofs range proofs -- values_per_proof = 1: single-value proofs; m > 1: aggregated proofs of m values
 * each, n_gens = m x bits -- over n_gens generator pairs in the wire format of
 * python-bulletproofs_amd/rangeproofs/codec.py (blob i = blobs[blob_off[i] .. blob_off[i+1]); the offsets must be
 * non-decreasing and end inside blobs[0 .. blobs_len), else BPMI_E_ARG):
 * parses every proof, runs the byte-level transcript checks of RangeVerifier / Verifier1 / Verifier2
 * (src/rangeproofs/rangeproof_verifier.py:42-53, src/innerproduct/inner_product_verifier.py:31-43,
 * 104-125) and computes, with the caller's random weights (4 scalars per proof, LE, in [1, q); or weights = NULL and
 * a fresh random 32-byte `seed`: the weights are then derived inside, SHA-256(seed || proof index || 0..3) cut to 248 bits), the
 * scalars of the ONE multi-scalar multiplication that is the identity iff every proof verifies:
 *   v_scalars   n_proofs x values_per_proof x 32 B   for the commitments V_i (V_i,0 .. V_i,m-1)
 *   pt_scalars  n_proofs x (6 + 2k) x 32 B, k = log2 n_gens, for each proof's points in wire order
 *               (T1 T2 A S u_new P_new L_1..L_k R_1..R_k)
 *   shared      (5 + 2 n_gens) x 32 B: coefficients of g, h, u, the constant added to every gs_i and
 *               to every hs_i, then of gs_0.. and hs_0..
 *   comp_out    (optional, may be NULL) n_proofs x (6 + 2k) x 33 B: the proofs' compressed points, gathered
 *               in the same order, ready for bpmi_ec_decompress_batch
 * *first_bad = index of the first proof that failed parsing or a transcript check, or -1.  `threads`
 * host threads share the proofs.  The native twin of BatchRangeVerifier.add (rangeproofs/batch.py). */
int bpmi_rp_batch_prepare(uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off,
                          const uint8_t *weights, const uint8_t *seed, int threads, uint8_t *v_scalars, uint8_t *pt_scalars, uint8_t *shared, uint8_t *comp_out, int64_t *first_bad);

/* out[i - lo] = mod_hash(str(i) || tail, q) for i in [lo, hi), 32 bytes little-endian each -- the reference's seeded
 * challenge / blinding derivation (src/utils/utils.py:84-97: the first counter c >= 1 with SHA-256(str(c) || msg) in [1, q)),
 * in bulk: the range-proof provers draw 2 n m blinding scalars this way (rangeproof_prover.py:57-60).  Host code. */
int bpmi_mod_hash_range(const uint8_t *tail, uint64_t tail_len, uint64_t lo, uint64_t hi, int threads, uint8_t *out);

/* The O(n m) scalar algebra of the range-proof provers and verifiers in native HOST code (csrc/rp_algebra_host.hpp; no elliptic-curve
 * arithmetic, no GPU): vectors of scalars mod q in and out, 32 bytes little-endian each, `threads` host threads.  aL: one byte per
 * bit (0 / 1); n bits per value, m values (m = 1 and aggregated = 0: the single proof's z^2 2^i terms).
 *   bpmi_rp_poly_coeffs       t1, t2 of `_get_polynomial_coeffs` (src/rangeproofs/rangeproof_prover.py:93-101,
 *                             rangeproof_aggreg_prover.py:117-130)
 *   bpmi_rp_final_vectors     l, r, t_hat of `_final_compute` (:103-112 / :132-146), plus yscale_i = y^-i and
 *                             hsc_i = (z y^i + zt_i) y^-i: the hs-scalars of P (:78-87 / :95-101) over the UNSCALED generators
 *   bpmi_rp_verifier_vectors  yscale, hsc as above and ysum = sum_{i < n m} y^i for delta(y, z) (rangeproof_verifier.py:55-99,
 *                             rangeproof_aggreg_verifier.py:55-108) */
int bpmi_rp_poly_coeffs(uint32_t n, uint32_t m, int aggregated, const uint8_t *aL, const uint8_t *sL, const uint8_t *sR, const uint8_t y[32],
                        const uint8_t z[32], int threads, uint8_t t1[32], uint8_t t2[32]);
int bpmi_rp_final_vectors(uint32_t n, uint32_t m, int aggregated, const uint8_t *aL, const uint8_t *sL, const uint8_t *sR, const uint8_t y[32],
                          const uint8_t z[32], const uint8_t x[32], int threads, uint8_t *ls, uint8_t *rs, uint8_t t_hat[32], uint8_t *hsc, uint8_t *yscale);
int bpmi_rp_verifier_vectors(uint32_t n, uint32_t m, int aggregated, const uint8_t y[32], const uint8_t z[32], int threads, uint8_t *hsc, uint8_t *yscale,
                             uint8_t ysum[32]);

/* Wire format 2 of a range proof (csrc/rp_wire_v2_host.hpp, rangeproofs/codec.py): format 1 without the three transcripts -- they
 * are functions of the other fields (/root/reference/src/utils/transcript.py:13-33, rangeproof_verifier.py:42-53) -- plus the four
 * challenges y, z, x, x_ip in binary and the two transcript seeds: 1.09 KB instead of 2.56 KB for a 64-bit proof.  This entry point
 * expands n_proofs format-2 proofs (proof g = blobs[off[g], off[g + 1])) into format-1 proofs packed in out[0, cap), out_off[0 ..
 * n_proofs]; HOST code.  *first_bad = first proof that is not a well-formed format-2 proof, or -1.  bpmi_rp_batch_prepare_dev and
 * bpmi_rp_batch_verify_dev take EITHER format (all proofs of a call in the same one, told by the magic of the first): format 2 is
 * uploaded as it is and expanded on the device.  A format-2 proof is valid exactly when its expansion is.
 * Wire format 3 (round 6) is a format-2 proof with the magic "BPRP3", followed by the y coordinate of each of its 6 + 2k points (32 B
 * big-endian, 0 for the identity; 1.67 KB for a 64-bit proof).  The verifiers CHECK each y -- below p, the parity of the encoding's
 * tag, on the curve with x: then it is the y a decompression would compute -- instead of taking 6 + 2k square roots per proof, which
 * were a quarter of a batch verification's device time.  A format-3 proof is valid exactly when its format-2 part is and every y is
 * right; a wrong y is an invalid proof (*first_bad names it).  This entry point and the three batch entry points take format 3
 * wherever they take format 2; bpmi_rp_prove_batch writes it under option "prover_wire_format" = 3 (the prover holds the points in
 * affine form anyway). */
int bpmi_rp_wire_v2_to_v1(const uint8_t *blobs, uint64_t blobs_len, const uint64_t *off, uint64_t n_proofs, uint8_t *out, uint64_t cap,
                          uint64_t *out_off, int64_t *first_bad);

/* The same preparation on the GPU (csrc/rp_batch_kernels.hpp; one lane per proof parses, re-hashes the transcripts and computes
 * the weighted scalars).  `blobs` / `blob_off` / `weights` / `seed` / `shared` are HOST pointers with the meaning above (blobs may be
 * page-locked memory from bpmi_host_alloc: the upload then runs at link speed); the outputs that feed the MSM stay on the device:
 *   d_v_scalars   n_proofs x values_per_proof x 32 B      d_pt_scalars  n_proofs x (6 + 2k) x 32 B
 *   d_points      n_proofs x (6 + 2k) x 64 B: the proofs' points, decoded where they lie in the blobs (wire order)
 * *first_bad = smallest index of a proof that failed parsing, a transcript check, or has an invalid point encoding; -1 if none.
 * When *first_bad >= 0 the device arrays and `shared` hold no usable result (the batch is rejected).  Otherwise: the same numbers
 * as bpmi_rp_batch_prepare for the same weights / seed, byte for byte (tests/test_gpu_batch_dev.py).  A wire proof longer
 * than 32 KiB is invalid (in both functions).  n_proofs <= 2^22, blobs_len <= 4 GiB per call.  One call at a time per ctx. */
int bpmi_rp_batch_prepare_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                              const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, void *d_v_scalars, void *d_pt_scalars, void *d_points,
                              uint8_t *shared, int64_t *first_bad);
/* The whole batch verification in ONE call (replaces a loop of RangeVerifier.verify, /root/reference/src/rangeproofs/
 * rangeproof_verifier.py:55-99 with src/innerproduct/inner_product_verifier.py:44-58, :127-147, over proofs that share their
 * generators): the preparation above (wire bytes uploaded in slices, the points of a slice decoded while the next slice is on the
 * link), the shared coefficients folded into the scalars of g, h, u, gs, hs on the device, and the batch's one MSM over
 * [g h u gs hs | commitments | proof points] -- no host round trip in between.
 *   v_points  HOST   n_proofs x values_per_proof x 64 B: the commitments, in proof order
 *   d_gens    DEVICE (3 + 2 n_gens) x 64 B: g, h, u, gs[0..n), hs[0..n)  (uploaded once per verifier)
 *   d_points / d_scalars  DEVICE scratch for n_proofs (values_per_proof + 6 + 2k) points of 64 B / scalars of 32 B
 * out = the 64-byte value of the random linear combination: the identity (64 zero bytes) exactly when every equation of every
 * proof holds (up to the 1/q soundness error of the random weights); ranks that verified disjoint shards fold their values.
 * *first_bad as for bpmi_rp_batch_prepare_dev; when it is >= 0 `out` means nothing.  At most 2^23 points in the MSM. */
int bpmi_rp_batch_verify_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                             const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens, void *d_points,
                             void *d_scalars, uint8_t out[64], int64_t *first_bad);
/* Which proofs of a rejected batch are invalid (replaces what a loop of RangeVerifier.verify gives by construction, a verdict per proof:
 * /root/reference/src/rangeproofs/rangeproof_verifier.py:55-99, /root/reference/src/rangeproofs/rangeproof_aggreg_verifier.py:55-108).
 * The call of bpmi_rp_batch_verify_dev with the batch cut into GROUPS of `group` consecutive proofs (group >= 1; the last group may be
 * short): one preparation, then every group's own combination over [g h u gs hs | the group's commitments | the group's proof points],
 * all groups in one launch.  Arguments as for bpmi_rp_batch_verify_dev (weights: 4 per proof by batch index, or derived from the seed by
 * batch index).
 *   values  HOST  ceil(n_proofs / group) x 64 B: values[t] = the value of group t's combination over its UNFLAGGED proofs; 64 zero
 *                 bytes exactly when every one of them verifies (up to the 1/q soundness error)
 *   status  HOST  n_proofs B: bit 0 = the proof failed a byte-level check (parsing, a transcript, a scalar's range), bit 1 = one of
 *                 its point encodings is invalid (wire format 3: a wrong y).  A flagged proof contributes to no group.
 * A well-formed proof of another wire format at the smallest flagged index is BPMI_E_ARG ("mixed wire formats"), as in the calls above;
 * under option "rp_only_role" >= 0 every status is non-zero.  Same limits as bpmi_rp_batch_verify_dev, and ceil(n_proofs / group) x
 * (3 + 2 n_gens) <= 2^26.  One call at a time per ctx. */
int bpmi_rp_batch_group_values_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                                   const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens,
                                   void *d_points, void *d_scalars, uint64_t group, uint8_t *values, uint8_t *status);
/* Range proofs of DIFFERENT sizes in one call and ONE MSM (replaces a loop of RangeVerifier.verify / AggregRangeVerifier.verify over
 * proofs of different sizes: src/rangeproofs/rangeproof_verifier.py:55-99, src/rangeproofs/rangeproof_aggreg_verifier.py:55-108).  A CLASS is a run of proofs with the same (n_gens, values_per_proof) and one wire format; class c
 * uses gs[0..n_c) and hs[0..n_c) of the one list g, h, u, gs[0..N), hs[0..N), N = n_gens_max >= every class's n_gens (what
 * AggregNIRangeProver proofs of m values over the first 64 m generators are).  Every equation of every proof is linear in the generators,
 * so the classes' shared coefficients are summed prefix by prefix and the whole call is one combination.  Proofs are numbered CLASS-MAJOR
 * over the whole call (class 0's first): that global index selects a proof's weights and is what *first_bad reports.
 *   classes   n_classes (1 .. 64) of bpmi_rp_class: blobs / blobs_len / blob_off as for bpmi_rp_batch_verify_dev (classes may differ in wire
 *             format from each other), v_points HOST n_proofs x values_per_proof x 64 B
 *   weights   4 per proof by GLOBAL index, or NULL with a seed: proof i takes SHA-256(seed || LE64(i) || t), i the GLOBAL index
 *   d_gens    DEVICE (3 + 2 n_gens_max) x 64 B: g, h, u, gs[0..N), hs[0..N)
 *   d_points / d_scalars  DEVICE scratch for sum_c n_proofs_c (m_c + 6 + 2 k_c) pairs: the classes' blocks back to back, each laid out as
 *             the single-class call lays out its one block ([commitments | proof points])
 * out = the 64-byte value of the ONE combination over [shared generators | every class's commitments and proof points]: the identity
 * exactly when every equation of every proof holds.  *first_bad = the smallest global index of a proof that fails a byte-level check or has
 * an invalid point, or -1; when it is >= 0 `out` means nothing.  A well-formed proof of another wire format at a class's first flagged
 * index is BPMI_E_ARG ("mixed wire formats", naming the class).  Argument errors (BPMI_E_ARG, decided before anything is read, allocated
 * or uploaded): a null argument, n_classes outside [1, 64], a class the single-class call refuses or with n_gens > n_gens_max (the message
 * names the class), more than 2^23 points in the MSM.  A commitment that is not a point of the curve is refused with its index among the
 * call's commitments, class-major.  One call at a time per ctx. */
typedef struct bpmi_rp_class {
  uint32_t n_gens, values_per_proof; uint64_t n_proofs;
  const uint8_t *blobs; uint64_t blobs_len; const uint64_t *blob_off;
  const uint8_t *v_points;
} bpmi_rp_class;
int bpmi_rp_batch_verify_mixed_dev(bpmi_ctx *ctx, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, const uint8_t *weights,
                                   const uint8_t *seed, const void *d_gens, void *d_points, void *d_scalars, uint8_t out[64], int64_t *first_bad);
/* Which GROUPS of a mixed batch hold an invalid proof, in one call: bpmi_rp_batch_verify_mixed_dev cut the way
 * bpmi_rp_batch_group_values_dev cuts a batch of one size.  The arguments up to d_scalars are those of bpmi_rp_batch_verify_mixed_dev
 * (classes, class-major global numbering, weights by global index or derived from the seed by global index, d_gens = g h u gs[0..N)
 * hs[0..N), the scratch sizes).
 *   group      n_classes entries, each >= 1: class c is cut into groups of min(group[c], n_proofs_c) consecutive proofs, the last one
 *              possibly short; a group never straddles a class
 *   value_off  HOST n_classes + 1 entries: groups are numbered class-major, class c owns values[value_off[c] .. value_off[c + 1]),
 *              value_off[n_classes] = the number of groups
 *   values     HOST 64 B per group: values[t] = the value of group t's combination over its UNFLAGGED proofs over
 *              [g h u gs[:n_c] hs[:n_c] | the group's commitments | the group's proof points]; 64 zero bytes exactly when all of them
 *              verify.  The same 64 bytes bpmi_rp_batch_group_values_dev writes for that class over gs[:n_c], hs[:n_c] under the same
 *              per-proof weights; with no proof flagged the sum of all values is the `out` of bpmi_rp_batch_verify_mixed_dev
 *   status     HOST one byte per proof by GLOBAL index: bit 0 = a byte-level check failed, bit 1 = an invalid point encoding (wire
 *              format 3: a wrong y), as in bpmi_rp_batch_group_values_dev.  A flagged proof takes part in no group.
 * BPMI_E_ARG, decided before anything is read beyond the offset tables, allocated or uploaded, with nothing written: everything
 * bpmi_rp_batch_verify_mixed_dev refuses, with its messages; group, values, value_off or status NULL; a group[c] = 0 (the message names
 * the class); sum_c n_groups_c x (3 + 2 n_c) > 2^26.  A call refused for a point (a commitment, a generator at validation level 2) leaves
 * 0xFF in every byte of `values`.  A well-formed proof of another wire format at a class's smallest flagged index is BPMI_E_ARG ("mixed
 * wire formats", naming the class); under option "rp_only_role" >= 0 every status is non-zero.  A group of more than 8 448 pairs
 * (3 + 2 n_c + group (m_c + 6 + 2 k_c)) runs as an MSM of its own: the same 64 bytes.  One call at a time per ctx. */
int bpmi_rp_batch_group_values_mixed_dev(bpmi_ctx *ctx, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, const uint64_t *group,
                                         const uint8_t *weights, const uint8_t *seed, const void *d_gens, void *d_points, void *d_scalars, uint8_t *values,
                                         uint64_t *value_off, uint8_t *status);
/* ---- a BATCH of single-value range proofs, proved on the device in one call (csrc/rp_prove_kernels.hpp, rp_prove_host.hpp) -------------
 * Replaces a LOOP of NIRangeProver(v, n, g, h, gs, hs, gamma, u, group, seed).prove() (/root/reference/src/rangeproofs/
 * rangeproof_prover.py:35-91) with NIProver.prove / FastNIProver2.prove inside (/root/reference/src/innerproduct/
 * inner_product_prover.py:27-44, :84-110) over proofs that share their generators: the same transcripts
 * (/root/reference/src/utils/transcript.py:13-33), the same seeded blinding scalars (/root/reference/src/utils/utils.py:84-97), the
 * same proofs byte for byte -- but every protocol step is ONE launch over all proofs, every scalar multiplication a lookup in tables
 * of the fixed generators, and the Fiat-Shamir hashes run on the device.
 *   bpmi_rp_prover_create   nbits: a power of two in [2, 128]; g, h, u: 64-byte points; gs, hs: nbits points each.  Builds the tables
 *                           (windows of "prover_table_bits" bits, default 16: 4.4 GB of device memory and ~72 ms for 64-bit proofs;
 *                           12 bits: 378 MB, 17 ms, 22 % slower proving) and keeps them for the prover's lifetime.  A table that does
 *                           not fit the device is BPMI_E_NOMEM.
 *                           The points are checked to be on the curve (option "validate_points" >= 1, the default): BPMI_E_ARG names the first bad one.
 *   bpmi_rp_prove_batch     values, gammas: n_proofs x 32 B little-endian, in [0, q) -- checked: BPMI_E_ARG names the first index that is not -- (of a value only the low nbits bits enter the
 *                           proof, as in rangeproof_prover.py:40); seeds: proof i's transcript seed = seeds[seed_off[i] .. seed_off[i+1])
 *                           (at most 65 535 bytes).  out[out_off[i] .. out_off[i+1]) = proof i in wire format 2 (3 under option "prover_wire_format")
 *                           (python-bulletproofs_amd/rangeproofs/codec.py; bpmi_rp_wire_v2_to_v1 expands it, bpmi_rp_batch_verify_dev
 *                           takes it as it is); out_off has n_proofs + 1 entries; cap >= n_proofs x bpmi_rp_prove_batch_proof_bytes
 *                           (of the longest seed).  At most 2^20 proofs and 2^27 elements (n_proofs x nbits x m) per call -- beyond
 *                           either BPMI_E_ARG names the bound, before anything is read or allocated; one call at a time per prover and ctx.
 *   bpmi_rp_prover_last_ms  device milliseconds of the last batch: A and S | y, z, T1, T2 | x, the vectors, P_new | the rounds of the
 *                           inner-product argument | the wire bytes | their copy to the host | the whole batch */
/* The same for AGGREGATED proofs (round 6): a proof covers m values of nbits bits each (AggregNIRangeProver,
 * /root/reference/src/rangeproofs/rangeproof_aggreg_prover.py:36-146); nbits (at most 128) and m powers of two with 2 <= nbits x m <= 1024 --
 * 4, 8 or 16 amounts of 64 bits are 256, 512 or 1 024 elements --, gs and hs nbits x m
 * points each; bpmi_rp_prove_batch then takes n_proofs x m values and blinding factors (proof p: entries p m .. p m + m - 1).  m = 1 is
 * bpmi_rp_prover_create.  The kernels with a lane per element run in blocks of 256 threads up to 256 elements, of 512 and 1 024 above.
 * Longer vectors (the 128 x 64-bit proof of config C4) are the single-proof prover's: one proof fills the chip there. */
int bpmi_rp_prover_create_aggregated(bpmi_ctx *ctx, uint32_t nbits, uint32_t m, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs,
                                     const uint8_t *hs, bpmi_rp_prover **out);
int bpmi_rp_prover_create(bpmi_ctx *ctx, uint32_t nbits, const uint8_t g[64], const uint8_t h[64], const uint8_t u[64], const uint8_t *gs, const uint8_t *hs,
                          bpmi_rp_prover **out);
void bpmi_rp_prover_destroy(bpmi_rp_prover *pv);
uint64_t bpmi_rp_prove_batch_proof_bytes(const bpmi_rp_prover *pv, uint64_t seed_len);
int bpmi_rp_prove_batch(bpmi_rp_prover *pv, uint64_t n_proofs, const uint8_t *values, const uint8_t *gammas, const uint8_t *seeds, const uint64_t *seed_off,
                        uint8_t *out, uint64_t cap, uint64_t *out_off);
int bpmi_rp_prover_last_ms(const bpmi_rp_prover *pv, double ms[7]);
/* out[i] = values[i] g + gammas[i] h: `commitment(g, h, x, r)` (/root/reference/src/utils/commitments.py:5-6) for count pairs
 * in one launch, from the prover's fixed-base tables of g and h (the path T1 and T2 take) -- the commitments V every verifier of the
 * prover's proofs needs, in the order bpmi_rp_batch_verify_dev takes them (an aggregated prover: count = n_proofs x m).
 * values, gammas: count x 32 B little-endian in [0, q), checked like bpmi_rp_prove_batch's: BPMI_E_ARG names the first index that is not.
 * The WHOLE value enters the commitment, not only its low nbits bits -- what makes the proof of an out-of-range value fail.
 * out: count x 64 B affine (x, y little-endian; the identity is 64 zero bytes).  count <= 2^24; count = 0 is BPMI_OK.  Shares the
 * prover's buffers: one call at a time per prover, like proving. */
int bpmi_rp_prover_commit_batch(bpmi_rp_prover *pv, uint64_t count, const uint8_t *values, const uint8_t *gammas, uint8_t *out);
/* Proofs of DIFFERENT sizes from one prover, one table and one call (csrc/rp_prove_mixed_plan_host.hpp, rp_prove_mixed_kernels.hpp,
 * rp_prove_mixed_host.hpp).  A prover created for (nbits, M) over gs, hs of N = nbits M points is a CAPACITY: a class of m values per
 * proof -- m a power of two, 1 <= m <= M, nbits m >= 2 -- runs over gs[:nbits m], hs[:nbits m], the generators a loop of
 * AggregNIRangeProver(vs, nbits, g, h, gs[:nbits m], hs[:nbits m], gammas, u, group, seed).prove()
 * (/root/reference/src/rangeproofs/rangeproof_aggreg_prover.py:36-146; m = 1: NIRangeProver, rangeproof_prover.py:35-91) would be given:
 * every proof is byte for byte what a prover created over that prefix writes.  The blocks bpmi_rp_batch_verify_mixed_dev verifies.
 *   bpmi_rp_prove_class     one class: n_proofs x m values and gammas, seeds and seed_off (n_proofs + 1 entries) as bpmi_rp_prove_batch takes them
 *   bpmi_rp_prove_batch_proof_bytes_class   bytes of a proof of a class of m values with a seed of seed_len bytes (0: m is no class of the prover)
 *   bpmi_rp_prove_batch_mixed   proves classes[0 .. n_classes) in the caller's order; the proofs are numbered class-major, proof j of the call
 *                           = out[out_off[j] .. out_off[j+1]), out_off has (sum of n_proofs) + 1 entries.  Every step of the protocol is one launch
 *                           per kernel over ALL classes (a class of k rounds leaves the rounds beyond its own out).  Two classes may
 *                           have the same m.  At most 64 classes, 2^20 proofs and 2^27 elements (sum of n_proofs x nbits x m) per call;
 *                           a class of 0 proofs, an m that is no class, a seed above 65 535 bytes, a scalar not below q (the message
 *                           names the class, the array and the first index), a cap below the sum of the proofs' bytes: BPMI_E_ARG, the
 *                           caps before anything is read or allocated, and neither out nor out_off is written.  n_classes = 0 is BPMI_OK
 *                           with out_off[0] = 0.  Options "prover_wire_format" and "prover_job_lanes" cover the whole call (a class's
 *                           lanes per job by the jobs of the whole launch); "prover_split" does not apply.  bpmi_rp_prover_last_ms
 *                           reports the same seven phases.  One window width serves every class: the capacity's. */
typedef struct {
  uint32_t m;                  /* values per proof */
  uint64_t n_proofs;
  const uint8_t *values, *gammas, *seeds;
  const uint64_t *seed_off;
} bpmi_rp_prove_class;
uint64_t bpmi_rp_prove_batch_proof_bytes_class(const bpmi_rp_prover *pv, uint32_t m, uint64_t seed_len);
int bpmi_rp_prove_batch_mixed(bpmi_rp_prover *pv, uint32_t n_classes, const bpmi_rp_prove_class *classes, uint8_t *out, uint64_t cap, uint64_t *out_off);

/* ---- batched inner-product prover ------------------------------------------ */
/* Many inner-product arguments over ONE generator set (g, h of n points each, one u), proved in one device call: a loop of
 * `NIProver(g, h, u, P_p, c_p, a_p, b_p, group, seed_p).prove()` (src/innerproduct/inner_product_prover.py:11-45) or of
 * `FastNIProver2(g, h, u, P_p, a_p, b_p, group, transcript_p).prove()` (:48-110), with the transcript of
 * src/utils/transcript.py:13-33 and mod_hash of src/utils/utils.py:84-97 -- the same proofs byte for
 * byte, every protocol step ONE launch over all proofs, every scalar multiplication a lookup in tables of the fixed generators, the
 * Fiat-Shamir hashes on the device (the machinery of bpmi_rp_prove_batch's Protocol-2 phase).  What bpmi_ipa_verify_batch_dev consumes.
 *   bpmi_ipa_batch_prover_create  (:20-27, :42-54) n: a power of two in [1, 1024] (longer vectors are the single-proof prover's, bpmi_ipa_create:
 *                           one proof fills the chip there); g, h: n 64-byte points each; u: one.  Builds the tables of the 2n + 1
 *                           bases (windows of "prover_table_bits" bits; default as for bpmi_rp_prover_create: 16 bits up to 128
 *                           elements, 302 MB at n = 4, 4.4 GB at n = 64) and keeps them for the prover's lifetime; a table that does
 *                           not fit the device is BPMI_E_NOMEM.  The points are checked to be on the curve (option "validate_points"
 *                           >= 1): BPMI_E_ARG names the first bad one.  The identity, equal and opposite generators are legal.
 *                           h_scale: NULL, or n scalars c_i in [0, q): the argument runs over the generators c_i h_i without
 *                           computing them (the extension of bpmi_ipa_create_scaled and bpmi_ipa_verify_batch_dev).
 *   bpmi_ipa_prove_batch    protocol 1 (:29-36): seeds[seed_off[p] .. seed_off[p+1]) is proof p's transcript seed; x_p =
 *                           mod_hash(base64(seed_p) "&"); head[p] = u_new || P_new = x_p u || P_p + (x_p c_p) u (2 x 64 B affine);
 *                           c: n_proofs x 32 B, or NULL for c_p = <a_p, b_p>; P: n_proofs x 64 B (checked under "validate_points"
 *                           >= 1: BPMI_E_ARG names the index; the identity is legal).
 *                           protocol 2 (:56-68, :94-110): seeds[..] is the `transcript` argument, appended after the "&" of the empty
 *                           seed (it may be empty); c, P and head must be NULL -- the reference's prover never reads P there.
 *                           a, b: n_proofs x n x 32 B little-endian in [0, q) -- checked, like c: BPMI_E_ARG names the first index
 *                           that is not.  A seed has at most 65 535 bytes; seeds may be NULL when every seed is empty.
 *                           Outputs: ab[p] = a || b (2 x 32 B); xs[p] = k x 32 B, k = log2 n; LR[p] = L_0 .. L_(k-1) R_0 .. R_(k-1),
 *                           64 B affine each (the identity is 64 zero bytes); transcripts[tr_off[p] .. tr_off[p+1]) = the final
 *                           digest text of the Protocol-2 argument (under protocol 1 it starts with "&" and the outer transcript
 *                           base64(seed) "&" str(x) "&"); tr_off has n_proofs + 1 entries; cap >= n_proofs x
 *                           bpmi_ipa_prove_batch_transcript_bytes (of the longest seed).  n = 1 has no rounds: xs and LR may be NULL.
 *                           At most 2^20 proofs and 2^27 elements (n_proofs x n) per call.  A wrong protocol, NULL where an array is
 *                           required or non-NULL where it must be NULL, a count beyond the caps, a seed that is too long, decreasing
 *                           offsets and a cap that is too small are BPMI_E_ARG before anything is read or allocated; no output is
 *                           written on any error.  n_proofs = 0 is BPMI_OK and touches nothing.  One call at a time per prover and ctx.
 *   bpmi_ipa_batch_prover_last_ms  device milliseconds of the last batch: the transcripts' start and the head | the rounds | the copy to
 *                           the host | the whole batch */
int bpmi_ipa_batch_prover_create(bpmi_ctx *ctx, uint32_t n, const uint8_t *g, const uint8_t *h, const uint8_t u[64], const uint8_t *h_scale,
                                 bpmi_ipa_batch_prover **out);
void bpmi_ipa_batch_prover_destroy(bpmi_ipa_batch_prover *pv);
uint64_t bpmi_ipa_prove_batch_transcript_bytes(const bpmi_ipa_batch_prover *pv, int protocol, uint64_t seed_len);
int bpmi_ipa_prove_batch(bpmi_ipa_batch_prover *pv, int protocol, uint64_t n_proofs, const uint8_t *a, const uint8_t *b, const uint8_t *c, const uint8_t *P,
                         const uint8_t *seeds, const uint64_t *seed_off, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint8_t *head, uint8_t *transcripts,
                         uint64_t cap, uint64_t *tr_off);
int bpmi_ipa_batch_prover_last_ms(const bpmi_ipa_batch_prover *pv, double ms[4]);
/* The STATEMENTS of a batch from the prover's tables: out[p] = sum_j a_p[j] g_j + sum_j b_p[j] (c_j h_j) + t_p u -- a loop of
 * `vector_commitment(g, h, a_p, b_p)` (src/utils/commitments.py:13, :9-13) plus `inner_product(a, b) * u`: the P that NIProver takes
 * as an input and every verifier takes (src/tests/test_innerprod.py:26, :112).  One launch lays out the scalars, one walks the tables
 * (16 additions per term at 16-bit windows, no buckets), one makes the points affine.
 *   c_j          the prover's h_scale, or 1 without one: multiplied into the scalars, no point is scaled.
 *   a, b         count x n x 32 B little-endian in [0, q).  Either may be NULL (all zeros: its half of every job's terms is dropped,
 *                not multiplied by zero), not both.
 *   u_mode       0: no u term, t must be NULL (NIProver's statement).  1: t_p = <a_p, b_p>, summed on the device over the UNSCALED b;
 *                t must be NULL, a and b are both required (FastNIProver2's statement).  2: t holds count x 32 B scalars in [0, q).
 *   out          HOST memory, count x 64 B affine (x, y little-endian), canonical; the identity is 64 zero bytes; complete on return.
 * BPMI_E_ARG with a message naming the cause, before anything is read or allocated: pv or out NULL, u_mode outside 0 .. 2, t given
 * where it must be NULL or missing under u_mode 2, a and b both NULL (or one of them under u_mode 1), count beyond the caps of
 * bpmi_ipa_prove_batch (2^20 proofs, 2^27 elements).  A scalar that is not below q is BPMI_E_ARG naming the array and the first such
 * index.  No output is written on any error.  count = 0 is BPMI_OK and touches nothing.  Shares the prover's buffers: one call at a
 * time per prover and ctx, like proving.
 *   bpmi_ipa_batch_prover_commit_last_ms  of the last such call: the device milliseconds of its three kernels | the milliseconds of
 *                the whole call on the host's clock (checks, staging, both copies).  bpmi_ipa_batch_prover_last_ms is not touched. */
int bpmi_ipa_batch_prover_commit_batch(bpmi_ipa_batch_prover *pv, uint64_t count, const uint8_t *a, const uint8_t *b, int u_mode, const uint8_t *t,
                                       uint8_t *out);
int bpmi_ipa_batch_prover_commit_last_ms(const bpmi_ipa_batch_prover *pv, double ms[2]);
/* Arguments of DIFFERENT lengths from one prover, one table and one call (csrc/ipa_prove_mixed_plan_host.hpp,
 * ipa_prove_mixed_kernels.hpp, ipa_prove_mixed_host.hpp).  A bpmi_ipa_batch_prover created for n = N is a CAPACITY: a class of
 * n_c = 2^k_c elements, 1 <= n_c <= N, runs over g[:n_c], h[:n_c], the one u, and h_scale[:n_c] where the prover has one -- the
 * generators a loop of `NIProver(g[:n_c], h[:n_c], u, P_p, c_p, a_p, b_p, group, seed_p).prove()`
 * (src/innerproduct/inner_product_prover.py:11-45) or of `FastNIProver2(g[:n_c], h[:n_c], u, P_p, a_p, b_p, group, transcript_p).prove()`
 * (:48-110) would be given: proof p of class c is byte for byte what bpmi_ipa_prove_batch writes on a prover created over that prefix.
 * The rounds never fold a generator (:94-110 read g and h through the fold coefficients), so the table of the longest list serves
 * every class; every protocol step is one launch per kernel over ALL classes, k_max + 1 steps where a loop over lengths runs the sum
 * of the k_c + 1.
 *   bpmi_ipa_prove_class    one class: n, n_proofs and the inputs a, b, c, P, seeds, seed_off as bpmi_ipa_prove_batch takes them
 *                           (n_proofs x n x 32 B etc.; c may be NULL per class), and the class's OWN outputs ab, xs, LR, head,
 *                           transcripts (cap bytes), tr_off (n_proofs + 1 entries): with the class's statements they are the fields of
 *                           one bpmi_ipa_packed_class of bpmi_ipa_verify_batch_packed_mixed_dev, untouched.
 *   bpmi_ipa_prove_batch_transcript_bytes_class   bpmi_ipa_prove_batch_transcript_bytes of a class of n elements (0: n is no class of
 *                           the prover, or the protocol is neither 1 nor 2)
 *   bpmi_ipa_prove_batch_mixed   proves classes[0 .. n_classes) in the caller's order, one protocol per call.  The NULL / non-NULL rules of
 *                           bpmi_ipa_prove_batch hold per class with the class's own k_c (a class of n = 1 may pass NULL xs and LR).
 *                           Two classes may have the same n.  BPMI_E_ARG, the message naming the class where there is one: more
 *                           than 64 classes, an n that is no class, a class of 0 proofs, more than 2^20 proofs or 2^27 elements (sum
 *                           of n_proofs x n) per call, a seed above 65 535 bytes, decreasing seed offsets, a class's cap below n_proofs
 *                           x bpmi_ipa_prove_batch_transcript_bytes_class of its longest seed, a scalar of a, b, c not below q (the
 *                           message names the class, the array and the first index), and under protocol 1 and "validate_points" >= 1
 *                           a P that is no point of the curve (the class and the index).  The shape errors come before anything is
 *                           read or allocated; no output of any class is written on any error.  n_classes = 0 is BPMI_OK (the
 *                           protocol is still checked) and touches nothing.  Option "prover_job_lanes" covers the whole call (a
 *                           class's lanes per job by the jobs of the whole launch).  bpmi_ipa_batch_prover_last_ms reports the same
 *                           four phases.  One window width serves every class: the capacity's.
 *   bpmi_ipa_commit_class, bpmi_ipa_batch_prover_commit_batch_mixed   the statements of such a block from the same tables:
 *                           out_c[p] = sum_j a_p[j] g_j + sum_j b_p[j] (c_j h_j) + t_p u over the class's prefix -- per class a loop of
 *                           `vector_commitment(g[:n_c], h[:n_c], a_p, b_p)` (src/utils/commitments.py:13) plus `inner_product(a, b) * u`.
 *                           u_mode is one value per call; the NULL rules of bpmi_ipa_batch_prover_commit_batch hold per class; the
 *                           caps and the class errors are those of the prove call; nothing is written on an error.
 *                           bpmi_ipa_batch_prover_commit_last_ms reports this call like the single-class one. */
typedef struct {
  uint32_t n;                    /* elements per vector: a power of two, 1 <= n <= the prover's */
  uint64_t n_proofs;
  const uint8_t *a, *b, *c, *P;
  const uint8_t *seeds;
  const uint64_t *seed_off;
  uint8_t *ab, *xs, *LR, *head, *transcripts;
  uint64_t cap;
  uint64_t *tr_off;
} bpmi_ipa_prove_class;
uint64_t bpmi_ipa_prove_batch_transcript_bytes_class(const bpmi_ipa_batch_prover *pv, uint32_t n, int protocol, uint64_t seed_len);
int bpmi_ipa_prove_batch_mixed(bpmi_ipa_batch_prover *pv, int protocol, uint32_t n_classes, const bpmi_ipa_prove_class *classes);
typedef struct {
  uint32_t n;
  uint64_t count;
  const uint8_t *a, *b, *t;
  uint8_t *out;
} bpmi_ipa_commit_class;
int bpmi_ipa_batch_prover_commit_batch_mixed(bpmi_ipa_batch_prover *pv, int u_mode, uint32_t n_classes, const bpmi_ipa_commit_class *classes);

/* ---- batch verifier of PACKED inner-product proofs ---------------------------------------- */
/* What bpmi_ipa_prove_batch writes, verified without leaving native code: the Fiat-Shamir re-hash, the byte-level checks and the
 * weighted scalars of every proof run per proof (host twin: csrc/ipa_packed_host.hpp; kernels: csrc/ipa_packed_kernels.hpp), then
 * the batch is the one MSM of bpmi_ipa_verify_batch_dev.  The arrays are the library's own layout (the wire format of a Protocol-2
 * proof is BPIP2, below): for n = 2^k the input is, per call,
 *   ab           n_proofs x 64 B        a || b, little-endian
 *   xs           n_proofs x k x 32 B    the challenges, little-endian                           (NULL allowed at k = 0)
 *   LR           n_proofs x 2k x 64 B   L_0 .. L_(k-1) R_0 .. R_(k-1), affine; the identity is 64 zero bytes   (NULL allowed at k = 0)
 *   transcripts, tr_off (n_proofs + 1)  proof p's inner (Protocol-2) transcript text is transcripts[tr_off[p] .. tr_off[p+1])
 *   start        n_proofs x uint32, or NULL: Proof2.start_transcript; NULL = 1 for every proof (the empty prefix).  Protocol 2 only
 *   u            protocol 2: n_proofs x 64 B; protocol 1: 64 B (the statements' one u)
 *   P            n_proofs x 64 B
 *   c, head      protocol 1: n_proofs x 32 B claimed inner products, n_proofs x 128 B u_new || P_new; NULL under protocol 2
 * Under protocol 1 the transcript is the inner one as the prover writes it, "&" base64(seed) "&" str(x) "&" rounds..: the rounds
 * begin at item 3 and Verifier1's challenge is item 2.
 * A packed proof is VALID exactly when the Proof2 / Proof1 object with the same bytes passes Verifier2.verify
 * (/root/reference/src/innerproduct/inner_product_verifier.py:104-147) / Verifier1.verify (:44-58; its transcript = items 1-2 of
 * the inner one plus "&", start_transcript = 3), with four conventions of this ABI on top: a, b, c and xs[j] are below q; a point
 * is the identity or on the curve; a decimal item is canonical (what str(int) prints); a transcript of more than 2^17 bytes is
 * invalid (the longest the prover writes, from a 65 535-byte seed at k = 22, is shorter).
 * Outputs of the preparation, per proof p:
 *   record        16k + 24 words: k pairs (x_j, x_j^-1), then a, b, w_p -- what the s-vector sum of bpmi_ipa_verify_batch_dev reads;
 *                 ONE inversion per proof
 *   extra pairs   protocol 2, 2k + 2:  points [u_p, L_0.., R_0.., P_p]               scalars [w a b, -w x_j^2, -w x_j^-2, -w]
 *                 protocol 1, 2k + 4:  points [u_new, L.., R.., P_new, P_p, u]       scalars [w a b + r2, -w x_j^2, -w x_j^-2, r1 - w, -r1,
 *                 -(r1 c + r2) x]: Verifier2's equation over (u_new, P_new) under w, P_new = P + x c u (:51) under r1, u_new = x u
 *                 (:52) under r2
 *   status        bit 0: a byte-level check failed -- a value >= q; a short or malformed transcript; an L / R item that is not
 *                 base64(SEC1(point)) ("AA==" for the identity) (:114-115); an x item that is not the canonical decimal of xs[j] or not
 *                 the re-hash of its prefix (:116-125); protocol 1: item 2 is not mod_hash(item 1 "&") (:36-42)
 *                 bit 1: a point of the proof (LR, P, head, a per-proof u) is neither the identity nor on the curve; checked under
 *                 "validate_points" >= 1 (always by the host twin); at 0 the result is unspecified but never out of bounds
 *                 A flagged proof contributes NOTHING: zero record, zero scalars, identity points.
 * Weights: explicit, little-endian, reduced mod q -- one per proof (w) under protocol 2, three (w, r1, r2) under protocol 1 -- or
 * NULL with a 32-byte seed: then weight t of proof p is SHA-256(seed || LE64(p) || t) cut to 248 bits, 0 replaced by 1, as in
 * bpmi_rp_batch_prepare.  They must be unpredictable to whoever made the proofs.
 * BPMI_E_ARG before anything is read or allocated: a protocol other than 1 or 2; NULL where an array is required or non-NULL where
 * it must be NULL; decreasing tr_off; more than 4 GiB of transcripts; the bounds of bpmi_ipa_verify_batch_dev (k <= 22, 1 .. 2^16
 * proofs, n_proofs x n <= 2^32, the half tables, 2^22 extra pairs); protocol 1: a u that is not on the curve.  n_proofs = 0 is
 * BPMI_OK and touches nothing.
 *   bpmi_ipa_batch_prepare       HOST code on `threads` threads, no ctx (its message: bpmi_last_error(NULL)); records, extra_pts,
 *                                extra_scalars, status in host memory
 *   bpmi_ipa_batch_prepare_dev   the same bytes (tests/test_gpu_ipa_packed.py) by the kernels, into device memory; status to the host
 *   bpmi_ipa_verify_batch_packed_dev   upload, preparation, s-vector sum and the one MSM over [g | h | extra] in one call:
 *                                out = the weighted combination over the unflagged proofs; the batch is valid iff every status is
 *                                0 and out is 64 zero bytes (up to the 1/q soundness error).  d_g, d_h (, d_hscale): as in
 *                                bpmi_ipa_verify_batch_dev; the generators are checked at "validate_points" = 2; a call refused for
 *                                a point leaves 0xFF.. in out.  n_proofs = 0 writes the identity.  One call at a time per ctx. */
int bpmi_ipa_batch_prepare(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts,
                           const uint64_t *tr_off, const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head,
                           const uint8_t *weights, const uint8_t *seed, int threads, uint8_t *records, uint8_t *extra_pts, uint8_t *extra_scalars,
                           uint8_t *status);
int bpmi_ipa_batch_prepare_dev(bpmi_ctx *ctx, uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR,
                               const uint8_t *transcripts, const uint64_t *tr_off, const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c,
                               const uint8_t *head, const uint8_t *weights, const uint8_t *seed, void *d_records, void *d_extra_pts, void *d_extra_scalars,
                               uint8_t *status);
int bpmi_ipa_verify_batch_packed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs,
                                     const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                                     const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head, const uint8_t *weights,
                                     const uint8_t *seed, uint8_t out[64], uint8_t *status);
/* Which GROUPS of a packed batch hold an invalid proof, in one call (the counterpart of bpmi_rp_batch_group_values_dev): the
 * preparation above runs once, the s-vectors are summed per group of `group` consecutive proofs, and the groups' MSMs over
 * [g | h | the group's extra pairs] run as one launch over (group, window) with a device tail -- or, where a group's 2n + group x
 * (2k + 2 | 2k + 4) pairs exceed 8 448, as one MSM per group.  Every argument before `group` as in bpmi_ipa_verify_batch_packed_dev
 * (NULL rules, explicit weights or seed-derived ones by batch index).
 *   group    >= 1; a value above n_proofs is clamped to it
 *   values   HOST memory, ceil(n_proofs / group) x 64 B: values[t] = the combination over the unflagged proofs of
 *            [t group, (t + 1) group) -- the 64 bytes bpmi_ipa_verify_batch_packed_dev writes for that sub-batch under the same weights;
 *            64 zero bytes exactly when all of them verify
 *   status   n_proofs bytes, bits as above; a flagged proof contributes to no group
 * n_proofs = 0 is BPMI_OK and touches nothing.  BPMI_E_ARG before anything is read, allocated or uploaded: what the verify call
 * refuses; group = 0; values or status NULL; ceil(n_proofs / group) x 2n > 2^26 (the rows of group scalars).  The generators are
 * checked at "validate_points" = 2; a call refused for a point leaves 0xFF in every byte of values.  bpmi_debug_ipap_t_budget (below)
 * cuts this call's preparation into rounds of at least 64 proofs as well.  One call at a time per ctx. */
int bpmi_ipa_group_values_packed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs,
                                     const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                                     const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head, const uint8_t *weights,
                                     const uint8_t *seed, uint64_t group, uint8_t *values, uint8_t *status);

/* ---- packed inner-product proofs of DIFFERENT lengths: a list of classes, one MSM ------------------------------------------
 * The packed verifier above for proofs over the PREFIXES of one generator list (the statements of bpmi_ipa_verify_batch_mixed_dev:
 * Verifier2 / Verifier1 over g[:n], h[:n], src/innerproduct/inner_product_verifier.py:104-147 and :44-58, with get_ss, :91-102, over the
 * proof's own k challenges).  A CLASS is what one call of bpmi_ipa_verify_batch_packed_dev takes -- n_proofs packed proofs of one
 * n = 2^k, e.g. the arrays one bpmi_ipa_batch_prover wrote -- and a call takes 1 .. 64 classes, in any order of k, several of one k
 * allowed.  Every class is prepared on the device (the re-hash, the byte-level checks, one inversion per proof, the weighted scalars:
 * one launch per round over the row chunks of ALL classes, csrc/ipa_packed_kernels.hpp), then the batch is the one mixed s-vector sum
 * and the ONE MSM of bpmi_ipa_verify_batch_mixed_dev.  No host loop over proofs.
 *   protocol     1 or 2, one per call.  Protocol 1: a class's u is that class's one point (64 B), checked on the host; protocol 2:
 *                n_proofs x 64 B.  The NULL / non-NULL rules of every class are those of the single-class call.
 *   classes      a class with n_proofs = 0 is legal and skipped: its pointers are not read.  If every class is empty the verify call
 *                writes the identity, the preparation calls touch nothing, and both return BPMI_OK.
 *   numbering    proofs are numbered CLASS-MAJOR over the call, class 0's first.  That global index addresses `status` (one byte per
 *                proof, bits as above), the explicit `weights` (1 x 32 B per proof under protocol 2, 3 x 32 B under protocol 1) and
 *                is the index of a seed-derived weight: SHA-256(seed || LE64(global index) || t) cut to 248 bits, 0 -> 1.
 *   validity     of a packed proof: unchanged, with the proof's own k, over the first 2^k generators.
 * Outputs of the preparation (K: the capacity, n_gens = 2^K; every k <= K):
 *   extra_pts, extra_scalars   the classes' blocks back to back in the CALLER's class order; inside a block proof-major, 2k + 2
 *                (protocol 2) or 2k + 4 (protocol 1) pairs per proof in the pair order above
 *   records      the classes' blocks (16k + 24 words per proof) in the order the mixed s-vector sum reads them: descending k, stable
 *                among equal k -- a class's proofs stay contiguous.  rec_byte_off[c] (n_classes entries): the byte offset of class
 *                c's block (0 for an empty class)
 *   a flagged proof contributes nothing: zero record, zero scalars, identity points.
 * The verify call: out = the one combination over [g[:n_top] | h[:n_top] | every class's extra pairs], n_top = 2^max k; the batch is
 * valid iff every status byte is 0 and out is 64 zero bytes.  Generators are checked as in bpmi_ipa_verify_batch_mixed_dev (the first
 * n_top at "validate_points" = 2); a call refused for a point leaves 0xFF.. in out.
 * BPMI_E_ARG before anything is read beyond tr_off, allocated or uploaded, and no output is written (the message names the class
 * where there is one): n_classes outside 1 .. 64 or a NULL classes; K > 22 or a k above K; a class the single-class call refuses;
 * more than 2^16 proofs, 2^32 elements (the sum of 2^k), 1 GiB of half tables, 2^22 extra pairs or 4 GiB of transcripts in total.
 * One call at a time per ctx.
 *   bpmi_ipa_batch_prepare_mixed       HOST code on `threads` threads over the whole call, no ctx (message: bpmi_last_error(NULL))
 *   bpmi_ipa_batch_prepare_mixed_dev   the same bytes (tests/test_gpu_ipa_packed_mixed.py) by the kernels, into device memory;
 *                                      rec_byte_off and status to the host
 *   bpmi_ipa_verify_batch_packed_mixed_dev   the whole verification */
typedef struct bpmi_ipa_packed_class {
  uint32_t k;                 /* n = 2^k elements, over g[:n], h[:n] (, c[:n]) */
  uint64_t n_proofs;
  const uint8_t *ab, *xs, *LR, *transcripts;      /* exactly the arrays of bpmi_ipa_verify_batch_packed_dev for this class */
  const uint64_t *tr_off;
  const uint32_t *start;
  const uint8_t *u, *P, *c, *head;
} bpmi_ipa_packed_class;
int bpmi_ipa_batch_prepare_mixed(uint32_t K, int protocol, uint32_t n_classes, const bpmi_ipa_packed_class *classes, const uint8_t *weights,
                                 const uint8_t *seed, int threads, uint8_t *records, uint64_t *rec_byte_off, uint8_t *extra_pts,
                                 uint8_t *extra_scalars, uint8_t *status);
int bpmi_ipa_batch_prepare_mixed_dev(bpmi_ctx *ctx, uint32_t K, int protocol, uint32_t n_classes, const bpmi_ipa_packed_class *classes,
                                     const uint8_t *weights, const uint8_t *seed, void *d_records, uint64_t *rec_byte_off, void *d_extra_pts,
                                     void *d_extra_scalars, uint8_t *status);
int bpmi_ipa_verify_batch_packed_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, int protocol,
                                           uint32_t n_classes, const bpmi_ipa_packed_class *classes, const uint8_t *weights, const uint8_t *seed,
                                           uint8_t out[64], uint8_t *status);
/* Which GROUPS of a list of classes hold an invalid proof, in one call: bpmi_ipa_group_values_packed_dev for the mixed packed call.
 * The preparation of bpmi_ipa_verify_batch_packed_mixed_dev and its half tables run once; the s-vectors are summed per group of
 * consecutive proofs of ONE class (one launch over every class's rows), and the groups' MSMs over [g[:n_c] | h[:n_c] | the group's
 * extra pairs] run as at most one launch per block shape over (group, window) with one device tail -- or, for a class whose
 * 2 n_c + group x (2k + 2 | 2k + 4) pairs exceed 8 448, as one MSM per group.  Arguments up to `classes`, `weights`, `seed` and
 * `status` (global class-major index, bits 0 and 1) as in bpmi_ipa_verify_batch_packed_mixed_dev.
 *   group      n_classes entries, each >= 1 (not read for an empty class): class c is cut into groups of min(group[c], n_proofs_c)
 *              consecutive proofs, the last one possibly short.  A group never straddles a class; an empty class has none.
 *   value_off  HOST memory, n_classes + 1 entries: groups are numbered class-major and class c owns the values
 *              [value_off[c], value_off[c + 1]); value_off[n_classes] is the number of groups
 *   values     HOST memory, 64 B per group: values[t] = the combination over the unflagged proofs of group t over
 *              [g[:n_c] | h[:n_c] | that group's extra pairs]; 64 zero bytes exactly when all of them verify.  The sum of all values is
 *              the `out` of the verify call under the same weights
 *   a flagged proof takes part in no group.  The call gives no verdict: the values and the status are the result.
 * Every class empty: BPMI_OK, value_off all zero, values untouched.  BPMI_E_ARG before anything is read beyond tr_off, allocated or
 * uploaded, and nothing is written: what the mixed packed verify call refuses, with its messages; group NULL or a group[c] = 0 on a
 * non-empty class (the message names the class); values, value_off or status NULL; the sum over the classes of n_groups x 2 n_c
 * above 2^26 (the rows of group scalars).  A call refused for a point (a class's u under protocol 1; one of the first n_top generators
 * at "validate_points" = 2) leaves 0xFF in every byte of values.  bpmi_debug_ipap_t_budget applies.  One call at a time per ctx. */
int bpmi_ipa_group_values_packed_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, int protocol,
                                           uint32_t n_classes, const bpmi_ipa_packed_class *classes, const uint64_t *group, const uint8_t *weights,
                                           const uint8_t *seed, uint8_t *values, uint64_t *value_off, uint8_t *status);
/* ---- wire format BPIP2 of Protocol-2 inner-product proofs, verified from bytes ------------------- */
/* The packed arrays above carry every fact two or three times (the points as LR rows and as base64 items of the transcript, the
 * challenges as xs rows and in decimal).  BPIP2 is the same information once, self-describing, 78 + 98 k + prefix_len bytes for a
 * proof of n = 2^k elements (0.67 KB at n = 64 against 2.04 KB packed):
 *   "BPIP2" | k (1 B)                              k <= 22
 *   a | b | xs[0..k)                               (2 + k) x 32 B big-endian
 *   L_0 .. L_(k-1) R_0 .. R_(k-1)                  2k x 33 B SEC1 compressed; 33 zero bytes = the identity
 *   start (4 B big-endian)                         Proof2.start_transcript
 *   prefix_len (4 B big-endian) | prefix           the transcript's bytes before item `start`
 * (scalars, identity and the points' offset as rangeproofs/codec.py).  A batch is `blobs` plus `off`: n_proofs + 1 offsets, proof p
 * is blobs[off[p] .. off[p+1]).  A blob STANDS FOR the packed proof with ab, xs little-endian, LR the decompressed points, start, and
 * the transcript
 *   prefix || for each round j:  item(L_j) "&" item(R_j) "&" decimal(x_j) "&"      item = base64(SEC1(point)), "AA==" for the identity
 * -- what FastNIProver2 writes (/root/reference/src/innerproduct/inner_product_prover.py:94-110 over src/utils/transcript.py:13-29;
 * for its proofs the prefix is "&" plus the `transcript` argument, :62-67).  A wire proof is VALID exactly when that packed proof is
 * valid for bpmi_ipa_verify_batch_packed_dev, with three conventions on top:
 *   status bit 0   a malformed blob: wrong magic; a k byte that is not the call's; a length that is not 78 + 98 k + prefix_len; a, b
 *                  or x_j >= q; an expansion above 2^17 bytes.  Nothing of it is expanded (zero ab / xs rows, start 0, no transcript)
 *   status bit 1   a point that does not decode -- a tag other than 0, 2, 3; tag 0 with a non-zero x; x >= p; an x with no y -- at
 *                  EVERY "validate_points" level (the decompression decides it anyway).  Its LR row is zero.  The points are decoded
 *                  whenever the blob has the call's header and at least 78 + 98 k bytes, so both bits can be set
 *   a flagged proof contributes nothing, as in the packed call; the status byte of a proof these two conventions flag holds their
 *   bits alone (the packed checks saw rows that are zero).
 * `start` is carried, not recounted: a prefix whose number of '&' does not match it expands to a proof the packed checks reject.
 * ENCODABLE is a packed proof whose transcript IS that text: at least `start` '&', and from item `start` on exactly the canonical
 * rounds; a, b, xs below q; every L, R the identity or on the curve.  A proof with trailing text passes Verifier2 (which never looks
 * behind the last round, inner_product_verifier.py:104-125) but has no wire form.
 * Protocol 2 only: Protocol 1, proofs of different lengths in one call, the group / locate calls and a format with y hints are out
 * of scope; every entry point below takes `protocol` where the packed calls do and refuses anything but 2 with BPMI_E_ARG.
 *   bpmi_ipa_wire_bytes        78 + 98 k + prefix_len
 *   bpmi_ipa_wire_encode       HOST code, no ctx (message: bpmi_last_error(NULL)).  packed -> blobs back to back in blobs[0, cap) and off
 *                              (n_proofs + 1; off[0] = 0); status[p] = 0, or 1 for a proof that is not encodable (an empty blob).
 *                              start NULL = 1 for every proof.  cap: n_proofs x (78 + 98 k) + the transcripts' bytes always suffice;
 *                              BPMI_E_ARG when it runs out
 *   bpmi_ipa_wire_expand       HOST code, no ctx: blobs -> ab, xs, LR, transcripts[0, cap) with tr_off (n_proofs + 1), start, status.
 *                              cap must hold the expansion BOUND of the call: per proof min(len - 78 - 98 k + 169 k, 2^17), 0 for a
 *                              blob shorter than 78 + 98 k (BPMI_E_ARG otherwise).  The host twin (csrc/ipa_wire_host.hpp)
 *   bpmi_ipa_wire_expand_dev   the same bytes (tests/test_gpu_ipa_wire.py) by the kernels of csrc/ipa_wire_kernels.hpp, downloaded: the
 *                              comparison hook.  bpmi_debug_ipap_t_budget applies
 *   bpmi_ipa_verify_batch_wire_dev   the blobs uploaded as they are; decompression and expansion in device memory; then the
 *                              preparation, the s-vector sum and the one MSM of bpmi_ipa_verify_batch_packed_dev, unchanged.  u, P:
 *                              n_proofs x 64 B; weights / seed, out, status, d_g, d_h (, d_hscale), the 0xFF rule of a refused
 *                              generator and the caps (2^16 proofs, k <= 22, ...) as there.  n_proofs = 0 writes the identity.
 *                              BPMI_E_ARG before anything is read beyond off, allocated or uploaded, and nothing is written:
 *                              decreasing off, more than 4 GiB of blobs, NULL arguments, a protocol other than 2.
 *                              bpmi_debug_ipap_t_budget applies (at least 64 proofs per launch).  One call at a time per ctx. */
uint64_t bpmi_ipa_wire_bytes(uint32_t k, uint64_t prefix_len);
int bpmi_ipa_wire_encode(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts,
                         const uint64_t *tr_off, const uint32_t *start, uint8_t *blobs, uint64_t cap, uint64_t *off, uint8_t *status);
int bpmi_ipa_wire_expand(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *blobs, const uint64_t *off, uint8_t *ab, uint8_t *xs, uint8_t *LR,
                         uint8_t *transcripts, uint64_t cap, uint64_t *tr_off, uint32_t *start, uint8_t *status);
int bpmi_ipa_wire_expand_dev(bpmi_ctx *ctx, uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *blobs, const uint64_t *off, uint8_t *ab, uint8_t *xs,
                             uint8_t *LR, uint8_t *transcripts, uint64_t cap, uint64_t *tr_off, uint32_t *start, uint8_t *status);
int bpmi_ipa_verify_batch_wire_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs,
                                   const uint8_t *blobs, const uint64_t *off, const uint8_t *u, const uint8_t *P, const uint8_t *weights, const uint8_t *seed,
                                   uint8_t out[64], uint8_t *status);
/* test hook (not part of the drop-in surface): the byte budget of the transposed transcripts of ONE round of the mixed packed calls
 * on this ctx (0: the default, 2^28) -- a small value makes a few hundred proofs run as several rounds.  It also bounds one preparation
 * launch of bpmi_ipa_group_values_packed_dev (at least 64 proofs).  Not an option. */
int bpmi_debug_ipap_t_budget(bpmi_ctx *ctx, uint64_t bytes);

/* Page-locked host memory (hipHostMalloc) for buffers handed to the library repeatedly, e.g. the receive buffer of wire proofs. */
int bpmi_host_alloc(bpmi_ctx *ctx, size_t bytes, void **out);
int bpmi_host_free(bpmi_ctx *ctx, void *p);

/* ---- self-test hook (not part of the drop-in surface) ---------------------------------------------------
 * Runs one member of the device's field-multiplication family on n operand tuples given as RAW 9 x 29-bit
 * limb vectors (9 uint32 each, any lazy magnitude the routine allows) and returns the raw result limbs:
 * op 0 a*b, 1 a^2, 2 a*b + c, 3 a^2 + c, 4 a*b + c*d, 5 carry(a), 6 canonical(a), 7 3 a^2, 8 a*b + 8 c,
 * 9 the limbs of the first 8 uint32 of a read as 32-byte little-endian words (fe_from_words).  tests/test_gpu_field.py
 * compares them with the host build of the same header, limb for limb -- the arithmetic under every
 * `Point + Point` of the reference (src/pippenger/group.py:31-32) is pinned at its worst-case bounds.
 * op 10..15: the mod-q limb arithmetic of the batch-preparation kernel (csrc/scalar.hpp "sq"): 10 a*b, 11 a+b, 12 a-b,
 * 13 -a (raw limbs out); 14 canonical 8 words of a; 15 inverse of a's canonical value (8 words, binary Euclid). */
int bpmi_debug_fe_op(bpmi_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint64_t n,
                     uint32_t *out);
/* self-test hook: out[i] = a[i] + b[i] on 144-byte XYZZ records (4 x 9 limbs of 29 bits: X, Y, ZZ, ZZZ; all zero = identity) with the
 * four-lane point addition of the bucket reduction (csrc/msm_kernels.hpp quad_add) */
int bpmi_debug_quad_add(bpmi_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out);
/* self-test hook: one member of the group law of csrc/curve.hpp on n raw 144-byte records, limb forms as given (36 uint32 each: XYZZ =
 * X, Y, ZZ, ZZZ; Jacobian = X, Y, Z in the first 27; an affine addend = x, y in the first 18 of b).  Results in the same layout, unused
 * words 0: op 0 xyzz_add(a, b), 1 xyzz_dbl(a), 2 xyzz_madd(a, b.x, b.y), 3 xyzz_dbl_affine(b.x, b.y), 4 jac_dbl(a) (Jacobian),
 * 5 jac_madd(a, b.x, b.y) (Jacobian), 6 xyzz_to_affine(a) (x, y), 7 jac_to_affine(a) (x, y), 8 xyzz_add(r, r, b) with r = a,
 * 9 xyzz_dbl(r, r) with r = a.  tests/test_point_forms.py compares them with the host build of the same header. */
int bpmi_debug_point_op(bpmi_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out);

/* ---- per-stage device timing (HIP events on the ctx's stream) --------------------------
 * After bpmi_profile(ctx, 1) every MSM records HIP events around each kernel
 * stage (enable = 2: around the dominant stage, msm_accumulate, only -- every recorded event costs
 * a ~10 us bubble between two kernels, so a timed run should use 2); bpmi_profile_read returns accumulated milliseconds and launch counts
 * per stage since the last reset.  Stage names: bpmi_profile_stage_name(i). */
#define BPMI_NSTAGES 15
int bpmi_profile(bpmi_ctx *ctx, int enable);
int bpmi_profile_reset(bpmi_ctx *ctx);
int bpmi_profile_read(bpmi_ctx *ctx, double ms[BPMI_NSTAGES], uint64_t calls[BPMI_NSTAGES]);
const char *bpmi_profile_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* BPMI_H */
