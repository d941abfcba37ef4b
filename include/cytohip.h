/*
 * cytohip.h -- C ABI of libcytohip.so, the MI355X (gfx950) implementation of CytoSPACE's
 * cell-to-spot linear-assignment hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an int status
 * (0 = CYTO_OK) and never throws.  Buffers are caller-owned and borrowed for the call only.
 * The reference is pure Python; the "FFI" a maintainer binds is ctypes.
 * Citations are into /root/reference/.
 */
#ifndef CYTOHIP_H
#define CYTOHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (errors of the reference it stands for are noted) ---- */
enum {
    CYTO_OK = 0,
    CYTO_ERR_BAD_ARG = 1,       /* non-square / null / negative sizes; reference: ValueError in lapjv */
    CYTO_ERR_NONFINITE = 2,     /* NaN/Inf in the cost matrix (zero-variance column in common.py:197) */
    CYTO_ERR_NOMEM = 3,         /* host or device allocation failed; reference: BrokenProcessPool/OOM */
    CYTO_ERR_INTERNAL = 4,      /* solver invariant violated */
    CYTO_ERR_HIP = 5,           /* a HIP runtime call failed; cyto_last_hip_error() has the text */
    CYTO_ERR_NO_DEVICE = 6,     /* no gfx950 device visible */
    CYTO_ERR_UNSUPPORTED = 7,   /* size outside what this build supports (n > 262144 per LAP); cyto_table_read: a file outside the grammar */
    CYTO_ERR_SHAPE = 8,         /* gene counts differ; reference: ValueError, common/common.py:191-192 */
    CYTO_ERR_PEER = 9           /* another rank of the communicator failed, aborted or did not arrive; reference: BrokenProcessPool */
};

const char *cyto_strerror(int status);
const char *cyto_last_hip_error(void);   /* thread-local text of the last failing HIP call */
const char *cyto_version(void);
/* ABI check for callers that mirror the structs below (ctypes, cgo ...): the library's own sizeof(cyto_lap_info),
 * sizeof(cyto_lap_opts), sizeof(cyto_assign_info), sizeof(cyto_chunk).  The structs carry no size member: a caller built
 * against another header version must compare these at load time (cytospace_amd/_lib.py does) instead of passing a struct
 * the library would overrun.  ABI history: INTEGRATION.md, "ABI versions". */
int cyto_abi_sizes(size_t *lap_info, size_t *lap_opts, size_t *assign_info, size_t *chunk);
/* Solves of this process whose searches ran in the wide solver's embedded form (one problem, several searches at once, prices in
 * global memory: DESIGN 4.1a) -- a process-wide count, so that a test can tell which form ran; it is not part of cyto_lap_info. */
long long cyto_wide_embedded_solves(void);
/* Searches of this process that several-searches-at-once solves ended before their ends, because a lower search of their batch was
 * already flagged (0 with the developer knob CYTO_AUG_ABORT=0).  Process-wide count, for tests and tools; every such
 * search is also counted in cyto_lap_info.wide_par_discarded. */
long long cyto_wide_aborted_searches(void);
/* Float32 solves of this process whose first row caches came from the column reduction's own pass (one problem per
 * call, no row map, from 32 768 rows on), and the rows of those solves that the row builder swept all the same (the rows the lists
 * could not certify; every row of a solve that gave the lists up).  Process-wide counts, for tests and tools. */
long long cyto_fused_cache_solves(void);
long long cyto_fused_cache_fallback_rows(void);

/* ---- device + memory plumbing (so callers can keep the cost matrix resident in HBM) ---- */
int cyto_device_count(int *count);
int cyto_device_name(int device_id, char *buf, size_t buflen);
int cyto_malloc(void **dptr, size_t bytes, int device_id);
int cyto_free(void *dptr, int device_id);
int cyto_memcpy_h2d(void *dst, const void *src, size_t bytes, int device_id);
int cyto_memcpy_d2h(void *dst, const void *src, size_t bytes, int device_id);
int cyto_memcpy_d2d(void *dst, const void *src, size_t bytes, int device_id);
int cyto_device_synchronize(int device_id);
/* Work buffers of the solves are taken from a per-device cache of HBM blocks and go back to it afterwards (a steady
 * stream of chunk solves performs no hipMalloc / hipFree: hipFree would synchronise the whole device and serialise the
 * chunks that run side by side).  This returns every cached block to the runtime. */
int cyto_trim_device_cache(int device_id);
/* Test hook: neither the cache nor the plain large buffers initialise what they hand out, so a word a kernel reads before anyone
 * wrote it reads as zero on a fresh block and as the previous solve's state on a reused one.  cyto_cache_poison(byte) with byte in
 * 0...255 makes every block the cache hands out (fresh or reused, over its whole rounded size) and every plain large buffer arrive
 * filled with that byte, the fill complete before the allocation returns; -1 turns the mode off (the default; off costs one relaxed
 * atomic load per allocation).  Process-wide, needs no device; anything else is CYTO_ERR_BAD_ARG.  cyto_cache_poison_fills() /
 * cyto_cache_poison_bytes() count the fills and the bytes filled in this process.  cyto_cache_peek takes a block of `bytes` from the
 * cache, copies its first `bytes` to host_out and releases it (tests/test_work_buffers_gpu.py). */
int cyto_cache_poison(int byte);
long long cyto_cache_poison_fills(void);
long long cyto_cache_poison_bytes(void);
int cyto_cache_peek(size_t bytes, void *host_out, int device_id);

/* ---- Device inputs and caller streams: what holds for every entry point below that takes a device matrix (cost_on_device,
 * x_on_device, cyto_matrix.on_device) or a `void *stream` (tests/test_device_inputs_gpu.py, tests/test_caller_stream_gpu.py).
 *
 * Layout.  A device matrix is row-major with ANY leading dimension ld >= its width (elements) and ANY base address aligned to its
 * element; the result does not depend on either, bit for bit.  Which layouts are read where they lie, without a copy:
 *   cost (float32)        ld % 4 == 0 and a 16-byte aligned base;   cost (float64): ld % 2 == 0 and a 16-byte aligned base
 *                         (anything else is re-pitched into a work buffer by one device-to-device copy: n x ld' more bytes)
 *   cyto_transform / cyto_standardize / cyto_ctx_create_ex inputs: always in place.  The four-column kernels run when the width and
 *                         ld are multiples of 4 and the base is aligned for four elements (16 bytes for float32 and float64, 8 for
 *                         uint16, 4 for uint8) -- and z_dev is 16-byte aligned with ldz % 4 == 0; otherwise a column per lane
 *   cyto_normalized_colsums input: always in place (its column-sum pass by the same rule, its summing kernel a column per lane)
 *   cyto_cost_metric / cyto_cost_pearson operands: in place; they keep their own rule (Gpad % 32 == 0, ld % 128 == 0, the columns
 *                         between the width and the next multiple of 128 zero, as cyto_transform leaves them); cost_dev: any ldc >= C
 * Padding.  Bytes outside the n x n (nu x n, G x C) block -- the columns between the width and ld, whatever lies before the base or
 * behind the last row, stored rows no entry of a row map names -- are never interpreted: they may hold anything, NaN and infinities
 * included, and do not raise CYTO_ERR_NONFINITE.  Inputs are never written.  Of an output the call writes its block and, for z_dev,
 * the zero padding (the whole Gpad x ldz buffer outside the G x C block); nothing else, the columns between C and ldc of cost_dev
 * included.
 * Streams.  `stream` is a hipStream_t of the HIP runtime this library is linked against (NULL: the device's default stream).  All
 * device work of the call is queued on it, behind whatever the caller queued there before: an input that an earlier copy or kernel on
 * that stream is still producing is read when it is complete.  Every call returns with its work complete: host outputs are
 * filled, device outputs (z_dev, cost_dev, dense_dev) may be read at once from any stream.
 * Entry points WITHOUT a stream parameter (cyto_lap_batch_f32*, cyto_ctx_*, cyto_assign_*) run on private non-blocking streams, which
 * wait for no other stream: their device inputs must be complete before the call. */

/* ---- A5: the LAP solve.  Replaces `_, y, _ = lapjv.lapjv(cost_scaled)`
 * (cytospace/linear_assignment_solvers/linear_assignment_solvers.py:34-40; solver imported
 * at :16-18).  Jonker-Volgenant: column reduction, reduction transfer, two augmenting row
 * reduction sweeps, shortest-augmenting-path augmentation.
 *
 *   n, ld         square problem size and leading dimension (elements) of the row-major cost
 *   cost          n x n costs; host pointer (cost_on_device = 0) or device pointer (= 1)
 *   rowsol[i]     column assigned to row i                      (host, n, out; may be NULL)
 *   colsol[j]     row assigned to column j -- CytoSPACE's `y`   (host, n, out; may be NULL)
 *   u, v          dual variables                                 (host, n, out; may be NULL)
 *   total         sum_i cost[i][rowsol[i]] accumulated in f64    (out; may be NULL)
 *   info          timing/work counters                           (out; may be NULL)
 *   stream        hipStream_t to launch on, NULL = the device's default stream
 * Results are bit-identical to oracle/jv_oracle.c for the same dtype (tests/test_lap_gpu.py).
 *
 * Range of the costs.  Any finite float32 costs, subnormal values and -0.0 included (-0.0 is the cost 0), and the results depend on
 * the matrix through its values only: a matrix scaled by a power of two, without under- or overflow, gives the same indices and the
 * duals scaled by it, bit for bit.  Every intermediate (a dual, a reduced cost, a distance) stays finite when
 * 2 * n * max|c| < 2^127; beyond that bound -- costs near FLT_MAX, where c - v can overflow -- the result is unspecified.  The float64
 * solve accepts any finite float64 costs under the same bound in its own format (2^1023); its warm start narrows to float32 and falls
 * back to the cold start when the narrowed image is not finite.  Pinned by tests/test_lap_ranges_*.py against the oracle, which
 * tests/test_lap_ranges_cpu.py pins against an exact solver over the same range.
 */
typedef struct {
    double ms_colred;        /* HIP-event time of the column-reduction kernels */
    double ms_cache;         /* HIP-event time of the row-cache build kernel (float32 path; else 0) */
    double ms_chain;         /* HIP-event time of the persistent chain kernels (RT+ARR, then augmentation) */
    double ms_total;         /* sum of the three (kernel time only: no H2D/D2H, no allocation) */
    int64_t scans_colred, scans_redtransfer, scans_arr, scans_aug_init, scans_aug_relax;
    int64_t augmentations, path_hops;
    int64_t free_after_colred, free_after_arr1, free_after_arr2;
    int64_t hbm_row_reads;   /* full cost rows the kernels actually fetched from HBM */
    int64_t dense_refreshes; /* RT/ARR steps whose row cache was exhausted (full re-scan) */
    double ms_arr;           /* float32 path: the RT+ARR kernel (jv_chain2) alone; wide solver: the row-reduction phase (wide_rt, the
                                phase machine's rounds on the whole chip, wide_arr) and the cache build for the searches behind it */
    double ms_aug;           /* float32 path: the augmentation kernel alone (wide solver: wide_aug -- plus, where the searches
                                paused for fresh caches, the rebuilds and the launches after the first) */
    int64_t aug_scans_skipped; /* augmentation scans elided as provable no-ops (duplicate rows) */
    int64_t row_groups;      /* number of runs of bitwise identical consecutive rows (== n: none) */
    int64_t aug_dense_scans; /* augmentation scans that had to read the full cost row (cache certificate failed) */
    int64_t aug_sparse_inits; /* augmentations whose initial row scan was served from the row cache */
    int64_t aug_handover;    /* -1, or the index of the search at which the cache-certified augmentation handed the
                                remaining free rows to the dense kernel (its certificates kept failing) */
    /* wide solver (cyto_lap_opts.mode = 2) */
    int64_t wide;                /* 1: solved by the wide solver */
    int64_t wide_rounds;         /* Jacobi rounds of augmenting row reduction that ran */
    int64_t wide_retired;        /* rows that left the rounds on a tie (handed to the augmentation) */
    int64_t wide_dense_arr;      /* bids whose row cache could not certify the top-2 (full row read) */
    int64_t wide_dense_aug;      /* augmentation: relaxations from the full cost row (cache certificate failed) */
    int64_t wide_aug_rounds;     /* augmentation: rounds of the speculative search (16 columns settled per round at most); schedule-dependent */
    int64_t wide_aug_settled;    /* augmentation: columns settled, re-settlements after a label improved included; schedule-dependent (results are not) */
    int64_t wide_trivial;        /* augmentation: searches that ended at the free row's own best column */
    int64_t wide_verify_passes;  /* augmentation: certificate passes (>= one per non-trivial search) */
    int64_t wide_list_rounds, wide_chain_rounds;   /* row-reduction rounds in the list / chain regime */
    double wide_ms_list, wide_ms_chain;            /* time inside wide_arr spent in them (the kernels' own 100 MHz clock) */
    double wide_ms_aug_rounds, wide_ms_aug_verify, wide_ms_aug_finish, wide_ms_aug_trivial;   /* wide_aug: search rounds, certificate
                                                      passes, price update + flip + reset, one-edge searches (one-workgroup kernel) */
    int64_t wide_arr_launches;   /* row reduction: launches of the round kernel (row-cache rebuilds in between) */
    int64_t wide_aug_launches;   /* augmentation: launches of the search kernel (row-cache rebuilds in between: cyto_lap_opts.wide_rebuild) */
    int64_t wide_scaled;         /* row reduction: 1 = the instance went through the eps-scaled phases */
    int64_t wide_phases;         /* row reduction: phases begun (scaled phases + the final eps = 0 phase) */
    int64_t wide_par_batches;    /* augmentation, several searches at once (cyto_lap_opts.wide_par): batches of searches run from one state */
    int64_t wide_par_discarded;  /* ... searches that met an earlier search of their batch and ran again in the next one */
    int64_t f64_warm;            /* float64: 1 = warm-started from the prices of the float32 wide solve of the narrowed matrix */
    double f64_warm_ms;          /* float64: kernel time of that float32 solve */
    /* float32, cyto_lap_opts.certify: the float64 certificate of the result */
    int64_t certified;           /* 1: the three fields below were computed */
    double gap_f64;              /* sum_i (u_i - min_j (c[i][j] - v[j])) with u_i = c[i][rowsol[i]] - v[rowsol[i]], every difference in
                                    float64: total - optimum <= gap_f64 (0: optimal for the float32 matrix in exact arithmetic) */
    double gap_max_f64;          /* the largest term of that sum */
    int64_t gap_rows;            /* rows with a positive term (their column loses to another by a fraction of a float32 ulp) */
    int64_t polished;            /* cyto_lap_opts.polish: 1 = the certificate left a gap and the float64 polish ran (rowsol / colsol / total and
                                    the duals -- narrowed to float32 -- are the float64 solve's; gap_f64 is the float32 result's, before it) */
    double polish_ms;            /* kernel time of the polish */
    /* float32, cyto_lap_opts.exact: the repair on the near-tight edges (gap_f64 / gap_max_f64 / gap_rows above still describe the float32
       result before it) */
    int64_t exact_status;        /* 0: not asked.  1: gap_f64 was 0, the result is already optimal.  2: repaired on E.  3: E went over its cap
                                    (cyto_lap_opts.exact) and the float64 polish ran instead */
    int64_t exact_edges;         /* edges of E besides the assignment's own: sum over rows of |{j != rowsol[i] : r_ij <= tau}| */
    int64_t exact_free_rows;     /* rows the repair freed (r_ij < 0 for some j: == gap_rows) */
    int64_t exact_changed_rows;  /* rows whose column the repair changed */
    int64_t exact_overflow_rows; /* rows with more near-tight columns than the per-row slots (a second emission pass wrote them) */
    double exact_ms_emit;        /* HIP-event time of the emission passes (near_tight_rows) */
    double exact_ms_repair;      /* host wall time of building E and the sparse solve */
} cyto_lap_info;

int cyto_lap_f32(int n, const float *cost, int64_t ld, int cost_on_device,
                 int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total,
                 cyto_lap_info *info, int device_id, void *stream);
int cyto_lap_f64(int n, const double *cost, int64_t ld, int cost_on_device,
                 int32_t *rowsol, int32_t *colsol, double *u, double *v, double *total,
                 cyto_lap_info *info, int device_id, void *stream);

/* The same solves with explicit kernel-selection options.  Within one `mode`, results never depend on them (every variant realises the same
 * search, bit for bit); they exist so that the kernels the solver picks for n > 26 624 / 32 768 and the hand-over paths can
 * be exercised on instances small enough for the CPU oracle (tests/test_lap_gpu.py).  NULL = the defaults. */
typedef struct {
    int32_t chain_variant;      /* 0: by size.  1: prices in L2 (u16 colsol in LDS), cached refresh -- what n > 26 624 uses.
                                   2: streaming dense refresh -- what n > 32 768 uses.  float64: != 0 selects the streaming chain (what n > 4 096
                                   uses), 1 with its row caches, 2 without (every scan reads its row).  3: as 2 (float64: as 1) with colsol in
                                   global memory too -- what n > 65 535 uses */
    int32_t augmentation;       /* 0: by size (cache-certified search above 5 120 columns).  1: dense register-resident search
                                   (n <= 26 624 only).  2: cache-certified search */
    int32_t no_handover;        /* 1: the cache-certified search never hands deep searches over to the dense kernel */
    int32_t inject_exceptions;  /* self-test of the rounding-exception list of the cache-certified search: treat the first k
                                   columns as exception columns (k > 64 overflows the list: certificates are abandoned) */
    int32_t group_state_global; /* 1: the duplicate-row group state (best offset / search stamp per row group) in global memory even
                                   where it fits LDS -- what large problems with thousands of row groups use */
    int32_t aux_state_global;   /* 1: the dense augmentation's per-column auxiliaries (cost of the assigned entry, owner's row group) in
                                   global memory even where they fit LDS -- what n > ~13 000 uses */
    int32_t mode;               /* 0: default.  1: the chain solver (classic Gauss-Seidel order: reduction transfer and augmenting row
                                   reduction row after row, Dijkstra one column per step -- oracle/jv_oracle_impl.h, first half).
                                   2: the wide solver (Jacobi reduction transfer, Jacobi rounds of row reduction, speculative
                                   shortest paths with (distance, tight-hop) labels -- same file, "WIDE MODE"; float32).  Both reach the same optimum;
                                   the duals and, where the optimum is not unique, the particular optimal assignment differ */
    int32_t wide_rounds;        /* wide solver: budget of row-reduction rounds.  0: 4096 + n / 4.  -1: none */
    int32_t wide_groups;        /* retired (it selected a search on several workgroups, since removed): accepted in -1 ... 32 and
                                   ignored.  Results never depended on it */
    int32_t wide_rebuild;       /* wide solver, augmentation: when the searches pause for the row caches to be rebuilt by the whole chip against
                                   the prices reached (a floor goes stale as searches lower the prices; deep-search instances otherwise
                                   fall back to full cost rows).  0: when the full-row relaxations since the last rebuild have cost what
                                   a rebuild costs.  -1: never.  k > 0: every k searches.  Results do not depend on it */
    int32_t wide_par;           /* wide solver, one problem: searches of consecutive free rows that run at once, a workgroup each, from one state and
                                   are committed in row order while their settled sets are disjoint (the rest runs again).  0: 16 for a problem
                                   of >= 2 048 rows without runs of identical rows, else one at a time.  -1: one at a time.  k > 1: k (<= 64;
                                   clamped to an eighth of the device's CUs -- the workgroups, one per CU, spread over the XCDs, meet at grid barriers and must all be resident).
                                   Results do not depend on it */
    int32_t wide_wipe;          /* wide solver, row reduction: the per-column bid words carry a 12-bit round tag relative to their last wipe;
                                   0: each of the two word buffers is wiped every 1 024 of its launches.  k > 0: every k (a self-test of the protocol at sizes the CPU
                                   oracle checks).  Results do not depend on it */
    int32_t cache_waves;        /* row-cache builder (float32): 0 / -1: by size (a wave per row, 8 or 20 waves per CU).  k > 0: k waves per CU
                                   (<= 32).  (-1 selected the workgroup-per-row builders of round 3, since removed.)  Results do not depend on it */
    int32_t cache_unroll;       /* ... 16-byte quads in flight per lane of the wave builder: 0 (default: 8), 4 or 8 */
    int32_t cache_stream;       /* ... 0 / 1: the guess-free streaming selection for rows of >= 2 048 columns.  -1: a neighbouring row's floor
                                   as the guess (round 4's first form) */
    int32_t certify;            /* float32: 1 = one more pass over the matrix behind the solve proves in float64 how far from optimal the
                                   assignment can be (cyto_lap_info.gap_f64: total - optimum <= gap, rounding of the float32 duals and nothing
                                   else; ~2 ms at n = 50 000).  An instance whose optimum is unique by more than the gap has exactly the
                                   returned indices, whatever the solver's constants.  (took the first of the reserved words: same size) */
    int32_t polish;             /* float32, single problems: 1 = certify, and where the certificate cannot prove the result optimal (gap_f64 > 0)
                                   finish in float64 -- the matrix widened on the device (n^2 x 8 more bytes), the float32 prices as the start with
                                   every row free, the float64 augmenting row reduction and augmentation of the force_doubles path (~1.2 n steps):
                                   the optimum of the float32 matrix in float64 arithmetic, indices that do not depend on the float32 solver's
                                   constants.  Several times the cost of the solve: off by default.  Single problems only (cyto_lap_f32_opts,
                                   cyto_lap_f32_rowmap): a batch has no polish, and cyto_lap_batch_f32_opts with polish != 0 returns
                                   CYTO_ERR_BAD_ARG for the call (every status_out entry too) before anything is solved.
                                   cyto_ctx_assign_chunks takes no options and never polishes.  (the second of the reserved words) */
    int32_t exact;              /* float32: the optimum of the float32 matrix (computed in float64), as lapjv returns it -- for single problems,
                                   row maps and batches alike.  Implies certify.  With pi = the float32 result, v its prices, and in float64
                                   w_ij = c_ij - v_j, r_ij = w_ij - w_i,pi(i) and gap = cyto_lap_info.gap_f64, every assignment at least as
                                   good as pi lies in
                                       E = { (i, j) : r_ij <= tau },   tau = gap * (1.0 + 0x1p-30)     (float64: one rounded multiply)
                                   ("Exact option").  One more pass over the matrix emits E (the raw float32 costs), the rows
                                   with r_ij < 0 are freed and a float64 successive-shortest-path solve over E on the host finishes.
                                   v is returned unchanged; a changed row gets u_i = fl32(c_i,sigma(i) - v_sigma(i)).  gap == 0: nothing to
                                   do.  0: off.  1: on, 16 edge slots per row.  k in 2 ... 64: k slots per row (a self-test of the
                                   overflow pass).  Rows with more near-tight columns than slots are emitted again into an exact-size
                                   list; when E holds more than max(2^22, 32 n) edges the float64 polish (above) runs instead
                                   (cyto_lap_info.exact_status = 3), one problem at a time in a batch.  Not with polish, not on the
                                   float64 entry points (CYTO_ERR_BAD_ARG).  (the third of the reserved words) */
    int32_t reserved[2];        /* must be zero */
} cyto_lap_opts;
int cyto_lap_f32_opts(int n, const float *cost, int64_t ld, int cost_on_device,
                      int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total,
                      cyto_lap_info *info, int device_id, void *stream, const cyto_lap_opts *opts);
int cyto_lap_f64_opts(int n, const double *cost, int64_t ld, int cost_on_device,
                      int32_t *rowsol, int32_t *colsol, double *u, double *v, double *total,
                      cyto_lap_info *info, int device_id, void *stream, const cyto_lap_opts *opts);

/* Row indirection (first half).  calculate_cost repeats every spot row slots[s] times
 * (linear_assignment_solvers.py:63-66: `cost[location_repeat, :]`); here the cost holds every DISTINCT row once (nu x ld) and
 * rowmap[i] (host, n entries, non-decreasing like np.repeat's output, values in [0, nu)) names the stored row of LAP row i --
 * 10x less memory and streaming traffic at config c3.  Results are bit-identical to solving the materialised n x n matrix. */
int cyto_lap_f32_rowmap(int n, const float *cost_rows, int64_t ld, int nu, int cost_on_device, const int32_t *rowmap,
                        int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total,
                        cyto_lap_info *info, int device_id, void *stream, const cyto_lap_opts *opts);

/* `lapjv(cost_scaled)` as the reference calls it (linear_assignment_solvers.py:38): a float64 HOST matrix solved in
 * float32.  The matrix is uploaded as it is and narrowed on the device (same rounding as numpy's astype(float32)). */
int cyto_lap_f32_from_f64(int n, const double *cost_host, int64_t ld, int32_t *rowsol, int32_t *colsol,
                          float *u, float *v, double *total, cyto_lap_info *info, int device_id, void *stream);

/* The host half of cyto_lap_opts.exact, on its own (no device is touched): the optimum of a sparse assignment problem that contains a
 * perfect matching, from that matching.
 *   rowsol[i]            the starting assignment, a permutation of 0 ... n-1
 *   row_ptr[n + 1], cols, r   row i's edges are cols[row_ptr[i] ... row_ptr[i+1]) with float64 costs r (rowsol[i] among them;
 *                        missing edges are infinite)
 *   rowsol_out[i]        the optimum's column of row i (may alias rowsol)
 * Rows with an edge cheaper than their own are freed; the duals u_i = min_j r_ij, v = 0 are feasible and tight on the rows kept, and
 * successive shortest paths over the edges (Dijkstra with potentials, float64) re-assign the freed rows: free rows in ascending order,
 * a binary heap keyed on (distance, column), so equal distances go to the lower column.  A row whose component cannot improve keeps
 * its column.  CYTO_ERR_BAD_ARG: n <= 0, a null pointer, a column out of range, rowsol not a permutation or not among its row's
 * edges, a non-finite r. */
int cyto_lap_repair_sparse(int n, const int32_t *rowsol, const int64_t *row_ptr, const int32_t *cols, const double *r,
                           int32_t *rowsol_out);

/* ---- A8 (one GPU): nb independent LAPs solved concurrently.  Replaces the per-chunk worker processes of
 * apply_linear_assignment (cytospace/cytospace.py:430-451) for the solver-only seam: the sequential
 * chain of one solve occupies one workgroup, so chunks run side by side (one launch per phase, a workgroup per problem).
 * n[b], cost[b], ld[b]: per problem; outputs are arrays of per-problem host pointers (each may be NULL);
 * total/info/status_out: arrays of length nb (may be NULL).  max_concurrent <= 0 -> min(nb, 256). */
int cyto_lap_batch_f32(int nb, const int *n, const float *const *cost, const int64_t *ld, int cost_on_device,
                       int32_t *const *rowsol, int32_t *const *colsol, float *const *u, float *const *v,
                       double *total, cyto_lap_info *info, int *status_out, int max_concurrent, int device_id);

int cyto_lap_batch_f32_opts(int nb, const int *n, const float *const *cost, const int64_t *ld, int cost_on_device,
                            int32_t *const *rowsol, int32_t *const *colsol, float *const *u, float *const *v,
                            double *total, cyto_lap_info *info, int *status_out, int max_concurrent, int device_id,
                            const cyto_lap_opts *opts);     /* opts->mode selects the solver for the whole batch (NULL: defaults);
                                                               opts->polish != 0: CYTO_ERR_BAD_ARG, nothing is solved */

/* ---- A8 (several GPUs, one process each): the only collective on the path is the broadcast of the
 * shared standardised ST matrix (RCCL over xGMI).  id128: 128-byte ncclUniqueId made on one rank by
 * cyto_comm_unique_id and handed to the others by the launcher (bench/driver: torch.distributed, MPI,
 * a file ...).  The reference has no counterpart: it pickles the matrix to every worker (cytospace.py:446-451). */
int cyto_comm_unique_id(char *id128);
int cyto_comm_init(const char *id128, int rank, int nranks, int device_id, void **comm_out);
/* One PROCESS driving several devices, one host thread per rank -- what apply_linear_assignment's `number_of_processors` pool
 * (cytospace.py:430-451) becomes on a multi-GPU node without a launcher: comms_out[r] is the handle rank r's thread uses, on
 * device_ids[r].  Distinct devices: RCCL (ncclCommInitAll).  A device listed more than once ("logical" ranks: several workers
 * on one GPU): the ranks meet inside the process and the broadcast is a device-to-device / peer copy out of the root's buffer. */
int cyto_comm_init_local(int nranks, const int *device_ids, void **comms_out);
int cyto_comm_count(void *comm, int *nranks_out);      /* ranks the communicator spans (RCCL: ncclCommCount) */
int cyto_comm_kind(void *comm, int *kind_out);         /* 0: RCCL, 1: in-process (logical ranks) */
int cyto_comm_bcast_f32(void *comm, float *dev_buf, size_t count, int root, int device_id, void *stream);
/* *status := the largest status any rank brought (0: all fine).  Collective: how the ranks agree to enter or skip a data
 * collective together. */
int cyto_comm_agree(void *comm, int *status);
/* For a rank that cannot reach a collective its peers wait in (its host code failed first): in-process kind -- the waiting ranks
 * return CYTO_ERR_PEER; RCCL kind -- ncclCommAbort of this rank's communicator and, for communicators made by
 * cyto_comm_init_local (host threads of one process), of EVERY sibling's: ranks already inside a collective are released and
 * return CYTO_ERR_PEER, as does every later collective on any of the handles.  Afterwards the handles are good for
 * cyto_comm_destroy only.  cyto_comm_aborted: 1 once that has happened. */
int cyto_comm_abort(void *comm);
int cyto_comm_aborted(void *comm, int *aborted_out);
int cyto_comm_destroy(void *comm);

/* ---- element types of the expression matrices at this boundary.  Every `x_is_f64` parameter below and cyto_matrix.is_f64 carry one
 * of these (0 and 1 mean what the name says; 2 and 3 came in round 6): raw counts are small integers, and a uint16 / uint8 matrix is a
 * half / a quarter of the float32 upload -- the transform kernels widen in their loads, the numbers are the same bit for bit. */
enum { CYTO_DTYPE_F32 = 0, CYTO_DTYPE_F64 = 1, CYTO_DTYPE_U16 = 2, CYTO_DTYPE_U8 = 3, CYTO_DTYPE_I32 = 4, CYTO_DTYPE_I64 = 5 };
/* (CYTO_DTYPE_I32 / _I64: integer matrices of cyto_downsample and cyto_mtx_write only) */

/* ---- A1: normalize_data (cytospace/common/common.py:142-147): nan_to_num, per-column counts per
 * million over the gene axis, log2(x + 1), nan_to_num.  x: G x C host matrix (float64 if x_is_f64
 * else float32; CYTO_DTYPE_*), out: G x C host float64.  Computed on the device in float64. */
int cyto_normalize_data(int G, int C, const void *x, int64_t ldx, int x_is_f64, double *out, int64_t ldo,
                        int device_id);

/* ---- A1 + first half of A2: per-column normalise (skipped if already_normalized) and standardise:
 *   z[g][c] = (y[g][c] - mean_c) / (std_c * sqrt(G))   (population std, like numpy's .std(0))
 * written as float32 into the DEVICE buffer z_dev (Gpad x ldz, zero padded by this call;
 * Gpad % 32 == 0 and ldz % 128 == 0 are what cyto_cost_pearson needs).  x may be a host or a
 * device pointer.  With these z the contraction of cyto_cost_pearson IS the Pearson correlation
 * of matrix_correlation_pearson (cytospace/common/common.py:190-199). */
int cyto_standardize(int G, int C, const void *x, int64_t ldx, int x_is_f64, int x_on_device,
                     int already_normalized, float *z_dev, int64_t ldz, int Gpad, int device_id, void *stream);

/* ---- second half of A2 + A3: cost = -corr on the fp32 matrix cores, each spot row written to its
 * slots[s] consecutive LAP rows in spot order (calculate_cost, lapjv/Pearson branch:
 * cytospace/linear_assignment_solvers/linear_assignment_solvers.py:42-69).
 * zst: Gpad x ldzst, zsc: Gpad x ldzsc (device); slots: host int64[S]; cost_dev: device,
 * (sum slots) x ldc float32.  gemm_ms (optional) = HIP-event time of the GEMM kernel. */
int cyto_cost_pearson(int Gpad, int S, int C, const float *zst, int64_t ldzst, const float *zsc, int64_t ldzsc,
                      const int64_t *slots, float *cost_dev, int64_t ldc, double *gemm_ms, int device_id,
                      void *stream);

/* ---- A7: the fused per-chunk path.  Replaces solve_linear_assignment_problem
 * (cytospace/cytospace.py:304-351) for solver_method "lapjv" + "Pearson_correlation": cost build and
 * JV solve on the device; mapped_spot[c] = index (into st's columns) of the spot cell c is mapped to.
 * sc: G x C, st: G x S host float64 row-major; slots: int64[S] with sum == C (square LAP).
 * ValueError-equivalents: CYTO_ERR_BAD_ARG (not square), CYTO_ERR_NONFINITE (zero-variance column). */
typedef struct {
    double ms_standardize;   /* normalise + standardise kernels incl. the H2D copies of sc and st */
    double ms_gemm;          /* HIP-event time of the MFMA cost GEMM */
    double gemm_flops;       /* 2 * Gpad * S * C */
    cyto_lap_info lap;
} cyto_assign_info;

int cyto_assign_pearson(int G, int C, int S, const double *sc, const double *st, const int64_t *slots,
                        int already_normalized, int64_t *mapped_spot, double *total_cost,
                        cyto_assign_info *info, int device_id);

/* ---- the other distance metrics of calculate_cost
 * (cytospace/linear_assignment_solvers/linear_assignment_solvers.py:53-59) through the same contraction.
 * Spearman_correlation: matrix_correlation_spearman (cytospace/common/common.py:202-215) = per-column average-tie
 * ranks (pandas rank() defaults), then the Pearson formula; Euclidean: scipy cdist(..., 'euclidean') transposed.
 * cyto_transform writes the float32 GEMM operand of one matrix: standardised values, standardised ranks, or the
 * plain values; cyto_cost_metric / cyto_assign_metric are cyto_cost_pearson / cyto_assign_pearson with a metric. */
enum { CYTO_METRIC_PEARSON = 0, CYTO_METRIC_SPEARMAN = 1, CYTO_METRIC_EUCLIDEAN = 2 };
enum { CYTO_TRANSFORM_STANDARDIZE = 0, CYTO_TRANSFORM_RANK = 1, CYTO_TRANSFORM_RAW = 2 };
int cyto_transform(int transform, int G, int C, const void *x, int64_t ldx, int x_is_f64, int x_on_device,
                   int already_normalized, float *z_dev, int64_t ldz, int Gpad, int device_id, void *stream);
int cyto_cost_metric(int metric, int Gpad, int S, int C, const float *zst, int64_t ldzst, const float *zsc, int64_t ldzsc,
                     const int64_t *slots, float *cost_dev, int64_t ldc, double *gemm_ms, int device_id, void *stream);
int cyto_assign_metric(int metric, int G, int C, int S, const double *sc, const double *st, const int64_t *slots,
                       int already_normalized, int64_t *mapped_spot, double *total_cost,
                       cyto_assign_info *info, int device_id);


/* ---- A8, the multi-chunk seam: apply_linear_assignment (cytospace/cytospace.py:354-469) normalises the two
 * matrices once and submits one solve_linear_assignment_problem per chunk, each with a column subset of the
 * scRNA matrix and either a column subset of the ST matrix (--single-cell, :434-435) or the full ST matrix with
 * per-chunk slot counts (--sampling-sub-spots, :438-439).  Here the matrices are uploaded and transformed once
 * into a device-resident context; a chunk gathers its columns out of it (spots with slots == 0 are not
 * contracted).  mapped_spot[c] = position in the chunk's spot list, as the reference's per-chunk result.
 * cyto_ctx_assign_chunk may be called concurrently from several host threads on one context. */
typedef struct cyto_expr_ctx cyto_expr_ctx;
int cyto_ctx_create(int metric, int G, int C, int S, const double *sc, const double *st, int already_normalized,
                    int device_id, cyto_expr_ctx **out);
int cyto_ctx_assign_chunk(cyto_expr_ctx *ctx, const int64_t *idx_sc, int n_sc, const int64_t *idx_st, int n_st,
                          const int64_t *slots, int64_t *mapped_spot, double *total_cost, cyto_assign_info *info);
void cyto_ctx_destroy(cyto_expr_ctx *ctx);

/* One process per GPU (cytospace.py:430-451 forks one worker per chunk and pickles the whole ST matrix to each): only rank
 * `root` holds the ST matrix; it transforms it once and the float32 operand reaches the other ranks with ONE broadcast over
 * xGMI (comm from cyto_comm_init; RCCL) -- the only collective of the path.  sc / C are THIS rank's cells only (raw counts
 * with already_normalized = 0: nothing normalised ever crosses PCIe twice).  st may be NULL on ranks != root.
 * bcast_ms (optional): HIP-event time of the broadcast. */
int cyto_ctx_create_shared(int metric, int G, int C, int S, const void *sc, const void *st, int x_is_f64, int already_normalized,
                           void *comm, int root, int rank, int device_id, cyto_expr_ctx **out, double *bcast_ms);

/* The general form: each matrix is a dense genes x columns array on the host or ALREADY ON THE DEVICE (e.g. expanded from sparse
 * counts by cyto_csc_to_dense_f32), float32 or float64, with its own leading dimension.  comm == NULL: no broadcast. */
typedef struct {
    const void *data;
    int64_t ld;              /* elements per row (>= number of columns) */
    int32_t is_f64;          /* the element type, CYTO_DTYPE_*: 0 float32, 1 float64 (what the name says), 2 uint16, 3 uint8 */
    int32_t on_device;       /* 1: device pointer */
} cyto_matrix;
int cyto_ctx_create_ex(int metric, int G, const cyto_matrix *sc, int C, const cyto_matrix *st, int S, int already_normalized,
                       void *comm, int root, int rank, int device_id, cyto_expr_ctx **out, double *bcast_ms);

/* ---- The per-spot reads of estimate_cell_number_RNA_reads (cytospace/cytospace.py:116-134): sums[c] = the sum over the G genes of
 * normalize_data's column c, i.e. numpy's `normalize_data(x).sum(axis=0)`, with the SAME float64 bits -- the values
 * cyto_normalize_data writes (the library log2, the same column sums), added in ascending gene order with one float64 add per gene,
 * as numpy adds the rows of a C-contiguous matrix -- and without the G x C float64 matrix: nothing of that size is written to HBM
 * or crosses PCIe; the temporaries are the column-sum partials and 2 C doubles.  (C == 1 is the one shape where numpy's order is
 * another: a single column is a contiguous vector, which numpy adds pairwise.  This call adds in gene order for every C;
 * common.normalized_column_sums lets numpy add a single column.)
 *   x      G x C matrix of CYTO_DTYPE_F32 / _F64 / _U16 / _U8 (x->is_f64); the sums do not depend on the dtype where it holds the
 *          values exactly.  on_device = 0: a host matrix, uploaded as it is.  on_device = 1: read where it lies, under the rules of
 *          "Device inputs and caller streams" above (any ld >= C, any element-aligned base, padding never interpreted).
 *   sums   host float64[C], filled when the call returns
 *   stream as every `void *stream` above
 * CYTO_ERR_BAD_ARG, before the device is touched: G <= 0, C <= 0, a null pointer, ld < C, another dtype.
 * cyto_normalized_colsums_timed: the same call; kernel_ms (optional) = HIP-event time of the summing kernel alone (without the
 * column-sum pass before it, the upload and the download). */
int cyto_normalized_colsums(int G, int C, const cyto_matrix *x, double *sums, int device_id, void *stream);
int cyto_normalized_colsums_timed(int G, int C, const cyto_matrix *x, double *sums, int device_id, void *stream, double *kernel_ms);

/* SURVEY 8(f) rank 2, device-side staging: sparse counts as the reference reads them from a 10x MatrixMarket file
 * (scipy.io.mmread, cytospace/common/common.py:49; CSC: colptr[C + 1], rowidx[nnz], vals[nnz], host arrays) are uploaded as
 * non-zeros and expanded into the dense float32 G x ld DEVICE matrix the transforms read (zero filled here).  The reference
 * densifies on the host (common.py:57).  CYTO_ERR_BAD_ARG: malformed colptr or a row index outside [0, G). */
int cyto_csc_to_dense_f32(int G, int C, int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const float *vals,
                          float *dense_dev, int64_t ld, int device_id, void *stream);

/* Every chunk of a rank in one call: per chunk the column gathers and the cost GEMM, then ALL the chunks' LAPs together (a
 * workgroup per chunk in every chain phase: cyto_lap_batch_f32).  Fields as cyto_ctx_assign_chunk's arguments; status, total_cost
 * and info are outputs.  max_concurrent bounds the chunks whose cost matrices exist at once (<= 0: min(nchunks, 64)). */
typedef struct {
    const int64_t *idx_sc; int32_t n_sc;
    const int64_t *idx_st; int32_t n_st;          /* NULL / ignored: all S spots */
    const int64_t *slots;
    int64_t *mapped_spot;                          /* out, n_sc entries */
    double total_cost;                             /* out */
    int32_t status;                                /* out */
    cyto_assign_info info;                         /* out */
} cyto_chunk;
int cyto_ctx_assign_chunks(cyto_expr_ctx *ctx, int nchunks, cyto_chunk *chunks, int max_concurrent);

/* The same two entry points for float32 host matrices (x_is_f64 = 0): half the host-to-device traffic, identical
 * results for data that is exactly representable in float32 (raw counts); the reference's own arrays are float64. */
int cyto_assign_metric_typed(int metric, int G, int C, int S, const void *sc, const void *st, int x_is_f64,
                             const int64_t *slots, int already_normalized, int64_t *mapped_spot, double *total_cost,
                             cyto_assign_info *info, int device_id);
int cyto_ctx_create_typed(int metric, int G, int C, int S, const void *sc, const void *st, int x_is_f64,
                          int already_normalized, int device_id, cyto_expr_ctx **out);
/* ... and with an element type PER MATRIX: scRNA counts as uint8 beside ST counts as uint16, say -- what
 * cytospace_amd.cytospace.assign_pearson passes for integer count matrices (config c3: the upload bounds the call).  A host matrix has
 * ld == columns; a matrix with on_device = 1 (any ld >= columns; complete before the call, which runs on a private stream) is
 * transformed where it lies, with the same results bit for bit. */
int cyto_assign_metric_ex(int metric, int G, const cyto_matrix *sc, int C, const cyto_matrix *st, int S, const int64_t *slots,
                          int already_normalized, int64_t *mapped_spot, double *total_cost, cyto_assign_info *info, int device_id);

/* ---- downsample (cytospace/common/common.py:149-173): every cell (column) whose total T exceeds `target` is replaced by the
 * histogram of `target` draws with replacement from its transcripts, with exactly the words numpy's legacy global RandomState
 * (MT19937) would use: per draw, 32-bit words w until (w & mask) <= T-1, mask = 2^bitlength(T-1) - 1; cells in column order;
 * cells with T <= target are copied and take no words.  x: G x C host matrix (ldx) of CYTO_DTYPE_U8 / _U16 / _I32 / _I64;
 * out: G x C host matrix (ldo) of CYTO_DTYPE_I64 or CYTO_DTYPE_U16 (target <= 65535, no negative count anywhere).
 * key[624] / *pos: numpy's state (get_state()[1:3]) in, the state after the last consumed word out (pos == 624 when that word
 * ends the key: the twist is deferred, as numpy defers it).  *words_out (may be NULL): raw words consumed.
 * CYTO_ERR_BAD_ARG, before any word is drawn: a negative count in a cell that is downsampled (np.repeat's ValueError), a
 * downsampled cell with T > 2^32 when target > 0 (numpy draws 64-bit words there), a bad dtype or size. */
int cyto_downsample(int G, int C, const void *x, int64_t ldx, int x_dtype, void *out, int64_t ldo, int out_dtype, int target,
                    uint32_t *key, int32_t *pos, int64_t *words_out, int device_id);
/* The same with x and out ALREADY ON THE DEVICE (two distinct buffers, any leading dimensions >= C): the same kernels, draws, key / pos /
 * words semantics and CYTO_ERR_BAD_ARG cases (and x_dev == out_dev); nothing but the per-cell totals and the generator's state crosses
 * PCIe.  Returns with out_dev complete. */
int cyto_downsample_dev(int G, int C, const void *x_dev, int64_t ldx, int x_dtype, void *out_dev, int64_t ldo, int out_dtype, int target,
                        uint32_t *key, int32_t *pos, int64_t *words_out, int device_id);
/* ---- place-holder cells (cytospace/cytospace.py:212-301, sampling_method "place_holders"): short_count synthetic cells of a cell
 * type with n cells, gene g of each drawn independently from the type's n values of that gene -- the reference's
 * fake[:, k] = [np.random.choice(own[g, :]) for g in range(G)], k = 0 .. short_count-1, with exactly the words numpy's legacy global
 * RandomState would use: per (cell, gene), in that order, 32-bit words w until (w & mask) <= n-1, and NO word when n == 1.
 * own: G x n host matrix (ld_own >= n) of CYTO_DTYPE_I64 / _U16 / _F64; out: G x short_count host float64 (ldo >= short_count),
 * out[g][k] = (double) own[g][draw(k, g)] (the plain cast, round to nearest).  key[624] / *pos / *words_out: as in cyto_downsample.
 * rbuf_bytes: 0, or a cap on the draws of one block of synthetic cells (at most the library's default; at least one cell per block):
 * results never depend on it (tests force many blocks at small sizes with it).
 * CYTO_ERR_BAD_ARG, before the device is selected: G <= 0, n <= 0, short_count < 0, a null pointer, ld_own < n, ldo < short_count, another
 * dtype, rbuf_bytes < 0, *pos outside [0, 624].  short_count == 0: CYTO_OK, out and the state untouched. */
int cyto_placeholders(int G, int n, const void *own, int64_t ld_own, int own_dtype, int64_t short_count, double *out, int64_t ldo,
                      uint32_t *key, int32_t *pos, int64_t *words_out, int64_t rbuf_bytes, int device_id);
/* The generator alone (a test hook): the next n raw 32-bit MT19937 words from (key, *pos), with the state after them. */
int cyto_mt19937_fill(uint32_t *key, int32_t *pos, int n, uint32_t *words, int device_id);

/* ---- dense delimited text tables (cytospace_amd.common.read_file_device): pd.read_csv(path, sep, header=0, index_col=0) on the
 * device.  The caller parses the header line; the data lines start at byte data_offset and each holds a row label and ncols values
 * (sep ',' or '\t').  On success *out is a handle and shape = {G data lines, C = ncols, bytes of the packed labels}.
 * CYTO_ERR_UNSUPPORTED: the file is outside the grammar and nothing is returned but reason = {CYTO_TABLE_ERR_*,
 * the file's line (1-based, the header is line 1; 0 if none), the byte offset (the column for CYTO_TABLE_ERR_INT_CAST)}.
 * Which refusal a file with several gets: (1) data_offset at or beyond the file's end: {BLANK, 2, the file's size}; (2) else the
 * lowest byte of the data region holding a '"' (QUOTE), a '\r' not followed by '\n' inside the file (CR) or a control byte
 * (BYTE), wherever the defects below are; (3) else the lowest (byte, kind) among an empty line, a line of one '\r' included
 * (BLANK, the line's first byte), a line without exactly ncols delimiters (FIELDS, the line's first byte) and, among the first
 * ncols values of a line only, a value outside the grammar (TOKEN) or out of range (RANGE), at its first byte; (4) else the lowest
 * column with both a decimal token and a "-0" or 17/18-digit integer token: {INT_CAST, 0, the column}.
 * ms (may be NULL): {host file reads, what the upload added to them, kernels and the small copies between them}. */
typedef struct cyto_table cyto_table;
enum {
    CYTO_TABLE_ERR_IO = 1,        /* not a readable regular file, or it shrank while read */
    CYTO_TABLE_ERR_BYTE = 2,      /* a control byte other than the delimiter, '\r', '\n' */
    CYTO_TABLE_ERR_QUOTE = 3,     /* '"' in a data line */
    CYTO_TABLE_ERR_CR = 4,        /* '\r' not followed by '\n' */
    CYTO_TABLE_ERR_BLANK = 5,     /* an empty data line, or none at all */
    CYTO_TABLE_ERR_FIELDS = 6,    /* a data line without exactly ncols delimiters */
    CYTO_TABLE_ERR_TOKEN = 7,     /* a value outside the integer / decimal token grammar (NA, empty, text, 19+ digits before the point) */
    CYTO_TABLE_ERR_RANGE = 8,     /* a decimal token whose value is +-inf or whose decimal exponent exceeds 308 */
    CYTO_TABLE_ERR_INT_CAST = 9   /* a float64 column with an integer token of 17 or 18 digits or a negative zero ("-0"): pandas'
                                     block-wise int64 cast of it may differ from the decimal converter */
};
int cyto_table_read(const char *path, char sep, int64_t data_offset, int64_t ncols, int device_id, cyto_table **out, int64_t *shape,
                    int64_t *reason, double *ms);
/* values: G x C int64 words, row-major (a float64 column's words are its values' bits); col_is_float: C flags; labels: the row
 * labels, each followed by sep and '\n' (shape[2] bytes); *ms_download (may be NULL). */
int cyto_table_fetch(cyto_table *t, int64_t *values, int8_t *col_is_float, char *labels, double *ms_download);
/* The parsed values where they lie (cytospace_amd.resident.DeviceFrame): *values_dev is a BORROWED device pointer to the G x C int64
 * words, row-major with leading dimension *ld, valid until cyto_table_free; no device is touched.  cyto_table_fetch_labels is
 * cyto_table_fetch without the values. */
int cyto_table_values(cyto_table *t, const void **values_dev, int64_t *ld);
int cyto_table_fetch_labels(cyto_table *t, int8_t *col_is_float, char *labels, double *ms_download);
void cyto_table_free(cyto_table *t);
/* The converter alone, on the host (a test hook): token i is text[offsets[i], offsets[i+1]); kinds[i] 0 integer token (ints[i],
 * and values[i] as a decimal), 1 decimal token (values[i]), 2 outside the token grammar, 3 out of range. */
int cyto_table_parse_tokens(const char *text, int64_t n, const int64_t *offsets, double *values, int64_t *ints, int8_t *kinds);

/* ---- flags of the two text writers' _ex entry points (cyto_mtx_write_ex, cyto_csv_write_ex and the host hooks).  0: the grammar of
 * cyto_mtx_write / cyto_csv_write, bit for bit.  Any other bit than those named here: CYTO_ERR_BAD_ARG before a device is touched.
 * CYTO_TEXT_FRACTIONS: every finite float32 / float64 value is written, by the shortest decimal digits that read back as the same value
 * of ITS type (among the shortest, those closest to the value): what repr(float), numpy and scipy print.  Let d1 d2 ... dk be those
 * digits and e the decimal exponent of d1.
 *   MatrixMarket:   [-]d1[.d2...dk][E<e>], no E part when e = 0, the exponent without '+' or padding: 1E-1, 2.5, 5E-324.
 *   CSV, float64:   repr(float): for -4 <= e < 16 positional with at least one digit after the point (0.0001, 2.5, 9007199254740992.0),
 *                   else d1[.d2...dk]e[+-]XX with at least two exponent digits (1e-05, 1.5e+20).
 *   CSV, float32:   numpy's text of a float32: the same two forms, the scientific one when |v| < 1e-4 or |v| >= 1e16 (by the value:
 *                   float32(1e-4) lies below 1e-4 and is 1e-04).
 * The longest texts: 24 bytes for a float64 in either layout, 19 for a float32 in CSV.  Only NaN and +-inf are still refused
 * (CYTO_*_ERR_NONFINITE); CYTO_*_ERR_FRACTION and CYTO_*_ERR_MAGNITUDE are never reported.  The integer types are not affected. */
enum { CYTO_TEXT_FRACTIONS = 1 };
/* The digits alone, on the host (test hooks; no device).  values: n float32 / float64 (CYTO_DTYPE_F32 / _F64), the sign is ignored:
 * values[i] = digits[i] * 10^exp10[i], digits[i] without a trailing zero, below 10^9 / 10^17; a zero gives (0, 0).  CYTO_ERR_BAD_ARG at
 * a NaN or an infinity.  It is the function the device calls (csrc/shortest.h). */
int cyto_shortest_digits(const void *values, int dtype, int64_t n, uint64_t *digits, int32_t *exp10);
/* out[0], out[1] := the high and low word of the routine's table entry for 10^k, ceil(10^k * 2^(127 - floor(log2(10^k)))),
 * -292 <= k <= 324 (else CYTO_ERR_BAD_ARG). */
int cyto_text_pow10(int k, uint64_t out[2]);

/* ---- the assigned-expression MatrixMarket file (cytospace_amd.post_processing.write_mtx_device): what
 * scipy.io.mmwrite(path, coo_matrix(X[:, cols])) writes, byte for byte, formatted on the device.
 * x: G x N host matrix (ldx) of any CYTO_DTYPE_*; cols: C source columns in [0, N), in file order, repeats allowed; G, C < 2^31.
 * The field is "integer" for the integer types and "real" for float32 / float64 -- and "real" for any type when no
 * entry is non-zero, as scipy has it.  block_bytes: the most text formatted per device
 * buffer (whole genes; a gene with more text stands alone), 0 for the default (32 MiB).
 * CYTO_ERR_UNSUPPORTED: info->reason says why, and nothing is left at `path` (as after any other failure):
 * a real non-zero that is not finite, not an integer, or not below 2^53 (2^24 in a float32 matrix: scipy writes a float32's
 * shortest digits, which above 2^24 are not the integer's own); G == C (scipy looks for symmetry in square matrices); the file cannot
 * be created or written. */
enum {
    CYTO_MTX_ERR_FRACTION = 2,    /* a real value with a fractional part */
    CYTO_MTX_ERR_NONFINITE = 3,   /* NaN or +-inf */
    CYTO_MTX_ERR_MAGNITUDE = 4,   /* a real value of magnitude >= 2^53 (float32: >= 2^24) */
    CYTO_MTX_ERR_SQUARE = 5,      /* G == C */
    CYTO_MTX_ERR_IO = 6           /* open() or write() failed */
};
typedef struct cyto_mtx_info {
    int64_t nnz, bytes;           /* entries written; bytes of the file, header included */
    int64_t blocks;               /* device buffers the body took */
    int32_t field;                /* 0 integer, 1 real (also: no entries) */
    int32_t reason;               /* CYTO_MTX_ERR_* with CYTO_ERR_UNSUPPORTED, else 0 */
    double ms_upload;             /* the matrix and the column list, host to device */
    double ms_kernels;            /* the count pass (with its small copies) and the format launches (device events) */
    double ms_download;           /* the blocks' copies into pinned memory (device events; they overlap the other phases) */
    double ms_write;              /* write() calls */
} cyto_mtx_info;
int cyto_mtx_write(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   int64_t block_bytes, int device_id, cyto_mtx_info *info);
/* The same with flags (CYTO_TEXT_FRACTIONS: no real value but a NaN or an infinity is refused); cyto_mtx_write is flags = 0. */
int cyto_mtx_write_ex(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                      int64_t block_bytes, int device_id, int flags, cyto_mtx_info *info);
/* The same with x ALREADY ON THE DEVICE (G x ldx elements, read where they lie): the same bytes; info->ms_upload counts the column
 * list only.  flags as cyto_mtx_write_ex's (the device form adds no bit). */
int cyto_mtx_write_dev(const char *path, int64_t G, int64_t N, const void *x_dev, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                       int64_t block_bytes, int device_id, int flags, cyto_mtx_info *info);
/* The formatter alone, on the host (a test hook): entry i is (rows[i], cols[i], values[i]), 0-based, values of CYTO_DTYPE_* dtype; its
 * line is out[offsets[i], offsets[i + 1]) -- empty for a zero, which the writer skips.  out holds 64 * n bytes, offsets n + 1 words.
 * CYTO_ERR_UNSUPPORTED at the first real value outside the device grammar. */
int cyto_mtx_format_entries(const int64_t *rows, const int64_t *cols, const void *values, int dtype, int64_t n, char *out,
                            int64_t *offsets);
int cyto_mtx_format_entries_ex(const int64_t *rows, const int64_t *cols, const void *values, int dtype, int64_t n, char *out,
                               int64_t *offsets, int flags);

/* ---- the place-holder expression table, <prefix>new_scRNA.csv (cytospace_amd.post_processing.write_csv_device): what pandas'
 * DataFrame.to_csv writes for the genes x selected-cells frame, byte for byte, the value fields formatted on the device (DESIGN.md
 * 4.1d').  x: G x N host matrix (ldx) of any CYTO_DTYPE_*; cols: C source columns in [0, N), in file order, repeats allowed;
 * G, C < 2^31.  The file is `header` (header_len bytes: the whole first line with its '\n', the caller's: quoting rules apply to it),
 * then per gene g the bytes labels[label_off[g], label_off[g + 1]) (the caller's too: the quoted label WITH its trailing ','), the C
 * values separated by ',' and a '\n'.  An integer type's value is its decimal digits; a float32 / float64 value that is an integer is
 * the integer's digits and ".0", with a '-' in front when the sign bit is set ("-0.0").  The source rows go up in slabs of whole genes
 * (two streams, two device and two pinned buffers: slab k + 1 is formatted while slab k is written), so device memory stays bounded
 * whatever G is; block_bytes: the most text per slab, by the longest field the type can have (0: 32 MiB; a gene with more stands alone).
 * CYTO_ERR_BAD_ARG, before any device is touched: a null pointer, G, N, C <= 0, header_len < 0, block_bytes < 0, ldx < N, a
 * column outside [0, N), an unknown dtype, label_off negative or decreasing.
 * CYTO_ERR_UNSUPPORTED: info->reason = CYTO_CSV_ERR_*, and nothing is left at `path` (not even a file that was there before): the
 * caller has pandas write the file.  A value is refused while the device counts its slab, so a late one removes a partial file. */
enum {
    CYTO_CSV_ERR_FRACTION = 2,    /* a real value with a fractional part */
    CYTO_CSV_ERR_NONFINITE = 3,   /* NaN or +-inf */
    CYTO_CSV_ERR_MAGNITUDE = 4,   /* a real value of magnitude >= 2^53 (float32: >= 2^24) */
    CYTO_CSV_ERR_IO = 6           /* open() or write() failed */
};
typedef struct cyto_csv_info {
    int64_t bytes;                /* bytes of the file, header included */
    int64_t blocks;               /* slabs the body took */
    int32_t reason;               /* CYTO_CSV_ERR_* with CYTO_ERR_UNSUPPORTED, else 0 */
    int32_t reserved;
    double ms_upload;             /* the slabs' source rows, label offsets and label bytes, host to device (device events); the column
                                     list goes up once before the first slab and is not counted */
    double ms_kernels;            /* count, scan and format launches (device events) */
    double ms_download;           /* the slabs' text into pinned memory (device events; overlaps the other phases) */
    double ms_write;              /* write() calls */
} cyto_csv_info;
int cyto_csv_write(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                   const char *header, int64_t header_len, const char *labels, const int64_t *label_off, int64_t block_bytes,
                   int device_id, cyto_csv_info *info);
/* The same with flags (CYTO_TEXT_FRACTIONS: no real value but a NaN or an infinity is refused; a slab's text is then bounded by 25
 * bytes per float64 field and 20 per float32 field); cyto_csv_write is flags = 0. */
int cyto_csv_write_ex(const char *path, int64_t G, int64_t N, const void *x, int64_t ldx, int x_dtype, const int64_t *cols, int64_t C,
                      const char *header, int64_t header_len, const char *labels, const int64_t *label_off, int64_t block_bytes,
                      int device_id, int flags, cyto_csv_info *info);
/* The field formatter alone, on the host (a test hook): the text of values[i] (CYTO_DTYPE_* dtype), without a separator, is
 * out[sum of lens[0 .. i), + lens[i]).  cap: the bytes of out, at least 20 * n.  CYTO_ERR_UNSUPPORTED at the first real value outside
 * the device grammar (lens[i] := -CYTO_CSV_ERR_* there). */
int cyto_csv_format_fields(const void *values, int dtype, int64_t n, char *out, int64_t cap, int32_t *lens);
/* The same with flags; cap is then at least 24 * n. */
int cyto_csv_format_fields_ex(const void *values, int dtype, int64_t n, char *out, int64_t cap, int32_t *lens, int flags);

/* ---- a MatrixMarket coordinate file read dense (cytospace_amd.common.read_mtx_device): what scipy.io.mmread(path).toarray() holds,
 * parsed and scattered on the device.  The caller parses the banner, the comments and the size line "G C nnz"; the
 * nnz entry lines "row col value" start at byte data_offset.  field: 0 integer (out: int64 values, duplicate entries summed with
 * int64 wrap-around), 1 real (out: float64 bits).  out: G x ldo host words, of which the call writes the first C of every row.
 * CYTO_ERR_BAD_ARG, before any device is touched: a null pointer, G <= 0, C <= 0, nnz < 0, data_offset < 0, ldo < C, another field.
 * CYTO_ERR_UNSUPPORTED: the body is outside the grammar and `out` is undefined; info->reason_kind = CYTO_MTXR_ERR_*, reason_line
 * the file's line (1-based; 0 if none), reason_byte the byte offset.  Which refusal a file with several gets: (1) IO, MEMORY;
 * (2) the lowest byte at or after data_offset that is outside the allowed set (BYTE) or a '\r' not followed by '\n' (CR);
 * (3) a line count other than nnz: {COUNT, 0, the lines found}; (4) the lowest (byte, kind) among an empty line (BLANK) and a line
 * without exactly three tokens (FIELDS), both at the line's first byte, an index outside [0-9]{1,18} or its range (INDEX) and a
 * value outside its grammar (TOKEN, INEXACT, NEGZERO), at the token's first byte; (5) real field: the second entry, in file order,
 * of the first cell to hold two non-zero entries (DUPLICATE, at the line's first byte). */
enum {
    CYTO_MTXR_ERR_IO = 1,         /* not a readable regular file, shorter than data_offset, or it shrank while read */
    CYTO_MTXR_ERR_BYTE = 2,       /* a byte other than digits - . e E + space tab '\r' '\n', or a blank as the file's last byte */
    CYTO_MTXR_ERR_CR = 3,         /* '\r' not followed by '\n' */
    CYTO_MTXR_ERR_COUNT = 4,      /* the body does not have exactly nnz lines */
    CYTO_MTXR_ERR_BLANK = 5,      /* an empty line */
    CYTO_MTXR_ERR_FIELDS = 6,     /* a line without exactly three tokens */
    CYTO_MTXR_ERR_INDEX = 7,      /* a row or column outside [0-9]{1,18}, below 1 or above G / C */
    CYTO_MTXR_ERR_TOKEN = 8,      /* a value outside the field's token grammar */
    CYTO_MTXR_ERR_INEXACT = 9,    /* a real value outside the window in which one IEEE operation gives the correctly rounded value */
    CYTO_MTXR_ERR_NEGZERO = 10,   /* a real zero with a minus sign */
    CYTO_MTXR_ERR_DUPLICATE = 11, /* real field: two non-zero entries in one cell (a float sum depends on the order) */
    CYTO_MTXR_ERR_MEMORY = 12     /* the text and the dense result do not fit in device memory */
};
typedef struct cyto_mtx_read_info {
    int64_t entries;              /* entry lines scattered (nnz) */
    int64_t duplicates;           /* integer field: entries that found a non-zero sum in their cell (for positive counts: entries
                                     minus distinct cells) */
    int64_t reason_kind, reason_line, reason_byte;      /* with CYTO_ERR_UNSUPPORTED, else 0 */
    double ms_read;               /* host file reads */
    double ms_upload;             /* what the upload added to them */
    double ms_kernels;            /* the zero fill, the kernels and the small copies between them */
    double ms_download;           /* the dense result, device to host */
} cyto_mtx_read_info;
int cyto_mtx_read(const char *path, int64_t data_offset, int64_t G, int64_t C, int64_t nnz, int field, int64_t *out, int64_t ldo,
                  int device_id, cyto_mtx_read_info *info);
/* The entry-line parser alone, on the host (a test hook): line i is text[offsets[i], offsets[i+1]), without its line end.  kinds[i]
 * 0 or CYTO_MTXR_ERR_* (BLANK ... NEGZERO), where[i] the offset within the line that a refusal names; rows[i], cols[i] 1-based and
 * values[i] the int64 value or the float64 bits (kind 0). */
int cyto_mtx_parse_entries(const char *text, int64_t n, const int64_t *offsets, int field, int64_t G, int64_t C, int8_t *kinds,
                           int64_t *where, int64_t *rows, int64_t *cols, int64_t *values);

/* ---- a table that stays in HBM between the stages (cytospace_amd.resident.DeviceFrame).  A VIEW is rows and columns
 * of a row-major device matrix: src_dev (G x C, leading dimension ld_src >= C, of src_dtype), rows (host, Gs positions in [0, G); NULL:
 * all G rows in order, Gs == G) and cols (host, Cs positions in [0, C); NULL: all C columns in order, Cs == C); repeats allowed in both.
 *
 * cyto_select: dst[i][j] = (dst type) src[rows[i]][cols[j]], device to device, into dst_dev (Gs x ld_dst, ld_dst >= Cs; the columns
 * Cs ... ld_dst-1 are not written; dst_dev must not overlap src_dev).  src_dtype: CYTO_DTYPE_I64, _F64 (cyto_table's two column
 * kinds), _U16, _F32; dst_dtype: _U8, _U16, _I64, _F32, _F64.  *inexact: the elements whose value does not survive the conversion
 * (numpy's round trip v.astype(dst).astype(src) == v: a fraction or a value out of range for an integer type, an integer beyond
 * float32's / float64's 24 / 53 bits, a float64 that is no float32 -- and any NaN, which equals nothing).  Where *inexact > 0 the
 * inexact elements of an integer destination are unspecified and the caller discards the result; a float32 / float64 destination
 * always holds the rounded values (a same-type select copies the bits, NaN included).  All offsets are 64-bit.
 * CYTO_ERR_BAD_ARG, before a device is touched: a position outside its range, a dtype outside the lists, ld < columns, a negative extent,
 * a NULL list with Gs != G / Cs != C, a null pointer with a non-zero extent.  Gs == 0 or Cs == 0: CYTO_OK, nothing launched.
 * stream: as above (NULL: the default stream); the call returns with dst_dev complete.
 *
 * cyto_value_range: one pass over the same view, what cytospace_amd.cytospace._counts_matrix looks at to choose its dtype: *lo / *hi
 * the least and the largest value (NaNs skipped; +inf / -inf for an empty view or one of NaNs only), for the integer sources also
 * exactly in *lo_i64 / *hi_i64 (may be NULL; INT64_MAX / INT64_MIN for an empty view); *non_integral finite values with a fraction,
 * *non_finite NaNs and infinities, *not_f32_exact values other than NaN that float32 does not hold.  Order-free: minima, maxima, counts.
 *
 * cyto_select_check: the predicate alone, on the host (a test hook; no device): ok[i] = values[i] (src_dtype) survives the conversion
 * to dst_dtype.  It is the function the kernel calls (csrc/select_exact.h). */
int cyto_select(int64_t G, int64_t C, const void *src_dev, int64_t ld_src, int src_dtype, const int64_t *rows, int64_t Gs,
                const int64_t *cols, int64_t Cs, void *dst_dev, int64_t ld_dst, int dst_dtype, int64_t *inexact, int device_id,
                void *stream);
int cyto_value_range(int64_t G, int64_t C, const void *src_dev, int64_t ld_src, int src_dtype, const int64_t *rows, int64_t Gs,
                     const int64_t *cols, int64_t Cs, double *lo, double *hi, int64_t *lo_i64, int64_t *hi_i64, int64_t *non_integral,
                     int64_t *non_finite, int64_t *not_f32_exact, int device_id, void *stream);
int cyto_select_check(const void *values, int src_dtype, int64_t n, int dst_dtype, int8_t *ok);

#ifdef __cplusplus
}
#endif
#endif /* CYTOHIP_H */
