/*
 * mtg_hip.h -- C ABI of libmtg_hip.so: batched PolynomialOptimization<N>::solveLinear()
 * for AMD MI355X (gfx950).  Eigen-free, torch-free: plain pointers and sizes.
 *
 * This is the drop-in boundary for the reference's linear-optimiser hot path.  The
 * reference exposes that path only as a header-only C++ class template, so "what the
 * reference's FFI would bind" is the set of member functions below; each entry point
 * cites the reference interface it replaces, with
 *   LINH = mav_trajectory_generation/include/mav_trajectory_generation/polynomial_optimization_linear.h
 *   LIN  = mav_trajectory_generation/include/mav_trajectory_generation/impl/polynomial_optimization_linear_impl.h
 *
 * Data conventions (all IEEE double):
 *   N  = coefficients per polynomial (even, 2..12; polynomial.h:44 kMaxN), h = N/2
 *   K  = segments, D = dimensions, B = independent trajectories in the batch
 *   fixed_mask[v] bit p set  <=>  derivative p is a fixed constraint at vertex v
 *       (a vertex keeps exactly h slots; LIN:206-221.  Constraints of order >= h are
 *        dropped by the reference, LIN:84-105 -- callers drop them before building masks)
 *   d_fixed : values of the fixed slots, ordered lexicographically by (vertex, derivative)
 *             = the reference's fixed_constraints_compact_ (LINH:288-295, LIN:238-246)
 *   d_free  : the free slots in the same order = free_constraints_compact_ (LINH:194-206)
 *   coeffs  : [B][K][D][N], increasing powers c0..c(N-1) (LINH:43-44, polynomial.h:34-35),
 *             i.e. segments_[k][dim].getCoefficients() of trajectory b (LIN:276-280)
 * Input layouts are described by element strides so that both
 *   AoS  times[B][K], d_fixed[B][D][n_fixed]   (what a host caller naturally holds) and
 *   SoA  times[K][B], d_fixed[D][n_fixed][B]   (fully coalesced on the device)
 * are accepted; mtg_layout_aos()/mtg_layout_soa() fill the stride block.
 *
 * Error convention: every function returns MTG_OK (0) or a negative mtg_status; nothing
 * aborts or throws (the reference CHECK-aborts; the C++ veneer maps codes back to that).
 */
#ifndef MTG_HIP_H_
#define MTG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTG_MAX_N 12

typedef enum mtg_status {
  MTG_OK = 0,
  MTG_ERR_INVALID_ARGUMENT = -1, /* LIN:60-65, :76, :289, :502-504 CHECKs                  */
  MTG_ERR_BAD_SEGMENT_TIME = -2, /* LIN:297 CHECK_GT(segment_time, 0)                      */
  MTG_ERR_SINGULAR = -3,         /* non-positive pivot in R_PP (rank-deficient problem)    */
  MTG_ERR_DEVICE = -4,           /* HIP runtime error; see mtg_last_error_string           */
  MTG_ERR_NO_DEVICE = -5,        /* no gfx950 device / HIP runtime unusable                */
  MTG_ERR_UNSUPPORTED = -6
} mtg_status;

typedef struct mtg_context mtg_context; /* (device, stream, scratch) -- one per host thread */
typedef struct mtg_plan mtg_plan;       /* a7 gather tables for one (N, K, D, d, masks)     */

/* Replaces the constructor + setupFromVertices() structure part: LINH:57, LIN:57-109 and
 * setupConstraintReorderingMatrix LIN:182-260 (pure indexing, done once per plan). */
typedef struct mtg_plan_desc {
  int32_t n_coeffs;               /* N                                                      */
  int32_t dimension;              /* D (LINH:57)                                            */
  int32_t n_segments;             /* K = vertices - 1 (LIN:72)                              */
  int32_t derivative_to_optimize; /* d in [0, N/2-1] (LIN:60-65)                            */
  const uint32_t* fixed_mask;     /* [K+1], see above                                       */
} mtg_plan_desc;

typedef struct mtg_plan_info {
  int32_t n_all;          /* getNumberAllConstraints()   LINH:218 = N*K                     */
  int32_t n_fixed;        /* getNumberFixedConstraints() LINH:219                           */
  int32_t n_free;         /* getNumberFreeConstraints()  LINH:220                           */
  int32_t kernel_variant; /* 0 generic (run-time K/masks), 1 static, 2 static dim-split only, 3 rolled */
  int64_t algorithmic_bytes_per_trajectory; /* 8*(K + D*n_fixed + K*D*N), SURVEY 8(d)       */
} mtg_plan_info;

typedef struct mtg_layout {
  int64_t times_stride_b, times_stride_k;               /* times[b*sb + k*sk]               */
  int64_t fixed_stride_b, fixed_stride_d, fixed_stride_c; /* d_fixed[b*sb + dim*sd + col*sc] */
  int64_t free_stride_b, free_stride_d, free_stride_c;    /* d_free likewise                 */
} mtg_layout;

enum {
  MTG_FLAG_HOST_POINTERS = 1u << 0, /* all buffers are host memory: the library stages them  */
  MTG_FLAG_GENERIC_KERNEL = 1u << 1, /* force the generic kernel (tests / A-B measurements)  */
  MTG_FLAG_FUSED_DIMS = 1u << 2,     /* all D dimensions in one workgroup (large batches)     */
  MTG_FLAG_SPLIT_DIMS = 1u << 3,     /* one dimension group per workgroup (small batches);    */
                                     /* default: chosen from the batch size                   */
  MTG_FLAG_COST_ONLY = 1u << 4,      /* only cost[] is produced (coeffs may be NULL): the     */
                                     /* objective evaluations of the time optimisers          */
                                     /* (polynomial_optimization_nonlinear_impl.h:313-359,    */
                                     /* :569-571) need J = computeCost(), not the segments    */
  MTG_FLAG_DIMLANE = 1u << 5,        /* force the dimension-in-lane launch form where the     */
                                     /* plan and the call are eligible (canonical SoA or AoS  */
                                     /* inputs -- mtg_layout_soa / mtg_layout_aos --, coeffs  */
                                     /* only); default: chosen from the batch size            */
  MTG_FLAG_HOST_BACKEND = 1u << 6,   /* with MTG_FLAG_HOST_POINTERS and batch <=               */
                                     /* MTG_HOST_BACKEND_MAX_BATCH: solve on the calling      */
                                     /* thread with the host build of the kernels' lane code  */
                                     /* (no launch, no PCIe): the single-trajectory calls of  */
                                     /* the reference's nlopt loops (polynomial_optimization_ */
                                     /* nonlinear_impl.h:569-571).  Ignored otherwise.        */
  MTG_FLAG_CONCURRENT_ITEMS = 1u << 7, /* mtg_multi_create: no merging -- every item runs as its */
                                     /* own best launch, spread over the context's side       */
                                     /* streams (longest chains first), forked from and       */
                                     /* joined back onto the context's stream                 */
  MTG_FLAG_QUERY_EXTRA_OUTPUTS = 1u << 9, /* mtg_plan_launch_form only: the form of a call that */
                                     /* also asks for the cost and / or d_free                */
  MTG_FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH = 1u << 8, /* mtg_solve_linear_sequence: never merge  */
                                     /* the queue into one persistent launch (latency of the  */
                                     /* single launches; A/B measurements)                    */
  MTG_FLAG_COOPERATIVE = 1u << 11,   /* force the row-cooperative launch form (16 lanes per   */
                                     /* trajectory-half: the LATENCY form for small launches  */
                                     /* of long chains) where the plan and the call are       */
                                     /* eligible (standard shapes, D = 3, coefficients only); */
                                     /* default: chosen from the batch size and chain length  */
  MTG_FLAG_REFINE = 1u << 12,        /* mtg_solve_linear / _status, device pointers: ONE step */
                                     /* of iterative refinement on the free derivatives --    */
                                     /* the residual -(R_PP d_P + R_PF d_F) formed in double- */
                                     /* double from the exact unit-time table (csrc/          */
                                     /* mtg_refine.hip), the correction solved and the        */
                                     /* coefficients recovered by the ordinary float64        */
                                     /* kernels.  For problems whose float64 solution is      */
                                     /* conditioning-limited (N = 12, d < N/2 - 1: every      */
                                     /* float64 evaluation, the reference's own included, is  */
                                     /* 1e-8 .. 2e-6 from the 50-digit solution) the result   */
                                     /* is good to ~1e-13.  An ACCURACY mode: five launches,  */
                                     /* the correction through the generic kernel -- measured */
                                     /* 10-25x a plain solve (N = 12 / K = 32 at 100k: 5.2 ms */
                                     /* against 0.5 ms); asynchronous.  Not with COST_ONLY /  */
                                     /* HOST_POINTERS / BASIC_SOLUTION.                       */
  MTG_FLAG_BASIC_SOLUTION = 1u << 10 /* mtg_solve_linear / _status: reference behaviour on     */
                                     /* RANK-DEFICIENT free systems (LIN:365-378: the rank-   */
                                     /* revealing SparseQR returns a basic solution and       */
                                     /* solveLinear() returns true).  Trajectories the sweep  */
                                     /* flags singular are solved on the host (column-pivoted */
                                     /* QR of the dense R_PP, Eigen's rank threshold, free    */
                                     /* variables beyond the rank zero) and their outputs     */
                                     /* replaced; the call then reports MTG_OK for them (bit 2 */
                                     /* stays set in trajectory_status: WHICH ones were basic).*/
                                     /* The call is SYNCHRONOUS and carries its OWN status     */
                                     /* word (host and device pointers alike): flags raised   */
                                     /* by earlier asynchronous launches stay in the context  */
                                     /* for the next mtg_context_sync.  Not with              */
                                     /* MTG_FLAG_COST_ONLY.  WHICH minimiser: a structurally  */
                                     /* deficient plan is solved through its shadow -- the    */
                                     /* LOWEST free slots (vertex, derivative < d) that       */
                                     /* complete the fixed ones pinned to zero -- i.e. ONE of */
                                     /* the minimisers: same cost and constraints as the      */
                                     /* reference's basic solution, differing from it by an   */
                                     /* element of the cost's null space (one polynomial of   */
                                     /* degree < d over the whole trajectory); which columns  */
                                     /* SparseQR drops depends on COLAMD's order.             */
                                     /* mtg_solve_linear_sequence* and mtg_multi_create accept */
                                     /* the flag and stay ASYNCHRONOUS: structurally deficient */
                                     /* plans run on their shadow (a regular plan of the      */
                                     /* queue / request like any other); there is no per-     */
                                     /* trajectory host fall-back there -- a trajectory whose */
                                     /* factorisation breaks down stays flagged in the        */
                                     /* context's status word.                                */
};
#define MTG_HOST_BACKEND_MAX_BATCH 64

/* ---- context ------------------------------------------------------------------------- */
/* stream: a hipStream_t (as void*) to enqueue on, or NULL for the library's own stream.   */
int mtg_context_create(int device, void* stream, mtg_context** out);
int mtg_context_destroy(mtg_context* ctx);
/* Waits for everything enqueued on the context; returns MTG_ERR_BAD_SEGMENT_TIME /
 * MTG_ERR_SINGULAR if any trajectory of a device-pointer solve since the last sync raised it
 * (also solves replayed from a captured hipGraph: the status word is read from the device on
 * every call).  Host-pointer calls report their status themselves.                        */
int mtg_context_sync(mtg_context* ctx);
const char* mtg_last_error_string(const mtg_context* ctx);
const char* mtg_status_string(int status);

/* ---- plan ---------------------------------------------------------------------------- */
int mtg_plan_create(mtg_context* ctx, const mtg_plan_desc* desc, mtg_plan** out);
int mtg_plan_destroy(mtg_plan* plan);
int mtg_plan_get_info(const mtg_plan* plan, mtg_plan_info* out);
/* The context a plan was created on (its stream, status word and error text): host objects that hold a plan and may be
 * used from another thread than their creator synchronise THIS context, not their own thread's.                     */
mtg_context* mtg_plan_context(const mtg_plan* plan);
/* (N, D, K, d) of the description the plan was created from (any out-pointer may be NULL).                                  */
int mtg_plan_get_shape(const mtg_plan* plan, int32_t* n_coeffs, int32_t* dimension, int32_t* n_segments, int32_t* derivative_to_optimize);
/* STRUCTURAL rank deficiency of the plan's free system R_PP (0: regular).  The cost's null space is the polynomials of degree
 * < derivative_to_optimize over the whole trajectory; what the fixed slots leave of it is a property of the constraint pattern,
 * not of a batch's values (under-constrained problems: fewer than d independent position / velocity / ... constraints in the
 * whole trajectory).  Every trajectory of such a plan is flagged MTG_ERR_SINGULAR (bit 1 of the per-trajectory status) by every
 * solve -- the reference's rank-revealing SparseQR returns a basic solution there (LIN:365-378): ask for it with
 * MTG_FLAG_BASIC_SOLUTION -- such a plan is then solved through its "shadow" (the same pattern with that many more slots
 * fixed to zero: a regular system, on the device like any other; free variables beyond the rank come back as exact zeros).
 * On regular plans the kernels flag a trajectory only when the factorisation breaks down (a non-positive or NaN pivot).
 * LIMITATION: the rank is computed at GENERIC vertex instants.  A Birkhoff-type pattern (a derivative fixed without the lower
 * ones) can be regular generically and singular at a batch's actual times -- e.g. d = 3, ends position-only, the middle vertex
 * velocity-only, EQUAL segment times: p(0), p'(T), p(2T) are dependent on the quadratics.  Such a plan reports 0 here, and a
 * trajectory with exactly those times is caught only by the breakdown guard (a pivot of round-off size and either sign), where
 * the reference's QR still returns a basic solution.  Hermite-type patterns (every fixed derivative with all lower ones: every
 * pattern of the reference's tests and generators) are not affected.                                                        */
int mtg_plan_rank_deficiency(const mtg_plan* plan);
/* The same number from the description alone (host arithmetic only: no context, no device): fixed_mask[n_segments + 1] as in
 * mtg_plan_desc.  Negative: mtg_status.                                                                                      */
int mtg_structural_rank_deficiency(int32_t n_coeffs, int32_t n_segments, int32_t derivative_to_optimize, const uint32_t* fixed_mask);
/* Which kernel form a device-pointer mtg_solve_linear(plan, batch, layout, ..., flags) call with coefficient output only
 * (with MTG_FLAG_QUERY_EXTRA_OUTPUTS: a call that also returns the cost / d_free) takes on this device: 0 generic (run-time K / masks), 1 fused static, 2 dimension-split static, 3 rolled (run-time K),
 * 4 fused with slab output (whole-sector stores), 5 dimension-in-lane (one unrolled body per chain length), 6 dimension-in-lane
 * with a run-time chain length (one body per polynomial order), 7 row-cooperative (16 lanes per trajectory-half; small
 * launches of long chains).  The answer is the launcher's own decision (one pure function, csrc/mtg_launch_plan.h, that
 * the solve call runs as well), not a restatement of it.  Negative: mtg_status.                                         */
int mtg_plan_launch_form(const mtg_plan* plan, int64_t batch, const mtg_layout* layout, uint32_t flags);
void mtg_layout_aos(const mtg_plan* plan, int64_t batch, mtg_layout* out);
void mtg_layout_soa(const mtg_plan* plan, int64_t batch, mtg_layout* out);
/* SoA with the row stride padded to the next multiple of 16 trajectories (times[K][Bs], d_fixed[D][n_fixed][Bs], d_free likewise;
 * Bs = (batch + 15) & ~15): every 16-trajectory row piece starts on a 128-byte boundary whatever the batch size -- with the plain
 * SoA stride a batch of 12 500 (100 000-byte rows) reads 1.75x its input bytes.  Read by the dimension-in-lane kernels like
 * the two canonical layouts (any other kernel takes it as the general strided layout it is).                              */
void mtg_layout_soa_padded(const mtg_plan* plan, int64_t batch, mtg_layout* out);

/* Optional: caller-owned scratch for the generic kernels' back-substitution workspace (no allocation inside
 * mtg_solve_linear then, e.g. for graph capture).  bytes == 0 restores library-managed scratch.               */
int mtg_plan_set_workspace(mtg_plan* plan, void* device_ptr, size_t bytes);

/* ---- device memory for host code that must not see HIP headers --------------------------
 * (the reference is host-only: its containers live in host memory, LINH:249-283.)  Allocation on
 * the context's device; the copies are ordered on the context's stream and return when done.  */
int mtg_device_malloc(mtg_context* ctx, size_t bytes, void** device_ptr);
int mtg_device_free(mtg_context* ctx, void* device_ptr);
int mtg_copy_to_device(mtg_context* ctx, void* dst_device, const void* src_host, size_t bytes);
int mtg_copy_to_host(mtg_context* ctx, void* dst_host, const void* src_device, size_t bytes);

/* ---- the hot path -------------------------------------------------------------------- */
/* Replaces updateSegmentTimes() + solveLinear() (LINH:101,108; LIN:286-305, :339-379,
 * incl. constructR :308-336 and updateSegmentsFromCompactConstraints :263-283) for `batch`
 * trajectories sharing one plan.  Asynchronous on the context's stream.
 *   times   in   segment times (> 0)
 *   d_fixed in   fixed constraint values
 *   coeffs  out  [batch][K][D][N]
 *   d_free  out  optional (NULL): optimised free constraints  (getFreeConstraints LINH:194)
 *   cost    out  optional (NULL): [batch], computeCost() LIN:124-140 = 0.5 * sum c^T Q c  */
int mtg_solve_linear(mtg_plan* plan, int64_t batch, const mtg_layout* layout,
                     const double* times, const double* d_fixed, double* coeffs,
                     double* d_free, double* cost, uint32_t flags);

/* mtg_solve_linear with a per-trajectory status output: trajectory_status[b] (int32, optional, NULL = none) receives
 * 0, or the OR of 1 (a segment time <= 0: LIN:297 CHECK_GT) and 2 (non-positive pivot: rank-deficient free system,
 * where the reference's rank-revealing SparseQR LIN:365-367 would still return a basic solution) for trajectory b --
 * the batch-wide codes MTG_ERR_BAD_SEGMENT_TIME / MTG_ERR_SINGULAR say THAT a trajectory failed, this says WHICH.
 * The library zero-fills it.  Device pointer, or host pointer with MTG_FLAG_HOST_POINTERS.
 * With MTG_FLAG_HOST_POINTERS every solve / update entry is synchronous and returns the batch status itself.     */
int mtg_solve_linear_status(mtg_plan* plan, int64_t batch, const mtg_layout* layout,
                            const double* times, const double* d_fixed, double* coeffs,
                            double* d_free, double* cost, int32_t* trajectory_status, uint32_t flags);

/* The basic solution of ONE trajectory's free system on the host (what MTG_FLAG_BASIC_SOLUTION applies to the flagged
 * trajectories of a batch; LIN:360-375 with a rank-revealing factorisation): times [K], d_fixed [D][n_fixed] ->
 * d_free [D][n_free] (host pointers); *rank (optional) receives the numerical rank of R_PP (n_free: regular system).
 * Coefficients follow from mtg_update_segments_from_free (LIN:263-283).                                          */
int mtg_basic_solution_host(const mtg_plan* plan, const double* times, const double* d_fixed, double* d_free, int32_t* rank);

/* A queue of n INDEPENDENT batches of the same plan (same batch size, layout and flags): solve i reads times[i] /
 * d_fixed[i] and writes coeffs[i] (host arrays of n DEVICE pointers; no batch may read what another one writes), enqueued
 * on the context's stream by ONE host call -- what a pipeline that streams batch after batch through the solver does (the
 * reference's counterpart is a loop over setupFromVertices + solveLinear, polynomial_timing_evaluation.cpp:104-110).
 * Because the batches are independent the library overlaps them: plans with a slab-output kernel (the standard shapes)
 * run the whole queue as ONE persistent launch whose workgroups walk the tiles of all batches, batch-major (the pointer
 * triples travel in the kernel arguments, up to 96 batches per launch): no drain / launch gap between batches, the store
 * tail of batch i under the elimination of batch i + 1.  Results are bit-identical to n mtg_solve_linear calls -- EXCEPT where a
 * single call of that batch size would take the row-cooperative form by default (mtg_plan_launch_form = 7: N = 12 / K >= 16,
 * N = 10 / K >= 64, N = 8 / K >= 80 in launches of at most one or two 4-trajectory workgroups per CU): that form eliminates in
 * another order, and the queue (and mtg_multi_*) agrees with it to round-off x conditioning, not bit for bit.  Other
 * plans, and calls with MTG_FLAG_SEQUENCE_ONE_LAUNCH_PER_BATCH, enqueue one launch per batch back to back.           */
int mtg_solve_linear_sequence(mtg_plan* plan, int32_t n, int64_t batch, const mtg_layout* layout,
                              const double* const* times, const double* const* d_fixed, double* const* coeffs,
                              uint32_t flags);
/* The same with two caller-owned hipEvent_t (either may be NULL) recorded on the context's stream immediately before the
 * first and after the last launch, inside the call: a caller that times the queue with events does not measure its own
 * latency between recording the start event and enqueueing the first launch (several microseconds from Python -- as
 * much as a kernel of this library).                                                                                  */
int mtg_solve_linear_sequence_events(mtg_plan* plan, int32_t n, int64_t batch, const mtg_layout* layout,
                                     const double* const* times, const double* const* d_fixed, double* const* coeffs,
                                     uint32_t flags, void* start_event, void* stop_event);

/* Replaces updateSegmentTimes() + setFreeConstraints() (LIN:500-508): coefficients from
 * caller-provided free constraints, no solve (the nonlinear optimiser's path,
 * polynomial_optimization_nonlinear_impl.h:695-696).  d_free is an INPUT here.            */
int mtg_update_segments_from_free(mtg_plan* plan, int64_t batch, const mtg_layout* layout,
                                  const double* times, const double* d_fixed,
                                  const double* d_free, double* coeffs, double* cost,
                                  uint32_t flags);

/* ---- the time optimisers' cost / gradient step ------------------------------------------------
 * Replaces, for a batch, PolynomialOptimizationNonLinear<N>::getCostAndGradientMellinger
 * (impl/polynomial_optimization_nonlinear_impl.h:287-364): per trajectory the reference runs K + 1 updateSegmentTimes +
 * solveLinear + computeCost -- the current times, and for each segment n the times with T_n += h and every other
 * T_i -= h / (K - 1) (h = increment_time, 0.1 in the reference), clamped from below to time_lower_bound
 * (kOptimizationTimeLowerBound = 0.1, polynomial_optimization_nonlinear.h:31) -- and returns J_d and the forward
 * differences (J_n - J_d) / h.  Here all (K + 1) * batch solves are ONE cost-only launch; the perturbed times are formed
 * in the kernel from `times` (nothing is materialised), a second small kernel forms the differences.
 *   cost     out optional [batch]: J_d
 *   gradient out [batch][K] with the strides of `times` in `layout` (gradient[b*times_stride_b + n*times_stride_k])
 * K == 1: zero gradient (impl:295-302).  Device pointers; asynchronous on the context's stream; flags raised by any of
 * the virtual problems surface at mtg_context_sync.                                                            */
int mtg_mellinger_cost_gradient(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                                const double* d_fixed, double increment_time, double time_lower_bound, double* cost,
                                double* gradient);

/* ---- next step after the path: batched sampling ---------------------------------------- */
/* Replaces, for a batch, Trajectory::evaluateRange (src/trajectory.cpp:81-141) / Polynomial::evaluate
 * (polynomial.h:137-149) as used by sampleTrajectoryInRange (src/trajectory_sampling.cpp:45-110):
 *   out[b][i][der][dim] = der-th derivative of dimension dim at t_i = t_start + i*dt,  i < n_samples,
 * der < n_derivatives (5 = position .. snap), from coeffs[batch][K][D][N] and times[b*stride_b + k*stride_k].
 * Samples beyond a trajectory's end are evaluated at its end; n_valid[b] (optional) = number of samples with
 * t_i <= total time.  Device pointers (out 16-byte aligned); asynchronous on the context's stream.
 * Rounding, so that a host caller can reproduce every choice the kernels make:
 *   t_i        the float64 value fl(t_start + fl(i * dt)): TWO roundings, never one fused multiply-add -- what a host loop that
 *              builds the timestamps as `t_start + i * dt` obtains; the sampler and n_valid use the same value;
 *   segment    the first k whose float64 prefix sum  acc_k = fl(acc_{k-1} + times[k])  (acc_{-1} = 0, sequential) exceeds t_i
 *              (a sample exactly on a vertex belongs to the segment on its right; none: the last segment);
 *   seg_start  acc_{k-1}: the prefix sum BEFORE the segment's own time is added (not acc_k - times[k]);
 *   local      min(fl(t_i - seg_start), times[k]); t_i < 0 extrapolates segment 0 with a negative local time;
 *   total time acc_{K-1}.                                                                                      */
int mtg_sample_range(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                     const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                     double t_start, double dt, int32_t n_samples, int32_t n_derivatives, double* out,
                     int32_t* n_valid);

/* ---- next step after the path: batched magnitude extrema and feasibility time scaling ---- */
/* Replaces, for a batch, Trajectory::computeMinMaxMagnitude (src/trajectory.cpp:190-227) over
 * Segment::computeMinMaxMagnitudeCandidates / selectMinMaxMagnitudeFromCandidates (src/segment.cpp:83-184):
 * extrema over [0, T_k] of  sqrt(sum_{dim in mask} (p_dim^(derivative)(t))^2)  for every segment.
 *   dimension_mask       bit d set = dimension d enters the magnitude (0 = all `dimension` of them); with exactly
 *                        one bit the candidates are the critical points of that polynomial (segment.cpp:124-131)
 *   segment_minmax   out [batch][K][4] = (t_min, v_min, t_max, v_max), times relative to the segment start
 *                        (Extremum::time, extremum.h:40-41); required, 16-byte aligned
 *   trajectory_minmax out optional [batch][4]: first segment with the strictly smallest / largest value
 *   trajectory_segment_idx out optional [batch][2] = (Extremum::segment_idx of the minimum, of the maximum)
 * The real roots of the magnitude derivative are isolated directly instead of running Jenkins-Traub
 * (src/rpoly/rpoly_ak1.cpp) -- same extrema values; extremum TIMES agree only where the root is well conditioned.
 * Needs n_coeffs - derivative - 1 >= 0 (polynomial.cpp:70-73).  Device pointers; asynchronous.               */
int mtg_minmax_magnitude(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                         const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                         int32_t derivative, uint32_t dimension_mask, double* segment_minmax,
                         double* trajectory_minmax, int32_t* trajectory_segment_idx);

/* Per-axis extrema: the SIGNED minimum and maximum of single axes.  Replaces, for a batch, Polynomial::computeMinMax(0, T,
 * q, &min, &max) -> selectMinMaxFromCandidates (src/polynomial.cpp:102-143) for every (trajectory, segment, axis) and
 * every order q = derivative_first .. derivative_first + n_derivatives - 1 (0 = position .. 4 = snap), with ONE root
 * search per axis: the derivative chain that isolates the roots of p^(derivative_first + 1) passes through the critical
 * points of every higher order.
 * The rule: the candidates of order q are 0, then T, then the real roots of p^(q+1) in [0, T] in ascending order; the
 * running pair starts at (0, DBL_MAX) / (0, -DBL_MAX); both comparisons are strict, so the first candidate wins a tie and a
 * constant derivative reports t = 0 twice.  Values are Polynomial::evaluate's Horner form.  The roots are isolated directly
 * instead of running Jenkins-Traub, as in mtg_minmax_magnitude: same values; extremum TIMES agree only where the root is
 * well conditioned.
 * One departure from the reference: if any candidate value of a (segment, axis, order) is NaN its row is (0, NaN, 0, NaN)
 * -- not the DBL_MAX / lowest sentinels, which a bounding-box caller would read as an empty box; in the per-trajectory
 * reduction a NaN row wins and the first such segment is reported.  No other row differs.
 *   n_coeffs 2..12, n_segments >= 1, dimension 1..8, batch >= 0; times[b * times_stride_b + k * times_stride_k] as in
 *   mtg_minmax_magnitude; derivative_first >= 0, n_derivatives >= 1, last order <= min(4, n_coeffs - 1)
 *   (polynomial.cpp:70-73)
 *   segment_minmax    out [batch][K][D][n_derivatives][4] = (t_min, v_min, t_max, v_max), times relative to the segment
 *                         start; required, 16-byte aligned on the device
 *   trajectory_minmax out optional [batch][D][n_derivatives][4]: per (axis, order) the first segment with the strictly
 *                         smallest / largest value, that segment's time and value
 *   trajectory_segment_idx out optional [batch][D][n_derivatives][2] = (segment of the minimum, of the maximum); read only
 *                         together with trajectory_minmax
 * Argument errors return MTG_ERR_INVALID_ARGUMENT with nothing enqueued; batch == 0 returns before anything is enqueued.
 * Device pointers; asynchronous on the context's stream; kernel launches only (capturable).                          */
int mtg_minmax_axes(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                    const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                    int32_t derivative_first, int32_t n_derivatives, double* segment_minmax,
                    double* trajectory_minmax, int32_t* trajectory_segment_idx);
/* The same on host pointers through the library's host build of the same lane code: synchronous, no context, no device. */
int mtg_minmax_axes_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                         const double* times, int64_t times_stride_b, int64_t times_stride_k,
                         int32_t derivative_first, int32_t n_derivatives, double* segment_minmax,
                         double* trajectory_minmax, int32_t* trajectory_segment_idx);

/* Replaces, for a batch, Trajectory::scaleSegmentTimesToMeetConstraints(v_max, a_max) (src/trajectory.cpp:385-429)
 * on top of computeMaxVelocityAndAcceleration (:343-361): `max_iterations` rounds of { maximum |velocity| and
 * |acceleration| over all dimensions; if either exceeds its bound by more than 1e-3 relative, stretch every
 * segment time by s = max(1, v_act/v_max, sqrt(a_act/a_max)) and rescale the coefficients by (1/s)^n }.
 * The reference allows up to 20 rounds but stretching by s meets both bounds exactly, so round 2 only verifies;
 * pass 2 for the reference's result, 1 to skip the verification.  In place on coeffs [batch][K][D][N] and times.
 *   workspace     [8 * batch * (K + 1)] doubles, 16-byte aligned; afterwards holds the last round's
 *                 per-segment tables [2][batch][K][4] and per-trajectory extrema [2][batch][4] (0 = velocity,
 *                 1 = acceleration), evaluated BEFORE that round's scaling
 *   scaling   out optional [batch]: total factor applied to the segment times
 *   within_range out optional [batch]: the reference's return value (1 = bounds met at the last check)       */
int mtg_scale_segment_times_to_meet_constraints(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments,
                                                int32_t dimension, int64_t batch, double* coeffs, double* times,
                                                int64_t times_stride_b, int64_t times_stride_k, double v_max,
                                                double a_max, int32_t max_iterations, double* workspace,
                                                double* scaling, int32_t* within_range);

/* ---- next step after the path: batched analytic input-feasibility check --------------------- */
/* Replaces, for a batch, FeasibilityAnalytic::checkInputFeasibility(const Segment&) and
 * FeasibilityBase::checkInputFeasibilityTrajectory (mav_trajectory_generation_ros/src/feasibility_analytic.cpp:42-233,
 * feasibility_base.cpp:97-107): which trajectories can the vehicle fly under up to six input limits.
 * A limit that is NaN is absent and its check is not computed; the others enter by magnitude (InputConstraints::
 * addConstraint stores |value|).  mtg_input_constraints_init: no limits, min_section_time_s 0.05, gravity 9.81;
 * ..._set_defaults: the reference's default limits (0.5 g, 1.5 g, 3.0, pi/2, pi/2, 2 pi).                       */
typedef struct mtg_input_constraints {
  double f_min, f_max;        /* thrust ||a + (0, 0, gravity)|| (mass-normalised, m/s^2)                         */
  double v_max;               /* ||velocity||                                                                    */
  double omega_xy_max;        /* roll/pitch rate: Mueller's bound sqrt(max jerk / min thrust) per section        */
  double omega_z_max;         /* |yaw rate| (dimension 3, D == 4 only)                                           */
  double omega_z_dot_max;     /* |yaw acceleration|                                                              */
  double min_section_time_s;  /* FeasibilityAnalytic::Settings: shortest section the roll/pitch split examines   */
  double gravity;             /* mav_msgs::kGravity upstream                                                     */
} mtg_input_constraints;
void mtg_input_constraints_init(mtg_input_constraints* constraints);
void mtg_input_constraints_set_defaults(mtg_input_constraints* constraints);

/* Result codes: the reference's enum InputFeasibilityResult (feasibility_base.h:34-50).  The analytic check never
 * returns MTG_INPUT_INFEASIBLE_ROLL_PITCH_RATES: a roll/pitch bound above the limit splits the section until it is
 * shorter than min_section_time_s, which is MTG_INPUT_INDETERMINABLE.                                            */
enum {
  MTG_INPUT_FEASIBLE = 0,
  MTG_INPUT_INDETERMINABLE = 1,
  MTG_INPUT_INFEASIBLE_THRUST_HIGH = 2,
  MTG_INPUT_INFEASIBLE_THRUST_LOW = 3,
  MTG_INPUT_INFEASIBLE_VELOCITY = 4,
  MTG_INPUT_INFEASIBLE_ROLL_PITCH_RATES = 5,
  MTG_INPUT_INFEASIBLE_YAW_RATES = 6,
  MTG_INPUT_INFEASIBLE_YAW_ACC = 7
};

/* Per segment, in this order, first hit decides: thrust (minimum below f_min before maximum above f_max), velocity,
 * yaw rate, yaw acceleration, roll/pitch sections; dimension other than 3 or 4: MTG_INPUT_INDETERMINABLE for every
 * segment.  Per trajectory: the result of the first segment (in segment order) that is not feasible.
 *   n_coeffs              5 .. 12 (the jerk polynomial must be at least linear; Polynomial::kMaxN = 12)
 *   times                 times[b * times_stride_b + k * times_stride_k]; strides >= 1, [B][K] or [K][B] without overlap
 *   trajectory_result out [batch]; required
 *   first_failing_segment out optional [batch]: index of that segment, -1 if none
 *   segment_result    out optional [batch][K]
 *   segment_bounds    out optional [batch][K][6], 16-byte aligned: thrust minimum, thrust maximum, velocity maximum,
 *                         roll/pitch bound of the whole segment, |yaw rate| maximum, |yaw acceleration| maximum; NaN
 *                         where the quantity's limit is absent (not computed)
 * The real roots of the magnitude derivatives are isolated directly instead of running Jenkins-Traub (as
 * mtg_minmax_magnitude): same extrema values; a verdict can differ from the reference's only where a bound lies
 * within rounding of its limit or a candidate's time within rounding of a section's end.
 * Device pointers; asynchronous on the context's stream.  Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued. */
int mtg_check_input_feasibility(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                const double* coeffs, const double* times, int64_t times_stride_b,
                                int64_t times_stride_k, const mtg_input_constraints* constraints,
                                int32_t* trajectory_result, int32_t* first_failing_segment, int32_t* segment_result,
                                double* segment_bounds);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device (the reference's one-trajectory-at-a-time callers).  segment_bounds needs no alignment here.          */
int mtg_check_input_feasibility_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                     const double* coeffs, const double* times, int64_t times_stride_b,
                                     int64_t times_stride_k, const mtg_input_constraints* constraints,
                                     int32_t* trajectory_result, int32_t* first_failing_segment,
                                     int32_t* segment_result, double* segment_bounds);

/* ---- the cheap, conservative input check: batched recursive input-feasibility check ----------
 * Replaces, for a batch, FeasibilityRecursive::checkInputFeasibility(const Segment&) with checkInputFeasibilityTrajectory
 * (mav_trajectory_generation_ros/src/feasibility_recursive.cpp:42-297): Mueller's recursive test on single-axis
 * extrema.  Per segment only the real roots of the acceleration, jerk and snap polynomials of x, y, z are needed
 * (degree N - 3, N - 4, N - 5) instead of the analytic check's three magnitude searches.  Everything not named here is
 * mtg_check_input_feasibility's: N in 5 .. 12, the times strides, the result codes, mtg_input_constraints (a NaN limit
 * is absent; min_section_time_s is FeasibilityRecursive::Settings', default 0.05), the argument errors, device pointers,
 * asynchronous on the context's stream: a caller swaps checkers by swapping the function name.
 * Per segment: the value FeasibilityRecursive::checkInputFeasibility(const Segment&) returns; per trajectory: the result
 * of the first segment (in segment order) that is not feasible; dimension other than 3 or 4: MTG_INPUT_INDETERMINABLE
 * everywhere.  Faithful to the reference, quirks included:
 *   - a section shorter than min_section_time_s is indeterminable before anything else is looked at: a whole segment
 *     with T < min_section_time_s is MTG_INPUT_INDETERMINABLE even with no limit set;
 *   - order inside a section [t1, t2]: (1) thrust at both ends, low before high; (2) velocity at both ends; (3) per-axis
 *     velocity extrema in axis order, a single axis above v_max fails at once; (4) per-axis thrust extrema, a single axis
 *     above f_max fails at once, a sign change gives a zero lower-bound term; (5) jerk extrema; (6) f_upper < f_min:
 *     thrust low; (7) f_lower > f_max: thrust high; (8) any bound beyond its limit: split at (t1 + t2) / 2, first half
 *     first, and return the first result that is not feasible;
 *   - a lower-bound thrust^2 <= 1e-6 makes the roll/pitch bound DBL_MAX;
 *   - all comparisons are strict;
 *   - MTG_INPUT_INFEASIBLE_ROLL_PITCH_RATES is never returned;
 *   - yaw rate, then yaw acceleration, are checked over the whole segment only after the recursion returned feasible,
 *     and only for dimension 4;
 *   - Polynomial::getRoots returning false does not occur: the real roots in [0, T] are isolated directly;
 *   - one guard of our own, as in the analytic check: depth 62 ends the walk as MTG_INPUT_INDETERMINABLE (with
 *     min_section_time_s = 0 the reference recurses without end).
 *   segment_bounds    out optional [batch][K][6], 16-byte aligned: the bounds of the whole-segment section [0, T] --
 *                         f_lower_bound, f_upper_bound, v_upper_bound, the roll/pitch bound -- then |yaw rate| maximum and
 *                         |yaw acceleration| maximum; NaN where the quantity's limit is absent (the thrust bounds are
 *                         computed when any of f_min, f_max, omega_xy_max is set).  A value is computed whenever its
 *                         limit is set, whatever the verdict and even where T < min_section_time_s: the reference
 *                         returns early here.
 *   segment_sections  out optional [batch][K]: the sections the walk examined, i.e. the calls of recursiveFeasibility
 *                         that got past the minimum-section-time test: 1 for a segment decided at the top, 0 if
 *                         T < min_section_time_s.  A measure of how hard a segment was.
 * A verdict can differ from the reference's only where a bound lies within rounding of its limit or a root's time
 * within rounding of a section's end.                                                                            */
int mtg_check_input_feasibility_recursive(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension,
                                          int64_t batch, const double* coeffs, const double* times,
                                          int64_t times_stride_b, int64_t times_stride_k,
                                          const mtg_input_constraints* constraints, int32_t* trajectory_result,
                                          int32_t* first_failing_segment, int32_t* segment_result, double* segment_bounds,
                                          int32_t* segment_sections);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device.  segment_bounds needs no alignment here.                                                             */
int mtg_check_input_feasibility_recursive_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                               const double* coeffs, const double* times, int64_t times_stride_b,
                                               int64_t times_stride_k, const mtg_input_constraints* constraints,
                                               int32_t* trajectory_result, int32_t* first_failing_segment,
                                               int32_t* segment_result, double* segment_bounds,
                                               int32_t* segment_sections);

/* ---- next to the input check: batched half-plane / flight-corridor feasibility check ------------
 * Replaces, for a batch, FeasibilityBase::checkHalfPlaneFeasibility(const Segment&) / (const Trajectory&) over
 * half_plane_constraints_ (mav_trajectory_generation_ros/src/feasibility_base.cpp:109-154) and the HalfPlane helpers
 * (:54-86): which trajectories stay strictly on the inner side of every plane of a set -- a room, a geofence, a
 * per-segment safe-flight corridor.
 * A plane is 4 doubles (nx, ny, nz, offset): UNIT normal pointing inwards, offset = point . normal.  The clearance of
 * a segment at local time t is  n . p(t) - offset  over dimensions 0-2 (a 4th, yaw, dimension is ignored); a plane
 * fails a segment iff the clearance is <= 0 at t = 0, t = T or a real root in [0, T] of the derivative of the projected
 * polynomial sum_dim n_dim p_dim (Polynomial::computeMinMaxCandidates), isolated directly as in mtg_minmax_magnitude.
 *   n_coeffs              1 .. 12 (odd counts and counts below 4 run zero-padded; N <= 2 has no interior candidates)
 *   n_segments            1 .. 2^22 - 1
 *   dimension             3 or 4; anything else: every trajectory infeasible at segment 0 with plane -1 and NaN
 *                         clearances (the reference returns false before it looks at a plane)
 *   times                 times[b * times_stride_b + k * times_stride_k]; strides >= 1, [B][K] or [K][B] without overlap;
 *                         T <= 0: no interior candidates, both ends are still evaluated
 *   planes                segment k of trajectory b uses the n_planes planes at planes + b * planes_stride_b +
 *                         k * planes_stride_k (strides in doubles, >= 0): (0, 0) one set for everything
 *                         (half_plane_constraints_), (0, 4 P) one cell per segment, (4 P K, 4 P) a corridor per trajectory
 *   n_planes              1 .. 64
 *   trajectory_feasible out [batch]; required: 1 / 0
 *   first_failing_segment out optional [batch]: first segment in segment order with a failing plane, -1 if none
 *   first_failing_plane   out optional [batch]: first plane in list order that fails that segment, -1 if none
 *   segment_clearance     out optional [batch][K]: minimum clearance over ALL planes and candidates (no early exit,
 *                         unlike the reference, which returns at the first failure)
 *   trajectory_clearance  out optional [batch]: minimum over the segments
 * Comparison and order are the reference's: `clearance <= 0` fails, so a NaN clearance does not fail (and does not
 * enter the minimum; nothing but NaN: +infinity).  A plane whose normal equals the previous plane's or its negation,
 * component by component (by value: +0 equals -0), reuses the previous plane's critical points: a bounding box costs
 * three root searches.  The clearance is evaluated on the projected polynomial (one Horner chain): it differs from the
 * reference's (p(t) - point) . n by rounding only, so a verdict can differ only where a clearance is within rounding of 0.
 * Device pointers (planes included: normals are not verified); asynchronous on the context's stream, three launches,
 * capturable.  Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued.                                        */
int mtg_check_half_plane_feasibility(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension,
                                     int64_t batch, const double* coeffs, const double* times, int64_t times_stride_b,
                                     int64_t times_stride_k, const double* planes, int32_t n_planes,
                                     int64_t planes_stride_b, int64_t planes_stride_k, int32_t* trajectory_feasible,
                                     int32_t* first_failing_segment, int32_t* first_failing_plane,
                                     double* segment_clearance, double* trajectory_clearance);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device.  Here the planes are readable: a normal with | |n|^2 - 1 | > 1e-9 is MTG_ERR_INVALID_ARGUMENT.          */
int mtg_check_half_plane_feasibility_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                          const double* coeffs, const double* times, int64_t times_stride_b,
                                          int64_t times_stride_k, const double* planes, int32_t n_planes,
                                          int64_t planes_stride_b, int64_t planes_stride_k,
                                          int32_t* trajectory_feasible, int32_t* first_failing_segment,
                                          int32_t* first_failing_plane, double* segment_clearance,
                                          double* trajectory_clearance);
/* HalfPlane(point, normal) for n planes (feasibility_base.cpp:54-59): points [n][3], normals [n][3] (any length > 0,
 * divided by their norm) -> out [n][4].  A zero or non-finite normal: MTG_ERR_INVALID_ARGUMENT.  Host pointers.       */
int mtg_half_planes_from_points_normals(int32_t n, const double* points, const double* normals, double* out);
/* HalfPlane::createBoundingBox(center, size) (:69-86) -> out [6][4], in its order and with its signs: per axis the
 * minimum face (center - size / 2) with normal +e, then the maximum face (center + size / 2) with -e.  Host pointers. */
int mtg_half_planes_bounding_box(const double* center, const double* size, double* out);

/* ---- next to the half-plane check: batched sphere-obstacle clearance check -----------------------
 * Replaces, for a batch and a set of spheres, the caller's loop of Trajectory::offsetTrajectory(-centre) followed by
 * computeMinMaxMagnitude(POSITION, {0, 1, 2}, &min, &max) per obstacle (src/segment.cpp:83-184): which trajectories
 * stay clear of every sphere, where the others hit first, and by how much each segment misses.
 * An obstacle is 4 doubles (cx, cy, cz, r).  The clearance of a segment at local time t is
 *   || p(t) - c || - r - inflation  over dimensions 0-2 (a 4th, yaw, dimension is never read); an obstacle fails a
 * segment iff !(clearance > 0) at t = 0, t = T or a real root in [0, T] of g = sum_dim (p_dim - c_dim) p_dim'
 * (Segment::computeMinMaxMagnitudeCandidates of the offset segment), isolated directly as in mtg_minmax_magnitude.
 * This is a safety check: a NaN clearance FAILS, and a NaN wins every minimum it enters (segment and trajectory).
 *   n_coeffs                 1 .. 12 (odd counts and counts below 4 run zero-padded in the next even instantiation)
 *   n_segments               1 .. 2^19 - 1
 *   dimension                3 or 4
 *   times                    times[b * times_stride_b + k * times_stride_k]; strides >= 1, [B][K] or [K][B] without
 *                            overlap; T <= 0: no interior candidates, both ends are still evaluated
 *   obstacles                trajectory b uses the n_obstacles spheres at obstacles + b * obstacles_stride_b (stride in
 *                            doubles, >= 0): 0 one shared set, 4 M a set per trajectory
 *   n_obstacles              1 .. 4096
 *   inflation                >= 0 and finite: the vehicle's radius, added to every sphere's
 *   trajectory_feasible      out [batch]; required: 1 / 0
 *   first_failing_segment    out optional [batch]: first segment in segment order with a failing obstacle, -1 if none
 *   first_failing_obstacle   out optional [batch]: smallest index among that segment's failing obstacles, -1 if none
 *   segment_clearance        out optional [batch][K]: minimum over ALL obstacles and candidates (no early exit)
 *   segment_nearest_obstacle out optional [batch][K]: the obstacle that attains it; a tie goes to the smallest index, a
 *                            NaN to the smallest index that produced one
 *   segment_closest_time     out optional [batch][K]: local time of that candidate (of one obstacle's candidates the
 *                            first in the order 0, T, roots ascending wins a tie).  As for the extremum times of
 *                            mtg_minmax_magnitude: the VALUE is second order in the root's error, the TIME is not --
 *                            where the distance is flat (a multiple root of g, a rest-to-rest segment's end) the time is
 *                            resolved to ~ eps^(1/m) T only
 *   trajectory_clearance     out optional [batch]: minimum over the segments
 * The convolution sum_dim p p' is formed once per segment; an obstacle is searched only if a lower bound of its
 * clearance over the segment's bounding boxes (less a rounding allowance) is not both > 0 and above the running minimum,
 * nearest bound first: no result depends on the pruning or on the order of the list beyond the index rules above.
 * Device pointers (radii are not verified); asynchronous on the context's stream, three launches, no workspace,
 * capturable.  Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued; batch == 0 returns before anything is.  */
int mtg_check_obstacle_clearance(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                 const double* coeffs, const double* times, int64_t times_stride_b,
                                 int64_t times_stride_k, const double* obstacles, int32_t n_obstacles,
                                 int64_t obstacles_stride_b, double inflation, int32_t* trajectory_feasible,
                                 int32_t* first_failing_segment, int32_t* first_failing_obstacle,
                                 double* segment_clearance, int32_t* segment_nearest_obstacle,
                                 double* segment_closest_time, double* trajectory_clearance);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device.  Here the obstacles are readable: a radius that is negative or not finite is MTG_ERR_INVALID_ARGUMENT.  */
int mtg_check_obstacle_clearance_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                      const double* coeffs, const double* times, int64_t times_stride_b,
                                      int64_t times_stride_k, const double* obstacles, int32_t n_obstacles,
                                      int64_t obstacles_stride_b, double inflation, int32_t* trajectory_feasible,
                                      int32_t* first_failing_segment, int32_t* first_failing_obstacle,
                                      double* segment_clearance, int32_t* segment_nearest_obstacle,
                                      double* segment_closest_time, double* trajectory_clearance);

/* ---- next to the sphere check: batched trajectory-to-trajectory separation check ------------------
 * Which pairs of solved trajectories keep a centre-to-centre distance above min_separation at every instant both fly,
 * where the others first come too close, and the exact minimum distance of each pair.  Replaces sampling both
 * trajectories and taking norms (which certifies nothing between samples), or a host loop over
 * Segment::computeMinMaxMagnitudeCandidates on difference segments the caller would have to build.
 * Side A is coeffs_a [batch_a][n_segments_a][dimension][n_coeffs] with its times and an optional global start time per
 * trajectory; side B likewise with its own batch and segment count.  The two sides may be the same buffers.
 *   Breakpoints  ea[0] = start_a (0 if start_a is null), ea[i + 1] = ea[i] + Ta[i]: one rounded float64 addition per
 *                step, in segment order; eb likewise.
 *   Pieces       all (i, j) with lo = max(ea[i], eb[j]) < hi = min(ea[i + 1], eb[j + 1]); along a pair they are ordered
 *                in time, i + j increases strictly, there are at most Ka + Kb - 1.  On a piece sa = lo - ea[i],
 *                sb = lo - eb[j], L = hi - lo and d(tau) = pA_i(sa + tau L) - pB_j(sb + tau L), tau in [0, 1].
 *   Candidates   tau = 0 and tau = 1 exactly, and the real roots in [0, 1] of g = sum_dim d_dim d_dim', isolated directly
 *                as in mtg_minmax_magnitude.  separation = || d(tau) || - min_separation over dimensions 0-2 (a 4th, yaw,
 *                dimension is never read); a piece fails iff a candidate has !(separation > 0).
 *   Fold         within a piece the candidates are taken in the order 0, 1, roots ascending with strict <, the first NaN
 *                wins; across the pieces of a pair the earliest piece wins a tie and a NaN wins every minimum it enters
 *                (the earliest one stays); the first failing piece is the earliest in time.  Times are global:
 *                lo + tau L.  This is a safety check: a NaN separation FAILS.
 *   No piece     (the two never fly at the same time, or touch at an instant only): the pair is feasible, its separation
 *                +inf, its times NaN, its segment indices -1, its piece counts 0.  A vehicle that has landed occupies
 *                nothing: a caller who wants it to keep its end point appends a constant segment.
 *   Invalid pair a segment time that is negative or not finite, or a start that is not finite, on either side; or a pair
 *                index outside [0, batch_a) x [0, batch_b), for which nothing of either side is read: the pair is
 *                infeasible, its separations and times NaN, its segment indices -1, its piece counts 0.
 *   n_coeffs                  1 .. 12 (odd counts and counts below 4 run zero-padded in the next even instantiation)
 *   dimension                 3 or 4, shared by both sides
 *   n_segments_a, _b          1 .. 1024 each
 *   batch_a, batch_b          >= 0
 *   times_a                   times_a[b * times_a_stride_b + k * times_a_stride_k]; strides >= 1, [B][K] or [K][B]
 *                             without overlap; a segment of time 0 makes no piece.  times_b likewise
 *   start_a, start_b          optional [batch]: the global time at which each trajectory starts; null: 0
 *   n_pairs                   >= 0, n_pairs * n_segments_a < 2^31
 *   pairs                     [n_pairs][2] int32: (index into A, index into B)
 *   min_separation            >= 0 and finite: the required centre-to-centre distance (the sum of both radii)
 *   pair_feasible             out [n_pairs]; required: 1 / 0
 *   first_failing_segment_a   out optional [n_pairs]: segment of A of the earliest failing piece, -1 if none
 *   first_failing_segment_b   out optional [n_pairs]: segment of B of that piece, -1 if none
 *   pair_separation           out optional [n_pairs]: minimum over all pieces and candidates (no early exit)
 *   pair_closest_time         out optional [n_pairs]: global time of the candidate that attains it
 *   pair_closest_segment_a    out optional [n_pairs]: segment of A of that piece
 *   pair_closest_segment_b    out optional [n_pairs]: segment of B of that piece
 *   segment_separation        out optional [n_pairs][Ka]: minimum over the pieces of segment i of A; +inf without a piece
 *   segment_closest_time      out optional [n_pairs][Ka]: global time of that candidate; NaN without a piece.  As for
 *                             the extremum times of mtg_minmax_magnitude the VALUE is second order in the root's error,
 *                             the TIME is not
 *   segment_closest_segment_b out optional [n_pairs][Ka]: segment of B of that piece; -1 without a piece
 *   segment_pieces            out optional [n_pairs][Ka]: pieces of segment i of A (pruned or not)
 * Any of the three pair_closest outputs needs segment_separation, segment_closest_time and segment_closest_segment_b:
 * they are found by a scan of those.  A piece is searched only if a lower bound of its separation from the hulls of the
 * two sides' Bernstein control points on the piece (less a rounding allowance) is not both > 0 and above the running
 * minimum of its segment of A: no result depends on the pruning.
 * Device pointers (the pair indices are verified per pair, see above); asynchronous on the context's stream, three
 * launches, no workspace, capturable.  Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued; n_pairs == 0 returns
 * before anything is.  The arguments are checked before the context is looked at (a null context is refused after
 * them), so the argument rules can be exercised in a process without a device.  */
int mtg_check_trajectory_separation(mtg_context* ctx, int32_t n_coeffs, int32_t dimension, int32_t n_segments_a, int64_t batch_a,
                                    const double* coeffs_a, const double* times_a, int64_t times_a_stride_b,
                                    int64_t times_a_stride_k, const double* start_a, int32_t n_segments_b, int64_t batch_b,
                                    const double* coeffs_b, const double* times_b, int64_t times_b_stride_b,
                                    int64_t times_b_stride_k, const double* start_b, int64_t n_pairs, const int32_t* pairs,
                                    double min_separation, int32_t* pair_feasible, int32_t* first_failing_segment_a,
                                    int32_t* first_failing_segment_b, double* pair_separation, double* pair_closest_time,
                                    int32_t* pair_closest_segment_a, int32_t* pair_closest_segment_b,
                                    double* segment_separation, double* segment_closest_time,
                                    int32_t* segment_closest_segment_b, int32_t* segment_pieces);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device.  Here the pair list is readable: an index outside its side's batch is MTG_ERR_INVALID_ARGUMENT.  */
int mtg_check_trajectory_separation_host(int32_t n_coeffs, int32_t dimension, int32_t n_segments_a, int64_t batch_a,
                                         const double* coeffs_a, const double* times_a, int64_t times_a_stride_b,
                                         int64_t times_a_stride_k, const double* start_a, int32_t n_segments_b, int64_t batch_b,
                                         const double* coeffs_b, const double* times_b, int64_t times_b_stride_b,
                                         int64_t times_b_stride_k, const double* start_b, int64_t n_pairs, const int32_t* pairs,
                                         double min_separation, int32_t* pair_feasible, int32_t* first_failing_segment_a,
                                         int32_t* first_failing_segment_b, double* pair_separation, double* pair_closest_time,
                                         int32_t* pair_closest_segment_a, int32_t* pair_closest_segment_b,
                                         double* segment_separation, double* segment_closest_time,
                                         int32_t* segment_closest_segment_b, int32_t* segment_pieces);

/* ---- next to the sphere check: batched keep-out zone check (convex obstacles: boxes, prisms) ------
 * The complement of mtg_check_half_plane_feasibility: which trajectories stay OUTSIDE every zone of a set, where the
 * others enter first, and by how much each segment misses.  Replaces wrapping each box in a sphere, or a host loop.
 * A zone is n_planes planes of 4 doubles (nx, ny, nz, offset) in the half-plane check's convention: unit normal pointing
 * INTO the zone, offset = point . normal; the zone is where every n_j . x - offset_j > 0, so the six planes of
 * mtg_half_planes_bounding_box are a box zone as they stand (mtg_keep_out_boxes).  For a segment at local time t, over
 * dimensions 0-2 (a 4th, yaw, dimension is never read):
 *   h_j(t) = offset_j - n_j . p(t)   (> 0: outside plane j),   c(t) = max_j h_j(t) - inflation,
 *   clearance = min over t in [0, T] of c(t);   a zone fails a segment iff !(clearance > 0).
 * clearance > 0 is a LOWER bound of the Euclidean distance to the zone with its planes pushed out by `inflation` (exact
 * where the nearest point lies in a face, up to sqrt(3) low at a box corner); clearance < 0 is minus the exact penetration
 * depth (the distance to the nearest face).  Pushing the planes out is a superset of the Minkowski sum with a ball.
 * Candidates: t = 0, t = T, the real roots in [0, T] of every h_j' and of every h_i - h_j (i < j), isolated directly as
 * in mtg_minmax_magnitude; each is evaluated as max_j h_j(t).  Planes with equal or negated normals (compared by value)
 * share their h' roots and pairs with equal normals are not searched: a box costs at most 3 + 15 searches (a
 * plane that is nowhere the maximum over the segment's bounding boxes is neither searched nor paired), and a zone may be
 * padded to n_planes by repeating a plane without changing any result.
 * This is a safety check: a NaN clearance FAILS, and a NaN wins every minimum it enters (segment and trajectory).
 *   n_coeffs                 1 .. 12 (odd counts and counts below 4 run zero-padded in the next even instantiation)
 *   n_segments               1 .. 2^19 - 1
 *   dimension                3 or 4
 *   times                    times[b * times_stride_b + k * times_stride_k]; strides >= 1, [B][K] or [K][B] without
 *                            overlap; T <= 0: no interior candidates, both ends are still evaluated
 *   zones                    trajectory b uses the n_zones zones at zones + b * zones_stride_b (stride in doubles, >= 0):
 *                            0 one shared set, 4 P M a set per trajectory; zone m's planes are at + 4 P m
 *   n_zones                  1 .. 4096
 *   n_planes                 1 .. 8, the same for every zone of a call
 *   inflation                >= 0 and finite: the vehicle's radius, every plane is pushed out by it
 *   trajectory_feasible      out [batch]; required: 1 / 0
 *   first_failing_segment    out optional [batch]: first segment in segment order with a failing zone, -1 if none
 *   first_failing_zone       out optional [batch]: smallest index among that segment's failing zones, -1 if none
 *   segment_clearance        out optional [batch][K]: minimum over ALL zones and candidates (no early exit)
 *   segment_nearest_zone     out optional [batch][K]: the zone that attains it; a tie goes to the smallest index, a NaN
 *                            to the smallest index that produced one
 *   segment_closest_time     out optional [batch][K]: local time of that candidate (of one zone's candidates the first in
 *                            the order 0, T, roots in search order wins a tie)
 *   trajectory_clearance     out optional [batch]: minimum over the segments
 * A zone is searched only if a lower bound of its clearance over the segment's four bounding boxes (less a rounding
 * allowance) is not both > 0 and above the running minimum, nearest bound first: no result depends on the pruning or on
 * the order of the list beyond the index rules above.
 * Device pointers (the planes are not verified); asynchronous on the context's stream, three launches, no workspace,
 * capturable.  Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued; batch == 0 returns before anything is.  */
int mtg_check_keep_out_zones(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                             const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                             const double* zones, int32_t n_zones, int32_t n_planes, int64_t zones_stride_b,
                             double inflation, int32_t* trajectory_feasible, int32_t* first_failing_segment,
                             int32_t* first_failing_zone, double* segment_clearance, int32_t* segment_nearest_zone,
                             double* segment_closest_time, double* trajectory_clearance);
/* The same check with HOST pointers on the library's host build of the same code, synchronous; needs no context and
 * no device.  Here the zones are readable: a normal with | |n|^2 - 1 | > 1e-9 or an offset that is not finite is
 * MTG_ERR_INVALID_ARGUMENT.  */
int mtg_check_keep_out_zones_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                  const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                  const double* zones, int32_t n_zones, int32_t n_planes, int64_t zones_stride_b,
                                  double inflation, int32_t* trajectory_feasible, int32_t* first_failing_segment,
                                  int32_t* first_failing_zone, double* segment_clearance, int32_t* segment_nearest_zone,
                                  double* segment_closest_time, double* trajectory_clearance);
/* n boxes (centers [n][3], sizes [n][3]) as zones: out [n][6][4], mtg_half_planes_bounding_box per box in that function's
 * own plane order and signs.  A size that is not positive or not finite is MTG_ERR_INVALID_ARGUMENT.  Host pointers. */
int mtg_keep_out_boxes(int32_t n, const double* centers, const double* sizes, double* out);

/* ---- next to the keep-out check: batched distance-field (ESDF voxel grid) clearance check ---------
 * For planners whose map is a voxel grid of distances (a Euclidean signed distance field, an inflated occupancy map), not a
 * list of shapes: which trajectories of a batch are collision-free in the map, where the others fail first, and by how much
 * each segment misses.  Replaces mtg_sample_range followed by index arithmetic, a gather and a reduction by the caller.
 * This is a SAMPLED check: between two samples nothing is certified.  The caller chooses dt against the vehicle's speed
 * and the map's resolution (a sample spacing of v_max dt well below voxel_size, and an inflation that covers the rest).
 * Everything below is float64 unless said otherwise, and every rule is fixed so that a host loop reproduces each choice.
 *   samples      of a segment with time T: local times t_0 = 0, then t_i = fl(i dt) for every i >= 1 with fl(i dt) < T
 *                (strict), then T itself as the last sample: S >= 2 of them, T never twice; T <= 0 or NaN: 0 and T.
 *                Sample index S - 1 means local time T, any other index i means fl(i dt).  S is found without walking
 *                (T / dt against max_samples as doubles, then one correction by the rule's own test).  If
 *                S > max_samples the segment is NOT sampled: segment_samples -1, segment_clearance NaN, both sample
 *                indices -1, and the segment fails.  That cap bounds the run time of a call.
 *   position     Polynomial::evaluate's Horner form (one fused multiply-add per coefficient) over dimensions 0-2; a 4th
 *                (yaw) dimension is never read
 *   voxel coord  u_a = fl(fl(p_a - origin_a) r),  r = fl(1 / voxel_size), a = x, y, z
 *   trilinear    inside iff 0 <= u_a <= n_a - 1 on every axis (closed); cell i_a = min((int)floor(u_a), n_a - 2) (a sample
 *                exactly on the last centre uses f = 1), f_a = fl(u_a - i_a); the eight floats are converted to double
 *                and combined along x, then y, then z, each step as fma(f, hi - lo, lo).  Needs n_a >= 2.
 *   nearest      i_a = (int)floor(fl(u_a + 0.5)); inside iff 0 <= i_a <= n_a - 1.  Needs n_a >= 1.
 *   outside      a sample outside the grid takes outside_distance; a NaN u_a gives a NaN; non-finite voxels follow from
 *                the arithmetic above
 *   clearance    of a sample: fl(d - inflation); the sample fails iff !(clearance > 0).  A NaN FAILS and wins every minimum
 *                it enters (segment and trajectory), as in the sphere and zone checks.  There is no early exit.           */
enum { MTG_FIELD_NEAREST = 0, MTG_FIELD_TRILINEAR = 1 };
typedef struct mtg_distance_field {
  const float* distances;      /* [nz][ny][nx], x fastest; device pointer (host pointer in the host form) */
  int32_t nx, ny, nz;          /* each >= 2 (trilinear) or >= 1 (nearest); nx ny nz <= 2^31 - 1 */
  double  origin[3];           /* position of the CENTRE of voxel (0,0,0); finite */
  double  voxel_size;          /* h > 0, finite, 1 / h finite */
  double  outside_distance;    /* value of a sample outside the grid; any double but NaN (0: unknown is an obstacle, +inf: free) */
  int32_t interpolation;       /* MTG_FIELD_NEAREST 0, MTG_FIELD_TRILINEAR 1 */
} mtg_distance_field;
void mtg_distance_field_init(mtg_distance_field* field);   /* zeroes; trilinear; outside_distance 0 */
/*   n_coeffs                 1 .. 12 (odd counts and counts below 4 run zero-padded in the next even instantiation)
 *   n_segments               1 .. 2^19 - 1
 *   dimension                3 or 4
 *   times                    times[b * times_stride_b + k * times_stride_k]; strides >= 1, [B][K] or [K][B] without overlap
 *   field                    read by the entry on the HOST; only field->distances is a device pointer
 *   dt                       > 0 and finite
 *   max_samples              2 .. 2^20: the largest S a segment may have
 *   inflation                >= 0 and finite: the vehicle's radius
 *   trajectory_feasible          out [batch]; required: 1 / 0
 *   first_failing_segment        out optional [batch]: first failing segment in segment order, -1 if none
 *   segment_clearance            out optional [batch][K]: minimum over all S samples
 *   segment_closest_sample       out optional [batch][K]: smallest sample index that attains it; with a NaN the smallest
 *                                index that produced one
 *   segment_first_failing_sample out optional [batch][K]: smallest failing index, -1 if none
 *   segment_samples              out optional [batch][K]: S, or -1 (not sampled)
 *   trajectory_clearance         out optional [batch]: minimum over the segments
 * Device pointers; asynchronous on the context's stream, three launches (init, segment kernel, per-trajectory decode), no
 * workspace, capturable.  Argument errors (null required pointers, n_a out of range or more than 2^31 - 1 voxels, voxel_size,
 * origin or inflation not finite or out of range, NaN outside_distance, unknown interpolation, bad dt or max_samples, a bad
 * shape): MTG_ERR_INVALID_ARGUMENT, nothing enqueued; batch == 0 returns before anything is.  */
int mtg_check_distance_field(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                             const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                             const mtg_distance_field* field, double dt, int32_t max_samples, double inflation,
                             int32_t* trajectory_feasible, int32_t* first_failing_segment, double* segment_clearance,
                             int32_t* segment_closest_sample, int32_t* segment_first_failing_sample,
                             int32_t* segment_samples, double* trajectory_clearance);
/* The same check with HOST pointers (field->distances too) on the library's host build of the same code, synchronous; needs
 * no context and no device.  */
int mtg_check_distance_field_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                  const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                  const mtg_distance_field* field, double dt, int32_t max_samples, double inflation,
                                  int32_t* trajectory_feasible, int32_t* first_failing_segment, double* segment_clearance,
                                  int32_t* segment_closest_sample, int32_t* segment_first_failing_sample,
                                  int32_t* segment_samples, double* trajectory_clearance);

/* ---- next to the sampled check: CERTIFIED distance-field check -----------------------------------
 * A verdict for every instant of every segment, and a guaranteed lower bound of the minimum clearance next to the sampled
 * upper bound: an adaptive interval bisection in which a node is one sample plus a Lipschitz bound of the field over the
 * Taylor reach of the position around the sample.  Takes what mtg_check_distance_field takes except dt and max_samples, and
 *   lipschitz L   the caller's promise: finite, > 0, and |D(x) - D(y)| <= L ||x - y|| for the trilinear interpolant D and all
 *                 x, y inside the grid.  mtg_distance_field_lipschitz_host computes a rigorous one.  Trilinear fields only.
 *   min_depth     0 .. 10, max_depth  min_depth .. 24, max_frontier  max(2, 2^min_depth) .. 1024
 * Every step is fixed so that a host loop reproduces each choice; s = 2^-36, r = fl(1 / voxel_size), and every operation
 * written below rounds once (no contraction) unless it is an fma.  A segment runs in the even instantiation NC of the sampled
 * check (N zero-padded to 4, 6, .. 12); N below is that NC.
 *   nodes      a segment with time T > 0 is covered by a binary tree; node (d, j), 0 <= j < 2^d, has half-width
 *              w = T 2^-(d+1) (an exact scaling) and midpoint m = fl((2 j + 1) w).  The tree starts with all 2^min_depth nodes
 *              of depth min_depth.  !(T > 0): ONE node with w = 0 and m = 0 (NaN T: m = T); it is terminal whatever its bound,
 *              and segment_depth is 0.
 *   per node   1. shift: q_a = the coefficients of axis a; for i = 0 .. N-2: for j = N-2 down to i: q[j] = fma(m, q[j+1], q[j]).
 *                 Then q_a,0 = p_a(m) -- the sampled check's Horner value bit for bit -- and q_a,k = p_a^(k)(m) / k!.
 *              2. reach: t = |q_a,N-1|; for k = N-2 .. 1: t = fma(t, w, |q_a,k|); R_a = t w  >= max_{|e| <= w} |p_a(m+e) - p_a(m)|
 *                 (the Taylor bound: exact in real arithmetic, first-order tight for small w).
 *              3. scale: A_a = horner over |c_a,N-1| .. |c_a,0| in |m| with one fma per coefficient, + |origin_a|.
 *              4. Rh_a = fma(s, A_a, R_a (1 + s)),  Rh = sqrt(fma(Rh_z, Rh_z, fma(Rh_y, Rh_y, Rh_x Rh_x))) (1 + s).
 *              5. sample: c = lookup(p(m)) - inflation with the sampled check's lookup (outside rule, NaN); fails iff !(c > 0).
 *              6. box: u_a by the sampled check's rule, rho_a = (Rh_a r) (1 + s).  INSIDE iff 0 <= u_a - rho_a and
 *                 u_a + rho_a <= n_a - 1 on every axis; TOUCHES iff u_a + rho_a >= 0 and u_a - rho_a <= n_a - 1 on every axis.
 *                 A NaN among the u_a - rho_a and u_a + rho_a (a NaN position, an infinite reach): the bound is NaN.
 *              7. bound_in: touches: Dc - inflation - L Rh - s (|Dc| + inflation + 2 L / r), left to right, Dc = the lookup
 *                 at u clamped to [0, n_a - 1] per axis (the projection onto the convex grid is non-expansive: the clamped
 *                 point certifies every point of the box that lies inside the grid); else +infinity.
 *              8. bound_out: inside: +infinity; else outside_distance - inflation.
 *              9. bound = min(bound_in, bound_out); a NaN wins.
 *             10. fate: the sample fails: terminal, evidence of a collision; else bound > 0: terminal, certified; else
 *                 d == max_depth (or the lone node): terminal, undecided; else replaced by its two children.
 *   levels     breadth-first, a frontier in ascending j.  After a level, if the next frontier would hold more than
 *              max_frontier nodes the segment stops with MTG_FIELD_UNDECIDED_BUDGET and its lower bound is -infinity.  The
 *              budget and the depth limit bound a call's run time; there is no early exit.
 *   segment    segment_result: 0 some evaluated sample failed (a definite point of the trajectory), 1 every terminal node is
 *              certified, 2 / 3 undecided; 0 wins over 2 and 3, 3 over 2.  segment_lower_bound: min of bound over the terminal
 *              nodes, a guaranteed lower bound of min_t D(p(t)) - inflation whatever the verdict; a NaN wins.
 *              segment_sampled_clearance: min of c over all evaluated nodes (an upper bound of the true minimum; a NaN wins),
 *              segment_closest_time the m of that node, ties to the smaller m.  segment_first_failing_time: the smallest m of
 *              a failing sample, NaN if none.  segment_nodes: evaluated nodes; segment_depth: the deepest level evaluated.
 *   trajectory trajectory_result: the code of the first segment, in segment order, that is not FREE, else 1;
 *              first_failing_segment: that segment, -1 if none; the two bounds: minima over the segments.  A
 *              trajectory_sampled_clearance <= 0 or NaN means that a definite collision exists somewhere.
 * All outputs are minima, sums or maxima over a node set fixed by the rule: they do not depend on how nodes are spread over
 * lanes, and the device and host forms agree bit for bit.  DESIGN.md 4.15 has the soundness argument.                      */
enum { MTG_FIELD_COLLIDES = 0, MTG_FIELD_FREE = 1, MTG_FIELD_UNDECIDED_DEPTH = 2, MTG_FIELD_UNDECIDED_BUDGET = 3 };
/* Device pointers; trajectory_result [batch] is required, every other output optional: first_failing_segment [batch] int32,
 * segment_result / segment_nodes / segment_depth [batch][K] int32, segment_lower_bound / segment_sampled_clearance /
 * segment_closest_time / segment_first_failing_time [batch][K], trajectory_lower_bound / trajectory_sampled_clearance [batch].
 * Asynchronous on the context's stream, three launches (init, segment kernel: one 64-lane workgroup per segment, decode), no
 * workspace, capturable.  Argument errors (those of the sampled check; a nearest field; lipschitz not finite and positive;
 * the three ranges above): MTG_ERR_INVALID_ARGUMENT, nothing enqueued; batch == 0 returns before anything is.  */
int mtg_certify_distance_field(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                               const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                               const mtg_distance_field* field, double lipschitz, int32_t min_depth, int32_t max_depth,
                               int32_t max_frontier, double inflation, int32_t* trajectory_result,
                               int32_t* first_failing_segment, int32_t* segment_result, double* segment_lower_bound,
                               double* segment_sampled_clearance, double* segment_closest_time,
                               double* segment_first_failing_time, int32_t* segment_nodes, int32_t* segment_depth,
                               double* trajectory_lower_bound, double* trajectory_sampled_clearance);
/* The same check with HOST pointers (field->distances too) on the library's host build of the same code, synchronous; needs
 * no context and no device.  */
int mtg_certify_distance_field_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                                    const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                    const mtg_distance_field* field, double lipschitz, int32_t min_depth, int32_t max_depth,
                                    int32_t max_frontier, double inflation, int32_t* trajectory_result,
                                    int32_t* first_failing_segment, int32_t* segment_result, double* segment_lower_bound,
                                    double* segment_sampled_clearance, double* segment_closest_time,
                                    double* segment_first_failing_time, int32_t* segment_nodes, int32_t* segment_depth,
                                    double* trajectory_lower_bound, double* trajectory_sampled_clearance);
/* A rigorous Lipschitz constant of the trilinear interpolant of a grid in HOST memory: per cell the largest absolute
 * difference over its four x-edges, four y-edges and four z-edges, gx, gy, gz; out = max over the cells of
 * sqrt(gx^2 + gy^2 + gz^2) / voxel_size, rounded up (times 1 + 2^-50).  Inside a cell dD/dx is a convex combination of the four
 * x-edge differences over h, and the grid is convex, so the bound holds globally.  A non-finite voxel makes it non-finite
 * (which the check refuses).  Reads distances, nx, ny, nz (each >= 2) and voxel_size only.  */
int mtg_distance_field_lipschitz_host(const mtg_distance_field* field, double* out);

/* ---- next to the distance-field checks: collision COST and its gradient ---------------------------
 * The map term of the CHOMP / continuous-time replanning objective  J_collision = sum over the segments of
 * int c(d(p(t)) - inflation) ||v(t)|| dt,  as a trapezoid sum on the sample grid of mtg_check_distance_field, and the exact
 * derivative of that sum with respect to every polynomial coefficient (same layout as coeffs).  Shape, times, field, dt,
 * max_samples and inflation are those of mtg_check_distance_field; the field must be TRILINEAR (a nearest-voxel field has a zero
 * gradient almost everywhere).  epsilon > 0, finite: the clearance at which the cost vanishes.  speed_epsilon >= 0, finite: the
 * smoothing of the speed, which makes the gradient well defined where the vehicle rests.
 * Every rounding is fixed so that a host loop reproduces each choice; fl() rounds once, every fma is fused, nothing else is:
 *   samples    the field check's: t_0 = 0, t_i = fl(i dt) for i >= 1 with fl(i dt) < T, then T; S of them.  S > max_samples: the
 *              segment is not sampled: segment_cost NaN, its gradient entries NaN, segment_samples -1.
 *   weights    w_0 = fl(fl(t_1 - t_0) 0.5),  w_i = fl(fl(t_{i+1} - t_{i-1}) 0.5),  w_{S-1} = fl(fl(t_{S-1} - t_{S-2}) 0.5).
 *              T <= 0: every weight is 0 (cost 0, gradient 0, S = 2).  T NaN: the weights, the cost and the gradient are NaN.
 *   p, v       dimensions 0-2, one pass per axis from the highest coefficient down, both from 0:
 *              v = fma(v, t, p); p = fma(p, t, c_j).  A 4th (yaw) dimension is never read; its N gradient entries are 0 in every
 *              segment (also one that is not sampled or has a NaN time).
 *   d          the field check's u_a and trilinear lookup, operation for operation
 *   G          the field's gradient from the lookup's own eight voxels, f_a, x00 .. x11, y0, y1 and r, inside the grid only.  With
 *              lerp_a(lo, hi) = fma(f_a, fl(hi - lo), lo) and e00, e10, e01, e11 the four (hi - lo) x-differences:
 *              G_x = fl(r lerp_z(lerp_y(e00, e10), lerp_y(e01, e11))),  G_y = fl(r lerp_z(fl(x10 - x00), fl(x11 - x01))),
 *              G_z = fl(r fl(y1 - y0)).  Outside: d = outside_distance, G = 0.  A NaN u_a: d and G are NaN.
 *   potential  x = fl(d - inflation).  x < 0: c = fl(fl(epsilon 0.5) - x), c' = -1.  0 <= x <= epsilon: q = fl(x - epsilon),
 *              c = fl(fl(q q) / fl(2 epsilon)), c' = fl(q / epsilon).  x > epsilon: c = c' = 0, and the sample is SKIPPED: it adds
 *              nothing to any sum, whatever its speed and G are.  x NaN: c = c' = NaN.  (The CHOMP potential: c, c' continuous.)
 *   speed      s = sqrt(fma(v_z, v_z, fma(v_y, v_y, fma(v_x, v_x, fl(speed_epsilon^2)))))
 *   cost       a sample's term is fl(fl(w c) s); a segment's cost is the sum of its terms
 *   gradient   the exact derivative of that sum,  d/dc_{a,j} = sum_i [ (w c' s G_a) t^j + (w c / s v_a) j t^(j-1) ]:
 *              k1 = fl(fl(w c') s), A_a = fl(k1 G_a);  k2 = fl(fl(w c) / s), 0 if s == 0, B_a = fl(k2 v_a);
 *              q_0 = 1, q_j = fl(q_{j-1} t);  entry (a, j): acc = fma(A_a, q_j, acc), then for j >= 1
 *              acc = fma(B_a, fl(j q_{j-1}), acc)
 *   sums       every segment sum is 64 partial sums from +0: partial g takes samples g, g + 64, .. in ascending order; they are
 *              joined by the butterfly P[l] = fl(P[l] + P[l xor off]) for off = 32, 16, 8, 4, 2, 1.  The host form does the same.
 *   trajectory trajectory_cost = the sum of segment_cost over the segments in ascending order, from +0, formed by a second kernel
 *              from the written segment_cost (hence required).  No floating-point atomics anywhere.
 * Non-finite voxels and outside_distance = +-infinity follow from this arithmetic.
 *   segment_cost     out [batch][K]; required
 *   trajectory_cost  out optional [batch]
 *   coeff_gradient   out optional [batch][K][D][N], the layout of coeffs; without it a kernel without the gradient's registers runs
 *                    and gives the same costs bit for bit
 *   segment_samples  out optional [batch][K]: S, or -1 (not sampled)
 * Device pointers; asynchronous on the context's stream, one launch (two with trajectory_cost), one wavefront per segment, no
 * workspace, no allocation, no synchronisation, capturable.  The arguments are checked before the context (the argument rules
 * need no device).  Argument errors (those of mtg_check_distance_field; a nearest field; epsilon not positive and finite;
 * speed_epsilon negative or not finite; a null segment_cost): MTG_ERR_INVALID_ARGUMENT, nothing enqueued; batch == 0 returns
 * before anything is.  Not provided: the derivative with respect to the segment times (the sample set changes with T).  */
int mtg_collision_cost(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                       const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                       const mtg_distance_field* field, double dt, int32_t max_samples, double inflation, double epsilon,
                       double speed_epsilon, double* segment_cost, double* trajectory_cost, double* coeff_gradient,
                       int32_t* segment_samples);
/* The same with HOST pointers (field->distances too) on the library's host build of the same code, synchronous; needs no
 * context and no device.  */
int mtg_collision_cost_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                            const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                            const mtg_distance_field* field, double dt, int32_t max_samples, double inflation, double epsilon,
                            double speed_epsilon, double* segment_cost, double* trajectory_cost, double* coeff_gradient,
                            int32_t* segment_samples);

/* ---- gradient with respect to the free derivatives: the transpose of mtg_update_segments_from_free ----
 * What an optimiser moves are the free derivatives d_free; the coefficients are a linear image of them,
 * c = A(T)^-1 M [d_F; d_P].  This call applies the exact transpose of that map to a coefficient-space gradient
 * G [batch][K][D][N] (the layout of coeffs; e.g. mtg_collision_cost's coeff_gradient) and, with coeffs given, adds the
 * derivative cost's gradient w Q(T) c (the cost mtg_solve_linear reports is 0.5 sum c^T Q(T) c, LIN:124-140) on the fly.
 * The reference has no such gradient (polynomial_optimization_nonlinear.h:215-243: gradient-free methods only).
 * Forward map per segment (time T) and dimension, h = N/2, x_S / x_E the derivative values at the segment's start / end
 * vertex, ai = rows h .. N-1 of A(1)^-1:   c_p = x_S,p / p!  (p < h),   c_(h+j) = T^-(h+j) sum_k ai[j][k] dl_k,
 * dl = [T^p x_S,p ; T^p x_E,p].  Every rounding is fixed so that a host loop reproduces each bit; fl() rounds once, every fma
 * is fused, nothing else is (contraction off); nothing depends on the launch geometry, and the device and host forms agree bit
 * for bit:
 *   powers     tp_0 = 1, tp_m = fl(tp_(m-1) T);  ti = fl(1 / T), tn_1 = ti, tn_m = fl(tn_(m-1) ti): repeated multiplication
 *              from T and ONE division
 *   input      G_i = grad_coeffs entry i of the row of (segment, dimension), +0 without grad_coeffs.  With coeffs, for
 *              i >= d = derivative_to_optimize:  y_j = fl(c_j tp_(j-d)) (j >= d),  S_i = the sum over j = d .. N-1 in
 *              ascending order, one fma(Q1[i][j], y_j, S) per term from +0 (Q1 = Q(1), the library's table),
 *              q_i = fl(tp_(i-d+1) S_i)  [(Q(T) c)_i = T^(1-2d) T^i sum_j Q1_ij c_j T^j with the powers joined: no division],
 *              G_i = fma(w, q_i, G_i).  Rows i < d of Q are zero: G_i stays as it is, whatever w is.
 *   u          u_j = fl(tn_(h+j) G_(h+j)),  j < h
 *   z          z_k = the sum over j = 0 .. h-1 in ascending order, one fma(ai[j][k], u_j, z) per term from +0
 *   halves     start vertex: g_S,p = fma(tp_p, z_p, fl(G_p rf_p)), rf_p = fl(1 / p!);  end vertex: g_E,p = fl(tp_p z_(h+p))
 *   vertex     0 < v < K: fl(g_E,p of segment v - 1  +  g_S,p of segment v): the left segment's end first, ONE rounded
 *              addition;  v = 0: g_S,p of segment 0;  v = K: g_E,p of segment K - 1
 *   routing    fixed_mask[v] bit p set: grad_fixed, the column of (v, p) in the order of d_fixed; else grad_free, the column
 *              of (v, p) in the order of d_free.  Every output element is written exactly once.
 * Times are NOT validated: T <= 0 or a NaN T gives what this arithmetic gives (ti = fl(1 / T) is infinite or NaN); no status
 * word is raised, other trajectories are unaffected.
 *   grad_coeffs        in  [batch][K][D][N] or NULL (treated as +0)
 *   coeffs             in  [batch][K][D][N] or NULL: no derivative-cost term, smoothness_weight is ignored
 *   grad_free          out layout's free strides (grad_free[b*free_stride_b + dim*free_stride_d + col*free_stride_c]); NULL: not wanted
 *   grad_fixed         out optional, layout's fixed strides
 * At least one of grad_coeffs / coeffs and at least one of grad_free / grad_fixed must be given (with n_free == 0 grad_free
 * may be NULL and is never written).  The map is linear and needs no factorisation: structurally rank-deficient plans are
 * accepted like any other, no shadow plan is involved.
 * Device pointers; asynchronous on the context's stream, ONE launch (one lane per trajectory, vertex and dimension), no
 * workspace, no allocation, no floating-point atomics, capturable.  The arguments are checked before the context is used.
 * Argument errors (a null plan, layout or times; a negative batch; both inputs or both outputs null; more than 2^31 - 1
 * lanes): MTG_ERR_INVALID_ARGUMENT, nothing enqueued.  */
int mtg_free_gradient(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                      const double* grad_coeffs, const double* coeffs, double smoothness_weight,
                      double* grad_free, double* grad_fixed);
/* The same with HOST pointers on the library's host build of the same code, synchronous; needs no context and no device:
 * the masks and columns are derived from desc (the rules of mtg_plan_create: N even in 2 .. 12, D, K >= 1, d < N/2).  */
int mtg_free_gradient_host(const mtg_plan_desc* desc, int64_t batch, const mtg_layout* layout, const double* times,
                           const double* grad_coeffs, const double* coeffs, double smoothness_weight,
                           double* grad_free, double* grad_fixed);

/* ---- the time optimisers' objective with soft constraints ---------------------------------------
 * Replaces, for a batch, the callbacks PolynomialOptimizationNonLinear<N> hands to nlopt
 * (impl/polynomial_optimization_nonlinear_impl.h, NL below): objectiveFunctionTime (NL:556-615) and
 * objectiveFunctionTimeAndConstraints (NL:660-742) = cost_trajectory + cost_time + cost_soft, with
 *   cost_trajectory = computeCost() after updateSegmentTimes + solveLinear (or + setFreeConstraints),
 *   cost_time       = time_penalty * T^2 (the squared-time kinds) or time_penalty * T (the Richter kinds), T = sum of the
 *                     segment times in segment order,
 *   cost_soft       = sum over the constraints, in their order, of
 *                     min(maximum_cost, exp(soft_constraint_weight * (max ||p^(derivative)|| / value - 1)))
 *                     (evaluateMaximumMagnitudeAsSoftConstraint NL:767-795 over computeMaximumOfMagnitude LIN:466-497).
 * Accepted derivatives: 1 .. N/2 - 1 -- continuous across vertices, so that the reference's candidate set (segment starts,
 * interior critical points, the end of the last segment) holds the true maximum; its own N - derivative - 1 > 0 check is
 * implied.  Values must be > 0.  dimension <= 4 (a lane keeps a segment's D x N coefficients in registers).
 * Non-finite coefficients (mtg_time_objective, mtg_magnitude_soft_cost and its host form alike): a NaN or Inf among the
 * coefficients that a constrained derivative reads -- indices >= derivative of any segment and dimension -- makes that
 * trajectory's maximum NaN and its violation NaN for that constraint, and its soft term maximum_cost (so does a magnitude
 * that overflows from finite coefficients).  No other trajectory and no other constraint is affected.                   */
#define MTG_MAX_MAGNITUDE_CONSTRAINTS 4
enum { /* NonlinearOptimizationParameters::TimeAllocMethod */
  MTG_TIME_SQUARED = 0,
  MTG_TIME_RICHTER = 1,
  MTG_TIME_MELLINGER_OUTER_LOOP = 2, /* (no time or soft term upstream: not accepted here) */
  MTG_TIME_SQUARED_AND_CONSTRAINTS = 3,
  MTG_TIME_RICHTER_AND_CONSTRAINTS = 4
};
typedef struct mtg_time_objective_params {
  int32_t time_cost_kind;         /* MTG_TIME_*; decides T^2 against T only                                          */
  int32_t use_soft_constraints;   /* 0: cost_soft = 0 (maxima are still written when asked for)                      */
  double time_penalty;            /* 500                                                                             */
  double soft_constraint_weight;  /* 100                                                                             */
  double maximum_cost;            /* 1e12: cap of each soft term                                                     */
  int32_t n_constraints;          /* 0 .. MTG_MAX_MAGNITUDE_CONSTRAINTS, in the order of addMaximumMagnitudeConstraint */
  int32_t derivative[MTG_MAX_MAGNITUDE_CONSTRAINTS];
  double value[MTG_MAX_MAGNITUDE_CONSTRAINTS];
} mtg_time_objective_params;
/* NonlinearOptimizationParameters' defaults (kSquaredTimeAndConstraints, 500, soft constraints on, 100, 1e12), no constraints */
void mtg_time_objective_params_init(mtg_time_objective_params* params);

/* d_free_in == NULL: objectiveFunctionTime -- the plan's ordinary solve (coefficients + cost) into `coeffs`;
 * d_free_in != NULL: objectiveFunctionTimeAndConstraints -- mtg_update_segments_from_free on the caller's free constraints.
 * Then ONE search launch (a lane per (trajectory, segment) reads its coefficients once and searches every constrained
 * derivative, maxima only) and a lane per trajectory that forms the components.
 *   coeffs     out [batch][K][D][N], 16-byte aligned; required
 *   objective  out [batch]; required.  +inf for a trajectory the solve flags (segment time <= 0, breakdown); the context's
 *                  flag is raised as for any solve (mtg_context_sync)
 *   components out optional [batch][3] = (cost_trajectory, cost_time, cost_soft)
 *   maxima     out optional [batch][n_constraints]; NaN by the non-finite rule above
 *   violations out optional [batch][n_constraints] = maximum - value (evaluateMaximumMagnitudeConstraint NL:745-763)
 * Device pointers; asynchronous on the context's stream.  The plan keeps 48 bytes of workspace per trajectory, grown by
 * the first call of a batch size (like mtg_mellinger_cost_gradient's): capture a call after one plain call of that size.
 * Argument errors: MTG_ERR_INVALID_ARGUMENT, nothing enqueued.                                                          */
int mtg_time_objective(mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times, const double* d_fixed,
                       const double* d_free_in, const mtg_time_objective_params* params, double* coeffs, double* objective,
                       double* components, double* maxima, double* violations);
/* The maxima + soft-cost stage alone on existing coefficients [batch][K][D][N] (getTotalCostWithSoftConstraints' third term):
 *   cost_soft out [batch]; required.  maxima required too here ([batch][n_constraints]: the search reduces into it);
 *   violations optional.  times[b * times_stride_b + k * times_stride_k] as in mtg_minmax_magnitude.
 *   Non-finite coefficients: the rule above (maximum and violation NaN, soft term maximum_cost, that trajectory only).   */
int mtg_magnitude_soft_cost(mtg_context* ctx, int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch,
                            const double* coeffs, const double* times, int64_t times_stride_b, int64_t times_stride_k,
                            const mtg_time_objective_params* params, double* cost_soft, double* maxima, double* violations);
/* The same with HOST pointers on the library's host build of the same lane code, synchronous; needs no context and no device.
 * maxima is optional here.                                                                                              */
int mtg_magnitude_soft_cost_host(int32_t n_coeffs, int32_t n_segments, int32_t dimension, int64_t batch, const double* coeffs,
                                 const double* times, int64_t times_stride_b, int64_t times_stride_k,
                                 const mtg_time_objective_params* params, double* cost_soft, double* maxima,
                                 double* violations);

/* cost_time alone, on the host: cost_time[b] = time_penalty * T^2 or * T (by params->time_cost_kind), T = the sum of
 * times[b * times_stride_b + k * times_stride_k] in segment order -- the expression the device entry evaluates.         */
int mtg_time_cost_host(const mtg_time_objective_params* params, int32_t n_segments, int64_t batch, const double* times,
                       int64_t times_stride_b, int64_t times_stride_k, double* cost_time);

/* ---- mixed requests: several plans in one launch ------------------------------------------
 * What a caller of the reference does with a list of independent PolynomialOptimization<N>
 * problems of different structure (BASELINE config 4: N in {8, 10, 12}, 4..32 segments): each
 * structure is a plan + a batch.  A mixed request is created once -- items with canonical SoA
 * (times[K][B], d_fixed[D][n_fixed][B]) or AoS inputs and coefficient output only whose plan has a
 * static dimension-in-lane configuration (the config-4 shapes: N = 8 / 10 / 12, K = 4 / 8 / 16 /
 * 32, D = 3) join ONE cross-structure launch whatever their N and K; of the others, items that
 * share D, the start / interior / end constraint pattern and the derivative (any K >= 2; N = 8 /
 * 10 / 12 standard shapes also across N) are merged into ONE launch of the run-time-K kernels
 * whose tiles are ordered longest-chain-first -- and solved as often as wanted
 * with new values in the same device buffers (same structure, new segment times: every
 * iteration of a time optimiser).  mtg_multi_solve only enqueues kernels (and memsets of the
 * cost outputs) on the context's stream: it can be stream-captured into a hipGraph.
 * Items that cannot be merged run as ordinary mtg_solve_linear launches.
 * Device pointers only; all plans must belong to `ctx`.                                       */
typedef struct mtg_multi mtg_multi;
typedef struct mtg_multi_item {
  mtg_plan* plan;
  int64_t batch;
  mtg_layout layout;
  const double* times;     /* device */
  const double* d_fixed;   /* device */
  double* coeffs;          /* device, 16-byte aligned, [batch][K][D][N] */
  double* d_free;          /* device, optional */
  double* cost;            /* device, optional */
} mtg_multi_item;
/* flags: 0, or MTG_FLAG_FUSED_DIMS / MTG_FLAG_SPLIT_DIMS to fix the launch geometry of the merged groups (a caller
 * that runs several mixed requests concurrently knows the total load; the default looks at this request only);
 * or MTG_FLAG_CONCURRENT_ITEMS: one launch per item through the ordinary variant choice (static / dimension-in-lane
 * kernels where the plan has them), the items overlapping on the device on up to 4 internal streams.               */
int mtg_multi_create(mtg_context* ctx, int32_t n_items, const mtg_multi_item* items, uint32_t flags, mtg_multi** out);
int mtg_multi_solve(mtg_multi* multi);              /* asynchronous on the context's stream */
int mtg_multi_launch_count(const mtg_multi* multi); /* kernel launches one mtg_multi_solve enqueues */
int mtg_multi_destroy(mtg_multi* multi);

/* ---- synthetic inputs and result check on the device (no tensor library needed) -------------
 * mtg_generate_waypoints: fills `times` / `d_fixed` (device pointers, any layout) of `batch` trajectories of the plan's
 * structure with the reference's random-waypoint recipe (src/vertex.cpp:27-82 createRandomVertices: positions uniform in
 * [-box, box]^D, consecutive vertices more than 0.2 apart, start / goal at rest; :255-272 estimateSegmentTimesNfabian with
 * the default magic constant 6.5); other fixed derivatives of interior vertices: random direction, magnitude <= v_max /
 * a_max / 1.  yaw_dimension != 0 with D = 4: the last dimension is an angle in [-3 pi, 3 pi].  Counter-based random
 * numbers: reproducible per (seed, trajectory), distribution-equivalent (not bit-equal) to the mt19937 original.
 * Asynchronous on the context's stream.
 * mtg_compare_coefficients: max over polynomials of ||a - b||_inf / ||b||_inf (the parity tests' norm-wise measure) and the
 * max absolute difference of two device buffers of n_polynomials x n_coeffs doubles; synchronous.                      */
int mtg_generate_waypoints(mtg_plan* plan, int64_t batch, const mtg_layout* layout, uint64_t seed, double box, double v_max,
                           double a_max, int32_t yaw_dimension, double* times, double* d_fixed);
int mtg_compare_coefficients(mtg_context* ctx, const double* a, const double* b, int64_t n_polynomials, int32_t n_coeffs,
                             double* max_normwise_rel, double* max_abs);

/* ---- several GPUs from one host process -----------------------------------------------------
 * The path shards by independent trajectories (LIN:339-379 touches only one optimiser's state): shard s of G is the
 * contiguous range mtg_shard_range(batch, G, s), solved on device s by that device's own context / plan / stream, with
 * no communication during the solve.  A device group = one context + one plan of the same description per device.
 * mtg_device_group_solve_linear fans one call out (asynchronous: the shards run concurrently); the caller holds the
 * per-device buffers (times[s], d_fixed[s], coeffs[s]: device pointers on device s, shard-local SoA (soa != 0) or AoS).
 * mtg_device_group_gather_coeffs is the optional final gather into one [batch][K][D][N] buffer: host memory (root < 0)
 * or memory of device `root` (peer copies over xGMI).  `devices` = NULL: devices 0 .. n-1.  The multi-process form
 * (one rank per GPU, RCCL all_gather over xGMI) is mav_trajectory_generation_amd/dist.py; both split the batch alike. */
typedef struct mtg_device_group mtg_device_group;
void mtg_shard_range(int64_t batch, int32_t n_shards, int32_t shard, int64_t* lo, int64_t* hi);
int mtg_device_group_create(int32_t n_devices, const int32_t* devices, const mtg_plan_desc* desc, mtg_device_group** out);
int mtg_device_group_destroy(mtg_device_group* group);
int mtg_device_group_size(const mtg_device_group* group);
mtg_context* mtg_device_group_context(mtg_device_group* group, int32_t shard);
mtg_plan* mtg_device_group_plan(mtg_device_group* group, int32_t shard);
int mtg_device_group_solve_linear(mtg_device_group* group, int64_t batch, int32_t soa, const double* const* times,
                                  const double* const* d_fixed, double* const* coeffs, uint32_t flags);
int mtg_device_group_sync(mtg_device_group* group);
int mtg_device_group_gather_coeffs(mtg_device_group* group, int64_t batch, const double* const* coeffs, int32_t root,
                                   double* dst);

/* ---- one PROCESS per GPU: the final gather over RCCL / xGMI (csrc/mtg_comm.hip) ----------------------------------------
 * north_star: batches shard across the GPUs of a node "with RCCL over xGMI only for the final gather".  Rank r of `world`
 * processes owns the slice mtg_shard_range(B, world, r), solves it with its own context / plan (no communication), and -- when
 * one consumer needs every shard on every device -- gathers the coefficient shards through a communicator:
 *   rank 0: mtg_comm_unique_id(id); ships the MTG_COMM_UNIQUE_ID_BYTES bytes to the other ranks (file, socket, MPI ...);
 *   every rank: mtg_comm_create(ctx, rank, world, id, &comm)   -- collective (ncclCommInitRank on the context's device);
 *   mtg_comm_all_gather(comm, local, n, gathered)              -- gathered[r][n] <- rank r's local[n] (equal n on every rank);
 *   mtg_comm_solve_all_gather(...)                             -- the batch in n_chunks pieces, chunk i's gather (on the
 *       communicator's own stream) under chunk i + 1's solve (on the context's stream): at 240 MB per rank the gather takes
 *       ~10x the solve (7 xGMI links x ~153 GB/s per GPU), so the solve hides behind it, not the other way round.
 *       gathered is chunk-major: [n_chunks][world][batch / n_chunks][K][D][N]; batch equal on every rank, a multiple of n_chunks.
 * Everything is asynchronous (ordered after the context's stream, which in turn waits for the last gather); mtg_comm_sync waits
 * for both streams and reports the context's status.  librccl.so is opened on first use (dlopen) -- a single-GPU consumer neither
 * links nor loads it; MTG_ERR_UNSUPPORTED where it is absent.  No RCCL types cross the boundary.                              */
typedef struct mtg_comm mtg_comm;
#define MTG_COMM_UNIQUE_ID_BYTES 128
int mtg_comm_unique_id(void* out_id /* MTG_COMM_UNIQUE_ID_BYTES bytes */);
int mtg_comm_create(mtg_context* ctx, int32_t rank, int32_t world, const void* unique_id, mtg_comm** out);
int mtg_comm_destroy(mtg_comm* comm);
int mtg_comm_rank(const mtg_comm* comm);
int mtg_comm_world(const mtg_comm* comm);
const char* mtg_comm_last_error(const mtg_comm* comm);
int mtg_comm_all_gather(mtg_comm* comm, const double* local, int64_t n_doubles, double* gathered);
int mtg_comm_solve_all_gather(mtg_comm* comm, mtg_plan* plan, int64_t batch, const mtg_layout* layout, const double* times,
                              const double* d_fixed, double* local_coeffs, double* gathered, int32_t n_chunks, uint32_t flags);
int mtg_comm_sync(mtg_comm* comm);

/* ---- measurement hooks (bench.py / tests) --------------------------------------------- */
/* Re-runs the last mtg_solve_linear launch of this plan `iters` times back-to-back on the
 * context's stream, bracketed by hipEvents recorded on that same stream; returns the mean
 * kernel-side duration per launch in microseconds.  (Queue launches of mtg_solve_linear_sequence
 * are not recorded: MTG_ERR_INVALID_ARGUMENT after one -- time those with the _events form.)   */
int mtg_time_last_solve(mtg_plan* plan, int iters, double* mean_us);
/* Accuracy self-test of the device reciprocal used by the LDL^T pivots: max relative error
 * of rcp(x) vs 1/x over n pseudo-random positive doubles.  (n < 0: diagnostic -- |n| samples with
 * (|n| & 3) Newton steps instead of the shipped two.)                                      */
int mtg_selftest_rcp(mtg_context* ctx, int n, double* max_rel_err);

#ifdef __cplusplus
}
#endif
#endif /* MTG_HIP_H_ */
