/*
 * lbfgsb_hip.h -- C ABI of the MI355X-native L-BFGS-B inner iteration.
 *
 * This is the drop-in boundary for the hot path of jacobwilliams/lbfgsb: the
 * n-dimensional work inside `mainlb` (reference src/lbfgsb.f90:312-949) runs as
 * hand-written HIP kernels on gfx950; the 2m x 2m algebra (bmv, formt, dpofa,
 * dtrsl, dcsrch) runs on the host inside this library.  The reverse-
 * communication protocol, the `task` strings and the documented isave/dsave/
 * lsave slots are the reference's (src/lbfgsb.f90:88-244).
 *
 * Plain C: pointers and sizes only, no torch/HIP types in the signatures
 * (a hipStream_t travels as void*).  There is NO CPU fallback: every entry
 * point that computes fails with LBFGSB_E_NOGPU when no gfx950 device is
 * usable.
 *
 * The Fortran module `lbfgsb_module` in lbfgsb_amd/fortran/ binds these with
 * iso_c_binding so that reference test/driver1.f90, driver2.f90, driver3.f90
 * link unchanged.
 */
#ifndef LBFGSB_HIP_H
#define LBFGSB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lbfgsb_hip_ctx lbfgsb_hip_ctx; /* opaque */

/* status codes */
enum {
  LBFGSB_OK = 0,
  LBFGSB_E_NOGPU = -100,   /* no usable HIP device / kernel launch failed   */
  LBFGSB_E_ARG = -101,     /* bad argument (n<=0, m<=0, m>LBFGSB_MAX_M ...) */
  LBFGSB_E_ALLOC = -102,   /* device allocation failed                      */
  LBFGSB_E_COMM = -103,    /* RCCL / host reducer failure                   */
  LBFGSB_E_STATE = -104    /* call sequence violates the task protocol      */
};

/* m: the fused passes hold all 2 m operands of a row group in registers and are unrolled for at most
 * LBFGSB_FUSED_M pairs (two passes over W per iteration; beyond 21 stored pairs the first one runs as
 * several launches over a part of the columns each); beyond that a context runs that first pass the same
 * way in front of unfused tile kernels for the subspace steps (k_wide.hip) -- two passes over W as well,
 * a few more vector kernels.  LBFGSB_MAX_M only bounds the host's O(m^2) arrays. */
#define LBFGSB_FUSED_M 32
#define LBFGSB_MAX_M 1024

/* flags for lbfgsb_hip_create */
enum {
  LBFGSB_F_REAL32 = 1,       /* REAL32 build of the reference (lbfgsb_kinds_module.F90:29):
                                fp32 storage + kernels, fp64 partials and host algebra */
  LBFGSB_F_MIRROR_INDEX = 2, /* keep the reference's Index/Indx2 lists (freev,
                                src/lbfgsb.f90:2044-2054, 2014-2035) on the device so
                                that lbfgsb_hip_export_state reproduces `iwa` */
  LBFGSB_F_NO_RETURN_SYNC = 4, /* the caller evaluates f,g on the SAME stream: do not block the
                                host when returning task='FG_LNSRCH' (x is ordered by the stream) */
  LBFGSB_F_PARALLEL_GCP = 8, /* OPT-IN deviation from the reference's arithmetic: when no pair is
                                stored (col = 0: first iteration, after every memory refresh -- the
                                calls where nseg ~ n) the model Hessian is theta*I, the derivative
                                along the projected path is -(1 - theta t) * sum_{t_j >= t} d_j^2,
                                and the generalized Cauchy point is t* = 1/theta in closed form: one
                                elementwise kernel instead of the ordered walk of
                                src/lbfgsb.f90:1378-1497.  Equal to the reference in exact arithmetic;
                                in floating point the reference's f1/f2 recurrence carries its own
                                rounding noise, so tsum (and nseg by a few units) may differ.  The
                                clamp f2 >= epsmch*f2_org (:1483) acts only once the gradient mass
                                still moving is below epsmch of the total: that is checked first and
                                such calls take the exact walk.
                                With pairs stored (col > 0) the flag replaces LONG walks (more than
                                32768 breakpoints within reach) by a full sort + prefix scans of the
                                walk's state on the device, the clamp included (a scan over the maps
                                x -> max(B, x + A)) -- again the reference's result in exact
                                arithmetic, EXCEPT for the order of equal breakpoints: the search
                                takes them in (t, variable index) order and has none of the walk's
                                detection of a stop inside a group of equal t (tie_split / grp_sens,
                                see LBFGSB_F_EXACT_TIES below).  A group crossed whole gives the same
                                sums in any order; when the stop falls INSIDE a group, the members
                                with the lowest indices are the ones fixed, where the reference fixes
                                those its heap (hpsolb, :2079) pops first -- which members, and when
                                their rows of W differ how many, may then differ.  Such a call is not
                                counted by lbfgsb_hip_tie_splits and not replayed: a documented limit
                                of the opt-in mode (the col = 0 closed form fixes every t_j <= 1/theta
                                and has no such case).  With several ranks the records of all
                                breakpoints are all-gathered and every rank runs the same
                                (bitwise-reproducible) scans.  Short walks always replay the walk
                                exactly.  tests/test_gpu_pgcp_door.py holds one call of either form
                                against an extended-precision walk. */
  LBFGSB_F_EXACT_TIES = 16,  /* accepted and ignored: this IS the default behaviour now (round 3).
                                Breakpoints with EQUAL t reach the walk in variable order; the reference
                                pops them in the order of hpsolb's heap (src/lbfgsb.f90:2079, used at
                                :1384-1403).  Sums over a whole group of equal breakpoints are merely
                                reassociated; the two orders differ in effect only when the walk ends
                                INSIDE such a group -- then the order decides which of its variables are
                                fixed at their bounds.  Such calls are detected, counted
                                (lbfgsb_hip_tie_splits) and REPLAYED from the start of the walk in the
                                reference's own order: all breakpoint times travel to the host of
                                every rank (O(n) bytes + an O(n) heap build; every rank pops the same
                                replicated heap and gathers the records of the rows it owns), so the
                                active set equals the reference's bit for bit.  Only the calls that
                                need it pay for it. */
  LBFGSB_F_INDEX_TIES = 32,  /* OPT-OUT of that replay: a walk that ends inside a group of equal
                                breakpoints fixes the group's members in variable order (which members --
                                and, when their rows of W differ, how many -- may then differ from the
                                reference).  For callers who prefer the
                                O(window) cost bound over the reference's tie order: the replay costs
                                what the reference's own walk costs (heap pops over all breakpoints). */
  LBFGSB_F_DEFER_LNSRCH = 64, /* for callers that evaluate f,g on the context's own stream and do nothing
                                else with the context between an 'FG_LNSRCH' return and the re-entry with
                                that evaluation (lbfgsb_hip_minimize with a built-in objective, bench.py).
                                The pass that forms the subspace step also stores the first trial point
                                of the line search, x = z (lnsrlb, src/lbfgsb.f90:2265: the unit step), and
                                produces the numbers its set-up needs (d'd, g'd, stpmx, subsm's iword,
                                :2196-2244, :2820-2828).  By default the call waits for them before it
                                returns 'FG_LNSRCH'.  With this flag it returns at once -- no host sync
                                in that call, implies LBFGSB_F_NO_RETURN_SYNC -- and the numbers come
                                over with the first fetch of the NEXT call, which then runs the set-up
                                and, in the same call, the step of dcsrch that consumes the evaluation:
                                one host round trip per iteration less.  Same arithmetic in the same
                                order: every 'NEW_X' return (x, f, g, isave, dsave, the exported state)
                                is bit for bit the default's.  What differs:
                                 * at such an 'FG_LNSRCH' return dsave / isave / csave do not describe
                                   the line search yet, and lbfgsb_hip_export_state is refused
                                   (LBFGSB_E_STATE) until the next 'NEW_X';
                                 * when the set-up turns out to ask for ANOTHER point than x = z --
                                   subsm's backtracking step (:2830-2879), an ascent direction (:2247)
                                   -- the evaluation the caller has just delivered is dropped (it is not
                                   counted in nfgv) and the call returns 'FG_LNSRCH' once more, with
                                   the point the reference would have asked for (lbfgsb_hip_defer_stats
                                   counts these).
                                Not with LBFGSB_F_MIRROR_INDEX, LBFGSB_F_PARALLEL_GCP or iprint >= 99: such
                                contexts wait as before (m > LBFGSB_FUSED_M: deferred while col <= 96 and the
                                options "wide_tail" / "wide_one" are on, the defaults). */
  LBFGSB_F_FOLLOW_BOUNDS = 128 /* follow bounds that the caller edits during a run, as the reference does (it
                                re-reads l, u, nbd on every call).  Every entry after 'START' compares the
                                caller's l, u, nbd with the context's snapshot, bit for bit, before it
                                launches anything that reads bounds: one pass over the three arrays (20 bytes
                                per row in fp64 with uniform bounds, 37 with streamed ones) and one host sync.
                                On a difference the snapshot is rebuilt and the call continues with the
                                reference's semantics; products an earlier call computed ahead of time from the
                                old bounds are dropped.  Other array pointers than in the last call count as
                                a difference.  Such a context never returns 'ERROR: BOUNDS CHANGED DURING RUN'
                                (option "bounds_check" is ignored).  What the reference keeps from 'START'
                                stays: prjctd, cnstnd, boxed and the projection of x0 (errclb and active do
                                not run again).  An nbd value outside 0..3 ends the run with
                                'ERROR: INVALID NBD' (isave(35), info, = -6).  Edits are made in stream order:
                                complete, or ordered on the context's stream, before the next call -- the rule
                                that applies to g.  Sharded runs: the changed-row count (a new pointer on
                                one rank included) is reduced over the ranks, so every rank rebuilds at the
                                same entry.  LBFGSB_F_DEFER_LNSRCH (and option "defer_lnsrch") is turned off
                                in such a context: a deferred line-search set-up would run with the bounds of
                                the next call, where the reference uses those of its own; the set-up then
                                runs in its own call -- the same numbers, one host sync more.  Only the
                                device-pointer forms follow edits; the host form keeps the default.  Not
                                needed by a caller that announces its edits (lbfgsb_hip_bounds_changed). */
};

/* -------------------------------------------------------------------------
 * Context.  Replaces the partition of caller memory done by setulb
 * (src/lbfgsb.f90:250-265): Ws, Wy (n x m each, column-major, leading
 * dimension padded to 32 rows), z, r, d, t, xp, iwhere and scratch live in
 * HBM for the life of the context.
 *   n_local   rows owned by this rank          n_global  total rows
 *   row0      global 0-based index of local row 0 (contiguous block sharding)
 * For one GPU: n_local = n_global = n, row0 = 0.
 * stream: a hipStream_t (may be NULL = a private stream is created).
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_create(int64_t n_local, int64_t n_global, int64_t row0, int m, int flags,
                      int device, void *stream, lbfgsb_hip_ctx **out);
void lbfgsb_hip_destroy(lbfgsb_hip_ctx *ctx);
const char *lbfgsb_hip_last_error(void);

/* -------------------------------------------------------------------------
 * Multi-GPU: every n-length reduction of the path is completed across ranks.
 * (a) RCCL on the context's stream (librccl is dlopen'ed on first use):
 *       id = 128-byte ncclUniqueId made by lbfgsb_hip_rccl_unique_id on rank 0
 *       and distributed by the caller (e.g. torch.distributed broadcast).
 *       ONE collective per host sync: the <= 8m+15 fp64 partials of a phase (sums,
 *       minima, maxima together) are all-gathered and reduced on every rank's host in
 *       rank order -- an all-reduce whose result is bit-identical on every rank and
 *       independent of the collective algorithm RCCL picks.
 * (b) a host callback, for launchers that already own a communicator
 *     (MPI, gloo): called with the rank-local partials in host memory; must
 *     return with buf[0..nsum) summed, buf[nsum..nsum+nmin) min-reduced and
 *     the following nmax entries max-reduced over all ranks.  gather: if
 *     non-NULL, must all-gather `bytes` bytes from every rank into out
 *     (rank-major).
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_rccl_unique_id(void *id128);
int lbfgsb_hip_comm_init_rccl(lbfgsb_hip_ctx *ctx, const void *id128, int rank, int nranks);
/* (ncclCommInitRank waits for every rank; the entry gives it LBFGSB_COMM_INIT_TIMEOUT_S seconds -- an
 *  environment variable, default 120; anything but a positive number is LBFGSB_E_ARG -- and returns
 *  LBFGSB_E_COMM after that instead of hanging.  A helper thread is then still inside the call: the process
 *  MUST EXIT after this error (non-zero; do not re-launch in place, do not destroy the context and carry on).
 *  Should the peers arrive later after all, the helper destroys the late communicator itself.)
 * What the context's communicator is: *kind = 0 none (one rank), 1 RCCL, 2 host callbacks; for RCCL
 * *nranks / *rank are the communicator's OWN answers (ncclCommCount, ncclCommUserRank), so a scaling
 * run can show that N ranks really took part. */
int lbfgsb_hip_comm_info(lbfgsb_hip_ctx *ctx, int32_t *nranks, int32_t *rank, int32_t *kind);
typedef int (*lbfgsb_allreduce_fn)(void *user, double *buf, int nsum, int nmin, int nmax);
typedef int (*lbfgsb_allgather_fn)(void *user, const void *in, void *out, int64_t bytes);
int lbfgsb_hip_comm_init_host(lbfgsb_hip_ctx *ctx, lbfgsb_allreduce_fn ar,
                              lbfgsb_allgather_fn ag, void *user, int rank, int nranks);

/* -------------------------------------------------------------------------
 * setulb, device-pointer form.  Mirrors reference setulb (src/lbfgsb.f90:88)
 * argument for argument except that
 *   - n, m, wa, iwa are replaced by the context,
 *   - x, l, u, nbd, g are DEVICE pointers to this rank's rows (real = double,
 *     or float with LBFGSB_F_REAL32; nbd int32), 16-byte aligned,
 *   - f, factr, pgtol are double; f is the GLOBAL objective value,
 *   - task/csave are 60 bytes, blank padded, no terminator (Fortran layout),
 *   - lsave[4] are int32 0/1, isave[44] int32, dsave[29] double, with the
 *     reference's meaning slot for slot (src/lbfgsb.f90:188-242).
 * The caller evaluates f,g on the device whenever task(1:2)=='FG'.
 * l, u and nbd MUST NOT CHANGE between task='START' and the end of the run.  The reference re-reads the three
 * arrays on every call (src/lbfgsb.f90:1270-1330, 2594-2622, 2789-2816); this library's passes over W read a
 * snapshot: a packed one-byte copy of nbd (refreshed on START, after import_state and when the nbd POINTER
 * changes), and for bound arrays found at START to hold one value each, or a few values (<= 8 each), that
 * constant / a table entry selected by the packed byte (lbfgsb_hip_uniform_bounds below).  An edit IN PLACE is
 * detected, not ignored: after the first iteration and then every 32nd (option "bounds_check") the caller's
 * arrays are compared with the snapshot bit for bit, and a difference ends the run with
 * task = 'ERROR: BOUNDS CHANGED DURING RUN' (isave(35), info, = -10).  Passing OTHER array pointers than at
 * START is allowed: the constants / tables are dropped and the arrays are streamed from then on.  A caller that
 * has to change bounds during a run creates the context with LBFGSB_F_FOLLOW_BOUNDS, or announces each edit
 * (lbfgsb_hip_bounds_changed), or starts a new run (task='START').
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_setulb_dev(lbfgsb_hip_ctx *ctx, void *x, const void *l, const void *u,
                          const int32_t *nbd, double *f, void *g, double factr, double pgtol,
                          char *task, int iprint, char *csave, int32_t *lsave, int32_t *isave,
                          double *dsave);

/* -------------------------------------------------------------------------
 * setulb, device-pointer form with PING-PONG iterate buffers.  The reference's line search starts
 * every iteration with two n-vector copies, t = x and r = g (lnsrlb, src/lbfgsb.f90:2235-2236), so
 * that the previous iterate survives the trial points written into x and g.  On a bandwidth-bound
 * device those copies are 16 of the 40 bytes per row the one storing pass of an iteration writes.
 * Here the caller hands over TWO buffers for x and TWO for g; nothing is copied: the pair that holds
 * the iterate BECOMES (t, r), the trial point is written to the other pair.
 *   *cur (out) = which pair (0 or 1) this return refers to:
 *     task 'FG...'        evaluate f at x[*cur], write the gradient into g[*cur], pass f as usual;
 *     task 'NEW_X', terminal tasks   x[*cur], g[*cur] are the iterate and its gradient.
 *   task 'START': x0 holds the starting point (the call returns 'FG_START' with *cur = 0).
 * The four buffers must stay the same for the whole run; a run uses either this entry or
 * lbfgsb_hip_setulb_dev, not both (LBFGSB_E_STATE).  A run resumed from lbfgsb_hip_import_state may
 * continue through either entry (here: iterate and gradient in x0 / g0, *cur = 0 until the next step).  Everything else -- task protocol, isave / dsave /
 * lsave, results bit for bit -- as lbfgsb_hip_setulb_dev; lbfgsb_hip_export_state writes the
 * reference's t and r slots from wherever they live.
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_setulb_dev_pp(lbfgsb_hip_ctx *ctx, void *x0, void *x1, const void *l, const void *u,
                             const int32_t *nbd, double *f, void *g0, void *g1, double factr,
                             double pgtol, char *task, int iprint, char *csave, int32_t *lsave,
                             int32_t *isave, double *dsave, int32_t *cur);

/* Stream ordering.  Every kernel of a context runs on ITS stream (the one given to
 * lbfgsb_hip_create, or a private non-blocking stream).  On an 'FG...' re-entry the library
 * reads g (and x, if the caller touched it) on that stream: whatever produced them must be
 * complete, or ordered before the context's stream.  Either evaluate f,g on the context's
 * stream (lbfgsb_hip_get_stream), or call lbfgsb_hip_wait_stream(ctx, producer_stream) before
 * the re-entry -- it records an event on producer_stream and makes the context's stream wait
 * for it, without blocking the host -- or synchronise the producer.  Unless
 * LBFGSB_F_NO_RETURN_SYNC is set, an 'FG...' RETURN has already synchronised the context's
 * stream, so x may be read from any stream. */
void *lbfgsb_hip_get_stream(lbfgsb_hip_ctx *ctx);
int lbfgsb_hip_wait_stream(lbfgsb_hip_ctx *ctx, void *producer_stream);
/* The mirror of lbfgsb_hip_wait_stream, for a caller whose objective runs on ANOTHER stream and who wants no host
 * sync at an 'FG...' return (LBFGSB_F_NO_RETURN_SYNC, LBFGSB_F_DEFER_LNSRCH): an event is recorded on the context's
 * stream behind everything the last call queued -- the storing pass that wrote the trial point included
 * (src/lbfgsb.f90:2255-2272: the point the caller is asked to evaluate) -- and, with make_wait != 0,
 * consumer_stream is made to wait for it (0 is the legacy default stream).  *event_out (may be NULL) receives the
 * hipEvent_t, owned by the context and re-recorded by the next call of this function.  The round trip of such a
 * caller:  setulb -> 'FG...' ; lbfgsb_hip_return_event(ctx, s, 1, NULL) ; f, g evaluated on s ;
 * lbfgsb_hip_f_device / lbfgsb_hip_wait_stream(ctx, s) ; setulb.  Nothing in it blocks the host. */
int lbfgsb_hip_return_event(lbfgsb_hip_ctx *ctx, void *consumer_stream, int make_wait, void **event_out);
/* The caller's objective value as a device scalar (fp64; with several ranks: this rank's part of f, the library
 * adds the parts up): it reaches the host with the next setulb call's first fetch, as the value of a built-in
 * objective evaluated with h_f == NULL does (lbfgsb_hip_objective), and that call stores it in *f -- the 'f'
 * argument of that call is ignored on entry.  order_after != 0: first order the context's stream behind
 * producer_stream (lbfgsb_hip_wait_stream), on which *d_f and g were produced.  Only for an 'FG...' re-entry. */
int lbfgsb_hip_f_device(lbfgsb_hip_ctx *ctx, const void *d_f, void *producer_stream, int order_after);

/* -------------------------------------------------------------------------
 * setulb, host-pointer form: the exact reference signature (what the Fortran
 * shim binds).  x,l,u,g are host arrays of the real kind, nbd/iwa/isave
 * default integers (int32), lsave int32.  The context handle is kept in
 * isave(17:18) (never touched by the reference, src/lbfgsb.f90:250-284),
 * created on task='START' and released when a terminal task is returned (or by
 * lbfgsb_hip_release_host).
 * What crosses PCIe per call, and only then: g host -> device on an 'FG...' entry; x device -> host at START
 * (active's projection), at every 'FG_LNSRCH' return (the trial point) and when the call restored the previous
 * iterate (src/lbfgsb.f90:568-569, 736-737: then g too); `wa`'s t-slot (wa(3n+2mn+11m^2+1 : +n), the previous
 * iterate test/driver3.f90:171-175 reads) when a line search was set up in the call (:2235).  At 'NEW_X' and at
 * the convergence returns the caller already holds x and g: nothing n-long moves.  The caller's x, g and that
 * slot of wa are pinned (hipHostRegister) from START to the end of the run, so the transfers are DMA copies
 * queued on the context's stream; the call returns when they have landed.  Nothing else of wa / iwa is written
 * unless mirror != 0, in which case the full reference layout of wa and iwa is exported on every return.
 * iteration_file may be NULL (-> 'iterate.dat', src/lbfgsb.f90:483-489).
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_setulb_host(int32_t n, int32_t m, void *x, const void *l, const void *u,
                           const int32_t *nbd, void *f, void *g, double factr, double pgtol,
                           void *wa, int32_t *iwa, char *task, int32_t iprint, char *csave,
                           int32_t *lsave, int32_t *isave, void *dsave,
                           const char *iteration_file, int32_t real_bytes, int32_t mirror);
/* The same for a caller whose default INTEGER / LOGICAL kind is int_bytes wide (4 or 8): nbd, iwa,
 * lsave, isave are arrays of that width, n / m / iprint travel as int64.  This is the entry the
 * Fortran module binds (int_bytes = storage_size(1)/8), so that ONE source serves an ordinary build
 * and a -fdefault-integer-8 build -- the build BASELINE.md section 3 calls mandatory for n = 1e8,
 * because the reference's own wa offsets (src/lbfgsb.f90:246-265) overflow a 32-bit integer there.
 * With 8-byte integers isave(1:16) receive those offsets in full; n < 2^31 - 16 on one device.
 * m > LBFGSB_MAX_M is answered the way the reference answers its own argument errors: task =
 * 'ERROR: M > 1024 (LIMIT OF LBFGSB_HIP)', return value 0, no iteration done (the reference itself puts
 * no upper limit on m, :93-97). */
int lbfgsb_hip_setulb_host_ik(int64_t n, int64_t m, void *x, const void *l, const void *u, const void *nbd,
                              void *f, void *g, double factr, double pgtol, void *wa, void *iwa,
                              char *task, int64_t iprint, char *csave, void *lsave, void *isave,
                              void *dsave, const char *iteration_file, int32_t real_bytes,
                              int32_t mirror, int32_t int_bytes);
int lbfgsb_hip_release_host_ik(void *isave, int32_t int_bytes);
/* A caller that leaves its loop without a terminal task FROM the library -- the reference's own
 * driver2/driver3 set task = 'STOP...' and exit (test/driver2.f90:174-195) -- releases the
 * context of the host-pointer form with this call (the Fortran module exports it as
 * lbfgsb_release).  isave(17:18) hold a registry id + tag, never a raw pointer: a stale or
 * garbage isave is refused (LBFGSB_E_STATE), a 'START' over a live id frees the old context
 * first; whatever is still registered at process exit is left to the process teardown (no GPU
 * call is made from a static destructor).  isave(1:16)
 * receive the reference's wa offsets (:250-265), saturated at INT32_MAX instead of wrapped. */
int lbfgsb_hip_release_host(int32_t *isave);
/* Pinning of the caller's arrays by the host-pointer form, for the whole process: mode 1 (default) = START
 * registers x, g and wa's t slot with hipHostRegister (3 n real_bytes: 2.4 GB at n = 1e8) until the run's
 * context goes; mode 0 = never, every transfer is a pageable copy (slower per call, nothing to undo).  Use 0 for
 * short runs of large problems, and for callers that may free x / g / wa of a run they abandoned without
 * lbfgsb_hip_release_host: an array must not be freed while it is registered.  What the library does by itself:
 * a call that arrives with another x, g or wa than START's releases that registration; a START whose arrays
 * overlap the registrations of a run still on the registry drops that (abandoned) run first. */
int lbfgsb_hip_host_pinning(int mode);

/* -------------------------------------------------------------------------
 * Convenience driver around lbfgsb_hip_setulb_dev -- the "high-level wrapper so the user
 * doesn't have to call the reverse communication routine directly" that the reference lists
 * as @todo (src/lbfgsb.f90:36-37).  Runs the loop of test/driver2.f90: evaluates f,g whenever
 * task(1:2)=='FG' -- through `fg` (device pointers in, GLOBAL f out), or, when fg == NULL, the
 * built-in objective `builtin_kind` of lbfgsb_hip_objective -- and stops on a terminal task or
 * when max_iter iterations / max_fg evaluations are reached ('STOP: ...' as the drivers do).
 * On return *f, x, g hold the final point; task/isave/dsave/lsave as after the last setulb.
 * ------------------------------------------------------------------------- */
typedef double (*lbfgsb_fg_fn)(void *user, const void *x_dev, void *g_dev);
int lbfgsb_hip_minimize(lbfgsb_hip_ctx *ctx, void *x, const void *l, const void *u,
                        const int32_t *nbd, void *g, double factr, double pgtol, int max_iter,
                        int max_fg, int iprint, lbfgsb_fg_fn fg, void *user, int builtin_kind,
                        double *f, char *task, int32_t *lsave, int32_t *isave, double *dsave);

/* -------------------------------------------------------------------------
 * State exchange with the reference's caller-array layout (checkpoint /
 * resume; used by the one-step parity tests).
 * wa: host, length 2mn+5n+11m^2+8m reals; iwa: host int32[3n].
 * export: fills every slot that has a defined meaning at a setulb return
 *   (SURVEY.md appendix B).  import: loads Ws, Wy, z, r, d, t, xp, iwhere,
 *   the free-set membership (from Index(1:nfree)), Sy, Ss, Wt, Wn, Snd, wa8m.
 * With several ranks every rank exports / imports ITS rows (n = n_local in the
 * lengths above; the 2m x 2m matrices are replicated; Index is the local list and
 * Indx2(1) carries this rank's number of free rows): checkpoint at a NEW_X return,
 * resume with the saved task / csave / lsave / isave / dsave on the same partition.
 * Contexts with LBFGSB_F_MIRROR_INDEX are single-rank.
 * ------------------------------------------------------------------------- */
int lbfgsb_hip_export_state(lbfgsb_hip_ctx *ctx, void *wa, int32_t *iwa);
int lbfgsb_hip_import_state(lbfgsb_hip_ctx *ctx, const void *wa, const int32_t *iwa,
                            const int32_t *isave);

/* -------------------------------------------------------------------------
 * The curvature model as a device operator.
 * At a setulb return the context holds what the reference's wa holds there: col stored pairs (s_j, y_j) -- the
 * columns of Ws / Wy in ring order from head --, theta (dsave(1)), Sy (L + D of S'Y), Ss (upper triangle of S'S)
 * and Wt (formt's Cholesky factor).  From them, with W = [Y, theta S] and M the 2col x 2col middle matrix of bmv:
 *   LBFGSB_QN_B:  B = theta I - W M W'  -- the matrix whose products bmv forms (src/lbfgsb.f90:1057-1123), that is
 *                 theta I updated by the col BFGS updates in ring order (col = 0: B = theta I);
 *   LBFGSB_QN_H:  H = B^-1, in the compact form of Byrd, Nocedal and Schnabel:
 *                 H = theta^-1 I + [S, theta^-1 Y] [[R^-T (D + theta^-1 Y'Y) R^-1, -R^-T], [-R^-1, 0]] [S'; theta^-1 Y']
 *                 with R the upper triangle of S'Y (diagonal included).  R's strict upper part and Y'Y are not state
 *                 the iteration keeps: one Gram pass over all rows computes them, once per set of pairs.
 * H starts from the solver's own theta (scipy's LbfgsInvHessProduct starts from H0 = I): it is exactly the inverse
 * of the matrix the solver uses.
 *
 * qn_apply: out_j = A v_j for k vectors (A = B or H), vector j at v + j*ldv, result j at out + j*ldo (ldv, ldo >=
 *   n_local; device memory of the context's real kind; out may not overlap v).  qn_diag: out = diag(A) (n_local
 *   reals), at most 32 stored pairs (a per-row quadratic form of width 2col: LBFGSB_E_ARG beyond).
 * The entries read the pairs of the context's last return, or of the last import_state (theta then y'y / s'y of the
 * newest pair, as matupd computes it).  They are valid at every return at which lbfgsb_hip_export_state is
 * (FG_START, NEW_X, FG_LNSRCH unless its set-up is deferred, CONVERGENCE / ABNORMAL / STOP) and after
 * lbfgsb_hip_minimize.  LBFGSB_E_STATE, changing nothing: a deferred line-search set-up is live, a built-in
 * objective's value is still on the device, or the context has no run.  LBFGSB_E_ARG: NULL, k < 1, ld < n_local.
 * Calling them changes nothing the run computes: every later return is bit-identical with or without the calls.
 * Streams: as lbfgsb_hip_setulb_dev -- v is read on the context's stream; out is complete when the call returns,
 * or, with LBFGSB_F_NO_RETURN_SYNC, ordered on that stream (lbfgsb_hip_return_event).  qn_apply waits for its
 * sums on the host once per 4 vectors.  Several ranks: every rank calls collectively with its own rows; the sums
 * are reduced as the iteration's (rank order / the host reducer), so every rank uses the same coefficients.
 * REAL32 contexts: v and out are fp32, every sum fp64.
 *
 * Square roots, log-determinants and draws.  Both models are A = alpha I + [S, Y] N [S, Y]' (alpha = theta for B,
 * 1 / theta for H), so with G = [S, Y]'[S, Y], P = G^(1/2) and P N P = V diag(delta) V'
 *   A^(1/2) = sqrt(alpha) I + [S, Y] C [S, Y]',
 *   C = N / (2 sqrt(alpha)) - (N P V) diag(1 / (2 sqrt(alpha) (sqrt(alpha) + sqrt(alpha + delta_i))^2)) (N P V)'
 *   log det A = n_global log alpha + sum_i log1p(delta_i / alpha)
 * -- the symmetric square root, from two symmetric eigenproblems of order 2col on the host (a cyclic Jacobi in a
 * fixed order: the same bits on every rank), once per set of pairs; G comes from Ss and the Gram pass above.  At
 * most LBFGSB_QN_ROOT_MAXCOL stored pairs (LBFGSB_E_ARG beyond); LBFGSB_E_STATE when alpha + delta_i < -1e-8 alpha
 * (the model is not positive definite).
 *   qn_apply with LBFGSB_QN_B_SQRT / LBFGSB_QN_H_SQRT: out_j = A^(1/2) v_j, everything else as for B / H (qn_diag
 *     takes no root mode: LBFGSB_E_ARG).  The modes 2 and 3 stay invalid, as they were.
 *   qn_logdet: *h_logdet = log det A over all n_global rows, the same value on every rank (collective on several
 *     ranks, as qn_apply); no stored pair: +- n_global log theta.
 *   qn_draw: out_j = mean + scale A^(1/2) z_(first + j), j < k, result j at out + j*ldo: a draw from N(mean,
 *     scale^2 A) (mode LBFGSB_QN_B or LBFGSB_QN_H names the covariance A).  mean (n_local reals) may be NULL; it is
 *     read once per sample and may not overlap out.  The standard normal z_s is generated inside the two passes over
 *     W and never stored.  Entry i of z_s is a function of (seed, the global row row0 + i, s) and nothing else -- not
 *     of the sharding, k, the launch shape or the layout of W: Philox4x32-10 (Random123 constants) with counter (row
 *     lo, row hi, pair lo, pair hi), pair = s >> 1, key (seed lo, seed hi); from the output words a = w0 2^32 + w1,
 *     b = w2 2^32 + w3: u = ((a >> 12) + 0.5) 2^-52, v = (b >> 12) 2^-52, r = sqrt(-2 log u); an even s takes
 *     r cospi(2v), an odd one r sinpi(2v).  REAL32 contexts: z and all arithmetic in fp64, rounded on store.
 * When, streams and refusals are qn_apply's.  LBFGSB_E_ARG in addition: NULL out / h_logdet, k < 1, first < 0,
 * ldo < n_local, a mode other than B / H, a scale that is not finite.
 *
 * Quadratic forms and Gaussian log-densities.  With d = v - center and p = [S, Y]'d, d'A d = alpha d'd + p'N p: ONE
 * pass over W per block of 4 vectors, which carries d'd along and writes nothing.  All results are host doubles,
 * complete over all ranks and the same bits on each; the entries wait for their sums whatever
 * LBFGSB_F_NO_RETURN_SYNC says, as lbfgsb_hip_kkt's summary does.
 *   qn_quad: h_q[j] = (v_j - center)' A (v_j - center) over all n_global rows, j < k, vector j at v + j*ldv.  mode is
 *     LBFGSB_QN_B or LBFGSB_QN_H and names A; the root modes and the modes 2 and 3 are LBFGSB_E_ARG (the quadratic
 *     form of A^(1/2) is not offered).  center (n_local reals) may be NULL; it is read once per vector.  Any number
 *     of stored pairs.  REAL32 contexts: v and center are fp32, the difference and every sum fp64.
 *   qn_logpdf: h_logp[j] = -1/2 [ n_global log 2 pi + 2 n_global log |scale| + log det A + q_j / scale^2 ], the
 *     log-density of N(mean, scale^2 A) at x_j.  mode names the COVARIANCE A, as it does for qn_draw; q_j is the
 *     quadratic form of the OTHER mode (A^-1) at x_j - mean.  log det A is qn_logdet's: the same cache, at most
 *     LBFGSB_QN_ROOT_MAXCOL stored pairs, LBFGSB_E_STATE for a model that is not positive definite.
 *   qn_draw_logpdf: qn_draw -- out is bit for bit what qn_draw writes for the same arguments -- which also returns
 *     h_logp[j] = -1/2 [ n_global log 2 pi + 2 n_global log |scale| + log det A + z_(first + j)' z_(first + j) ],
 *     the log-density of draw j under N(mean, scale^2 A), with z the generated fp64 deviates: z'z is summed inside
 *     the W'z pass, where every z already is in a register.  REAL32 contexts: this is the density of the draw
 *     BEFORE it is rounded to fp32 on store; qn_logpdf at the stored fp32 draw differs by that rounding.
 * When, streams, the collective rule and the refusals are qn_apply's.  LBFGSB_E_ARG in addition, changing nothing:
 * NULL v / x / out / h_q / h_logp, k < 1, first < 0, ld < n_local, a mode other than B / H, and for the two
 * log-densities a scale that is 0 or not finite.
 *
 * Gram matrices.  qn_quad's values are the diagonal of the k x k matrix (V - center)' A (V - center); qn_gram returns
 * all of it: the covariance C'H C of k linear functionals under N(x*, H), the Rayleigh-Ritz projection V'B V onto a
 * subspace, Mahalanobis Gram matrices of points or draws.  With d_a = v_a - center and p_a = [S, Y]'d_a,
 * d_a'A d_b = alpha d_a'd_b + p_a'N p_b: qn_quad's pass over W per block of 4 vectors, which carries the block's
 * d_a'd_b (a <= b) along, and for two vectors of different blocks a pass over the vectors alone.  Nothing is written
 * on the device.
 *   qn_gram: h_g[a + b*ldg] = (v_a - center)' A (v_b - center) over all n_global rows, a, b < k <=
 *     LBFGSB_QN_GRAM_MAXK, vector j at v + j*ldv.  h_g is a host array; both triangles are written, entry (b, a) a
 *     copy of entry (a, b) -- symmetric bit for bit -- and rows a >= k of a column (ldg > k) are left alone.  mode,
 *     center, the stored pairs and REAL32 contexts as for qn_quad; complete over all ranks, the same bits on each, and
 *     the call waits for its sums as qn_quad does.  g_aa is qn_quad's formula on the same kind of sums.
 *     Not offered: a two-operand form U'A V -- stack [U, V] and read the off-diagonal block -- and the root modes
 *     (the Gram of A^(1/2) is qn_gram of A itself on other vectors; LBFGSB_E_ARG).
 * When, streams, the collective rule and the refusals are qn_apply's.  LBFGSB_E_ARG in addition, changing nothing:
 * NULL v / h_g, k < 1, k > LBFGSB_QN_GRAM_MAXK, ldv < n_local, ldg < k, a mode other than B / H.
 *
 * Eigenvalues and eigenvectors.  With the delta_i of the square root above, A has the eigenvalue alpha + delta_i
 * with the unit eigenvector u_i = [S, Y] (N P V)_i / delta_i for every delta_i != 0, and the bulk eigenvalue alpha
 * on the n_global - r remaining dimensions: A = alpha I + U diag(lambda - alpha) U' with orthonormal U.  A direction
 * with |delta_i| <= LBFGSB_QN_EIG_CUT alpha counts as bulk and is not returned, so r <= min(2col, n_global); nearly
 * parallel pairs lower r and cost no accuracy elsewhere (no division by G).  The host part is the root's (the same
 * Gram pass, once per set of pairs; at most LBFGSB_QN_ROOT_MAXCOL stored pairs, LBFGSB_E_ARG beyond; LBFGSB_E_STATE
 * for a model that is not positive definite, as qn_logdet).
 *   qn_eig: *h_bulk = alpha (theta for B, 1 / theta for H), *h_r = r, and h_lambda[0 .. min(r, cap)) the r eigenvalues
 *     alpha + delta_i in ascending order -- host doubles, the same bits on every rank.  cap = 0 with h_lambda = NULL
 *     is the counting call.  No stored pair: r = 0.  No pass over W besides the Gram pass.  The eigenvalues of B and
 *     of H are reciprocal up to rounding.
 *   qn_eigvec: out + j*ldo receives the n_local rows of the unit eigenvector of eigenvalue number h_which[j], a 0-based
 *     index into qn_eig's ascending list of the same mode, j < k <= 128; repeats are allowed, h_which = NULL means
 *     0 .. k-1.  One pass over W per tile of 16 stored pairs writes all k vectors (fp64 sums, rounded on store in
 *     REAL32 contexts).  The sign makes the largest coefficient of u_i in the [S, Y] basis positive (the first of
 *     equals): a function of replicated host data, the same on every rank and for every sharding.  A repeated
 *     eigenvalue returns some orthonormal basis of its eigenspace.
 *     Accuracy: the bulk eigenspace has n_global - r dimensions, so a vector whose eigenvalue lies delta_i off alpha
 *     is determined by fp64 data only up to about eps |A| / |delta_i|.  Vectors with |delta_i| >= 1e-3 alpha are
 *     orthonormal to the accuracy of qn_apply; just above the cut (|delta_i| ~ 1e-8 alpha) the norm and the angles of
 *     a vector may be off by 1e-6, while A u_i = lambda_i u_i still holds to the accuracy of qn_apply, because such a
 *     vector's error lies in directions that A maps like the bulk.
 * When, streams, the collective rule and the refusals are qn_apply's (every rank calls with its own rows).
 * LBFGSB_E_ARG in addition, changing nothing: NULL h_r / h_bulk / out, cap < 0, cap > 0 with h_lambda = NULL, k < 1,
 * k > 128, an index outside 0 .. r-1, ldo < n_local, a mode other than B / H.
 *
 * The model plus a diagonal.  A Laplace posterior with a Gaussian prior has the precision B + diag(tau); a
 * trust-region, Levenberg-Marquardt or proximal Newton step solves with B + mu I; the model on the free variables is
 * the limit d_i -> infinity on the rows at bounds.  None of them is a function of B's spectrum.  With
 * Delta = (theta + mu) I + D, w = 1 / Delta elementwise (w_i = 0 on a pinned row) and W = [Y, theta S]:
 *   (B + mu I + D)^-1 = diag(w) + diag(w) W K^-1 W' diag(w),   K = M^-1 - W' diag(w) W   (2col x 2col),
 *   log det           = sum over the free rows of log Delta_i + log |det K| - log |det M^-1|,
 *   diag              = w_i + w_i^2 r_i' K^-1 r_i,   r_i = row i of W,
 * with M^-1 = [[-D_sy, L'], [L, theta S'S]] from Sy and Ss.  K is factorised on the host by two Cholesky factors (the
 * negated (1, 1) block, then the Schur complement); it has col negative and col positive eigenvalues exactly when the
 * shifted model is positive definite on the free rows.
 *   qn_shift_set: d (n_local reals of the context's kind on the device, or NULL for D = 0) is read once on the
 *     context's stream and need not outlive the call; the weights go to a buffer of the context (n_local doubles).
 *     d_i = +inf pins row i: w_i = 0 exactly, its row of every later solve / diag output is +0 and it is left out of
 *     log det; *h_pinned (may be NULL) receives the number of pinned rows over all ranks.  All rows pinned is legal:
 *     solves return 0 and log det is 0.  One pass over d (16 B per row in fp64) and ceil(2col / 4) weighted passes
 *     over W, then the factor.  LBFGSB_E_ARG, the context as it was (an earlier shift of the same pairs stays in
 *     force): a NaN or infinite mu, any row with theta + mu + d_i <= 0 or NaN (counted by the pass over d), more than
 *     LBFGSB_QN_ROOT_MAXCOL stored pairs.  LBFGSB_E_STATE, the context as it was: K does not have the inertia
 *     (col, col) -- the shifted model is not positive definite on the free rows.
 *   qn_shift_solve: out_j = (B + mu I + D)^-1 v_j on the free rows (+0 on the pinned ones, whatever v holds there),
 *     j < k, vector j at v + j*ldv, result j at out + j*ldo; out may not overlap v.  Any k: per block of 4 vectors one
 *     weighted W'v pass and one weighted expansion, each 8 B per row more than qn_apply's.
 *   qn_shift_logdet: *h_logdet = log det of the shifted model on the free rows, a host double with the same bits on
 *     every rank; no device pass (the sum over log Delta_i is reduced inside qn_shift_set).  No stored pair: the sum
 *     over the free rows of log(theta + mu + d_i).
 *   qn_shift_diag: out = the diagonal of the inverse above (n_local reals), at most 32 stored pairs as qn_diag.
 * The factor belongs to the pairs it was made of: after a return that changes the pairs or theta (and before any
 * qn_shift_set) solve, logdet and diag return LBFGSB_E_STATE ("call qn_shift_set again"); they never use old weights
 * with new pairs.  When, streams, the collective rule, REAL32 (d, v, out fp32; the weights and every sum fp64) and
 * the refusals are qn_apply's, and the run does not notice the calls.
 * Not offered: the product (B + mu I + D) v -- it is qn_apply(LBFGSB_QN_B) plus an axpy with mu + d.
 *
 * Square roots, draws and log-densities of the model plus a diagonal: N(mean, scale^2 Sigma) with Sigma =
 * (B + mu I + D)^-1 on the free rows -- the Laplace posterior under a Gaussian prior -- sampled and evaluated.  With
 * the weights w of qn_shift_set and W = [S, Y],
 *   L = diag(sqrt w) + diag(w) W C W' diag(sqrt w),   L L' = Sigma,
 * where I + What C What' is the symmetric root of I + What N What', What = diag(sqrt w) W, N the matrix of the solve: C
 * comes from the weighted Gram that qn_shift_set has reduced, by the host algebra of the square roots above, at the
 * first of these calls after a qn_shift_set (qn_shift_set itself costs what it did).  L is zero on pinned rows and
 * columns; it is a factor of Sigma, not its symmetric root.
 *   qn_shift_sqrt: out_j = L v_j, vectors and results laid out as qn_shift_solve's; pinned rows of out are +0 whatever
 *     v holds there.  The two passes of qn_shift_solve with other weights, the same bytes.
 *   qn_shift_draw: out_j = mean + scale L z_(first + j), j < k, z_s the standard normal vector of qn_draw: its entry
 *     for a row depends on (seed, the global row, s) alone, so the free rows' draws do not move with the rows that are
 *     pinned, the sharding or k.  A pinned row of out is its mean bit for bit (+0 with mean = NULL).  mean: n_local
 *     reals or NULL.  Per block of 4 samples one weighted W'z pass and one weighted expansion; z is never stored.
 *   qn_shift_draw_logpdf: qn_shift_draw -- the same bits in out -- and h_logp[j] = log N(out_j; mean, scale^2 Sigma)
 *     over the free rows of all ranks, from the z'z over the free rows that the W'z pass carries.
 *   qn_shift_quad: h_q[j] = (v_j - center)'(B + mu I + D)(v_j - center) over the free rows of all ranks (center:
 *     n_local reals or NULL); what v and center hold on pinned rows is not used.  One pass per 4 vectors, nothing
 *     written on the device.
 *   qn_shift_logpdf: h_logp[j] = log N(x_j; mean, scale^2 Sigma) = -q_j / (2 scale^2) - (nf / 2) log 2 pi - nf log
 *     |scale| + log det (B + mu I + D) / 2 with nf = n_global - pinned and q_j of qn_shift_quad; the log det is the
 *     root's (sum log Delta_i - sum log1p(delta_i)), which agrees with qn_shift_logdet to rounding.  With every row
 *     pinned the log-densities are 0.
 * h_q and h_logp are host doubles with the same bits on every rank.  At most LBFGSB_QN_ROOT_MAXCOL stored pairs (which
 * qn_shift_set already demands).  LBFGSB_E_STATE: no shift in force or the pairs have changed ("call qn_shift_set
 * again"), or the root finds the shifted model not positive definite.  LBFGSB_E_ARG, nothing changed and the shift
 * still in force: NULL ctx / v / x / out / h_q / h_logp, k < 1, first < 0, ld < n_local, scale 0 or not finite.  When,
 * streams, the collective rule and REAL32 are qn_shift_solve's, and the run does not notice the calls.
 *
 * Entries at index lists.  After a Laplace fit with 1e8 parameters the first question is the marginal covariance and
 * the correlations of a few of them.  Every entry of the model depends on the rows of [S, Y] at its two indices alone:
 *   A[a, b]     = alpha [a == b] + r_a N r_b'           (A = B or H, N the 2col x 2col matrix of qn_diag),
 *   Sigma[a, b] = w_a [a == b] + w_a w_b r_a K^-1 r_b'  (Sigma = (B + mu I + D)^-1 of the shift in force),
 * so a block at k indices costs one gather of k 2col reals -- no unit vector, no pass over W.  All indices are GLOBAL,
 * 0-based int64 rows in HOST arrays, as lbfgsb_hip_kkt_list hands them out (copied to the host).  They are checked on
 * the host, 0 <= idx < n_global, before anything is launched; lists may be unsorted and may repeat indices.  On several
 * ranks every rank passes the same list, collectively: a rank contributes the rows it owns and exact zeros elsewhere,
 * the contributions are added in rank order, so the one stored value survives exactly and host results have the same
 * bits on every rank.
 *   qn_rows: h_rows[j + c*ldr] = entry h_idx[j] of logical column c of [S, Y] -- c < col: S in ring order from the
 *     oldest pair, col <= c < 2col: Y -- widened to double, exactly the stored value.  k <= LBFGSB_QN_IDX_MAXK,
 *     ldr >= k, any number of stored pairs; with no stored pair nothing is written.
 *   qn_block: h_a[a + b*lda] = A[h_ia[a], h_ib[b]], mode LBFGSB_QN_B or LBFGSB_QN_H.  h_ib = NULL means ib = ia (kb is
 *     not read): the upper triangle is computed and the lower copied from it, symmetric bit for bit.  ka, kb <=
 *     LBFGSB_QN_IDX_MAXK, lda >= ka, any number of stored pairs: the diagonal at a list where qn_diag refuses.
 *   qn_cols: out + j*ldo receives this rank's n_local rows of column h_idx[j] of A (device memory, the context's real
 *     kind): what qn_apply gives on the unit vector, which never exists.  k <= 128, ldo >= n_local.  The gather, then
 *     one pass over W per tile of 16 pairs that writes all k outputs (2col*8 + k*8 B per row and tile in fp64).
 *   qn_shift_block, qn_shift_cols: the same for Sigma, at most LBFGSB_QN_ROOT_MAXCOL stored pairs as qn_shift_set
 *     demands.  A pinned row or column is exactly +0.  LBFGSB_E_STATE with no shift in force or after the pairs have
 *     changed ("call qn_shift_set again"), as qn_shift_solve.
 * The three host-result entries wait for their data whatever LBFGSB_F_NO_RETURN_SYNC says, as qn_quad; the two that
 * write device memory follow qn_eigvec.  LBFGSB_E_ARG, nothing changed: a NULL pointer, k < 1, k over the cap, an ld
 * that is too small, an index outside 0 .. n_global - 1, a mode that is not B or H.  When, REAL32 (W and out fp32,
 * every sum and host result fp64) and the refusals are qn_apply's, and the run does not notice the calls.
 *
 * The model over a range of shifts.  A trust-region or Levenberg-Marquardt step looks for the mu with
 * ||(B + mu I)^-1 g|| = Delta, evidence maximisation over a prior precision tau needs log det (B + tau I) at dozens of
 * tau: questions about many shifts, each of which would cost a qn_shift_set.  When the diagonal is "pins plus a scalar"
 * they cost the device nothing: with F the rows that are not pinned, R = [S, Y] and w = 1 / (theta + mu), the weighted
 * Gram of qn_shift_set is w G_F, G_F = R_F'R_F, and p = R_F'v does not depend on mu.  From one Gram and one read pass
 * per vector the host has, for x(mu) = (B_FF + mu I)^-1 v_F = w 1_F o (v + R c(mu)) and vv = sum_F v_i^2,
 *   ||x||^2 = w^2 (vv + 2 c'p + c'G_F c),   v'x = w (vv + p'c),   d||x||^2 / d mu = -2 x'(B_FF + mu I)^-1 x,
 *   log det (B_FF + mu I) = nf log(theta + mu) + log |det K(mu)| - log |det M^-1|,   K(mu) = M^-1 - w G_F in W's basis,
 * at any number of shifts.
 *   qn_path_set: status (device int8 codes as lbfgsb_hip_kkt writes them, or NULL: nothing pinned) and code_mask (bit
 *     (code + 1) selects a code to PIN, lbfgsb_hip_kkt_list's convention: 0b11100 pins the rows at a lower bound, at
 *     an upper bound or fixed) give one free / pinned byte per row in a buffer of the context; *h_pinned (may be NULL)
 *     receives the pinned rows over all ranks.  G_F is reduced by ceil(2col / 4) masked passes over W; with no pinned
 *     row it is the pairs' cached Gram and no pass is launched.  All rows pinned is legal.  At most
 *     LBFGSB_QN_ROOT_MAXCOL stored pairs (LBFGSB_E_ARG).  Independent of qn_shift_set: both may be live.
 *   qn_path_logdet: host only, any k >= 1, nothing launched.  h_info[j] = 0: h_logdet[j] = log det (B_FF + h_mu[j] I);
 *     1: theta + mu_j <= 0 or mu_j not finite; 2: K does not have the inertia (col, col) -- the shifted model is not
 *     positive definite on the free rows.  h_logdet[j] is written only where h_info[j] = 0; the call returns 0 all the
 *     same.
 *   qn_path_solve: out + j*ldo receives x(h_mu[j]), j < k <= LBFGSB_QN_PATH_MAXK, in the context's real kind and
 *     natural row order; a pinned row is +0 whatever v holds there.  h_norm2[j] = ||x_j||^2 and h_vx[j] = v'x_j by the
 *     formulas above; either may be NULL, and out may be NULL when one of them is given (the read pass alone).  out
 *     may not overlap v (the caller's responsibility, as in qn_shift_solve: not checked).  A bad mu_j is
 *     LBFGSB_E_ARG (info 1) or LBFGSB_E_STATE (info 2), the message names j, nothing is written.  One read pass over W, then one pass per tile of 16 pairs that stores all k outputs (2col*8 + 8 + 1
 *     + 8k B per row and tile in fp64).
 *   qn_path_trust: step = -(B_FF + mu I)^-1 g_F with mu >= 0, ||step|| <= delta and mu (delta - ||step||) = 0 to
 *     rtol: mu = 0 when ||x(0)|| <= delta (the Newton step of the free variables), else Newton on 1 / ||x(mu)|| -
 *     1 / delta from mu = 0 inside a bracket that bisects whenever Newton leaves it, until | ||x|| - delta | <= rtol
 *     delta or the ends of the bracket are adjacent doubles; max_it bounds the evaluations.  rtol = 0 and max_it = 0
 *     select 1e-10 and 100.  h_res = {mu, ||step||, the predicted decrease g'x / 2 + mu ||x||^2 / 2, on_boundary (0 /
 *     1)}, *h_iters the host evaluations made.  on_boundary = 1 says mu > 0, the constraint is active; ||step|| =
 *     delta then holds to rtol unless the iteration ended by max_it or by adjacent doubles, when the step is the one
 *     at the upper end of the bracket: ||step|| <= delta (1 + rtol) always, and h_res[1] says what it is.  If max_it
 *     evaluations find no shift with ||step|| <= delta at all (max_it = 1 outside the region, say) the call returns
 *     LBFGSB_E_STATE and writes nothing: never a step outside the region (to rtol).  step may be NULL (the scalars
 *     alone).  With g_F = 0 or every row pinned step is +0 and h_res = {0, 0, 0, 0}.  The read pass, plus one write pass per tile when step is given; the
 *     secular iterations launch nothing.  LBFGSB_E_ARG: delta not > 0 or not finite, rtol outside [0, 1), max_it < 0,
 *     g NULL.
 * The result of qn_path_set belongs to the pairs it was made of: after a return that changes the pairs or theta the
 * other three return LBFGSB_E_STATE ("call qn_path_set again").  Host results have the same bits on every rank.  When,
 * streams, LBFGSB_F_NO_RETURN_SYNC, the collective rule, REAL32 (v, out fp32; the bytes, every sum and every host
 * number fp64) and the refusals are qn_shift_solve's, and the run does not notice the calls.
 *
 * Pairs in and out: a curvature model of the caller's own.  The stored pairs (s_j, y_j) and theta are all that the
 * entries above read; these three move them as DEVICE data, with no run required and nothing of the reference's wa
 * through host memory.  S, Y, s, y are device memory of the context's real kind: pair j (oldest first, as qn_rows
 * orders its columns) at S + j*lds and Y + j*ldy, n_local rows each, lds, ldy >= n_local, element alignment only.  On
 * several ranks the calls are collective: every rank passes its rows, the sums are reduced as qn_apply's, the host
 * results have the same bits on every rank.  Streams as qn_apply, LBFGSB_F_NO_RETURN_SYNC included for the device
 * outputs of qn_pairs_get.
 *   qn_pairs_get: valid exactly when qn_apply is.  *h_col = the number of stored pairs, *h_theta = theta, then the
 *     pairs in ring order from the oldest into S and Y.  cap = 0 (S, Y may be NULL) is the counting call; 0 < cap <
 *     *h_col is LBFGSB_E_ARG with *h_col and *h_theta written.  W is read in the layout it is in (2col*16 B per row in
 *     fp64); the run does not notice the call.
 *   qn_pairs_set: loads 0 <= k <= m pairs.  theta > 0 and finite is taken as given; theta = 0 means y'y / s'y of the
 *     newest pair (k >= 1), as matupd sets it; anything else is LBFGSB_E_ARG.  Allowed on a context that has never
 *     run, and at any return: it ENDS the run and puts the context into model mode -- the pairs sit in the ring slots
 *     1 .. k in natural row order, nothing deferred or pending survives, and sy, ss, wt (formt) and the Gram cache of
 *     the operators are made from one Gram pass over the loaded columns, so the first operator call afterwards runs
 *     none.  k = 0 is the empty model B = theta I.  LBFGSB_E_ARG when some s_j'y_j is not finite or not positive
 *     (the message names the pair) or when formt fails: the context then holds NO model and NO run -- every qn entry
 *     returns LBFGSB_E_STATE until the next qn_pairs_set, START or import_state.
 *   qn_pairs_push: model mode only (LBFGSB_E_STATE otherwise, nothing changed: the pairs of a run belong to the run).
 *     One pass over W reads s, y and the stored columns and carries S's, S'y, Y's, Y'y, s's, s'y, y'y, in fp64 also in
 *     REAL32 contexts ((2col + 2)*8 B per row in fp64, nothing written).  The pair is stored iff s'y is finite and
 *     s'y > epsmch sqrt(s's y'y), epsmch of the context's real kind.  *h_stored = 0: not stored, nothing changed.
 *     *h_stored = 1: the two columns are written (32 B per row), a full ring drops its oldest pair, and sy, ss, theta
 *     (= y'y / s'y unless the argument is > 0), wt and the Gram cache follow on the host from the sums alone as matupd
 *     and formt do it -- no further pass over W, none at the next qn_apply either.  *h_stored = -1: formt failed and
 *     the model was refreshed as the reference refreshes (no pair, theta = 1); the return is still 0.
 * In model mode lbfgsb_hip_setulb_dev / _dev_pp (and the host forms above them) return LBFGSB_E_STATE for every task
 * but START; START and lbfgsb_hip_import_state leave the mode.
 * ------------------------------------------------------------------------- */
#define LBFGSB_QN_B 0
#define LBFGSB_QN_H 1
#define LBFGSB_QN_SQRT 4   /* qn_apply only, added to LBFGSB_QN_B / LBFGSB_QN_H: the symmetric square root */
#define LBFGSB_QN_B_SQRT (LBFGSB_QN_SQRT | LBFGSB_QN_B) /* 4: out = B^(1/2) v */
#define LBFGSB_QN_H_SQRT (LBFGSB_QN_SQRT | LBFGSB_QN_H) /* 5: out = H^(1/2) v */
#define LBFGSB_QN_ROOT_MAXCOL 64
#define LBFGSB_QN_GRAM_MAXK 64
int lbfgsb_hip_qn_apply(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const void *v, int64_t ldv, void *out,
                        int64_t ldo);
int lbfgsb_hip_qn_diag(lbfgsb_hip_ctx *ctx, int mode, void *out);
int lbfgsb_hip_qn_logdet(lbfgsb_hip_ctx *ctx, int mode, double *h_logdet);
int lbfgsb_hip_qn_draw(lbfgsb_hip_ctx *ctx, int mode, int64_t k, uint64_t seed, int64_t first, const void *mean,
                       double scale, void *out, int64_t ldo);
int lbfgsb_hip_qn_quad(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const void *v, int64_t ldv, const void *center,
                       double *h_q);
int lbfgsb_hip_qn_logpdf(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const void *x, int64_t ldx, const void *mean,
                         double scale, double *h_logp);
int lbfgsb_hip_qn_draw_logpdf(lbfgsb_hip_ctx *ctx, int mode, int64_t k, uint64_t seed, int64_t first,
                              const void *mean, double scale, void *out, int64_t ldo, double *h_logp);
int lbfgsb_hip_qn_gram(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const void *v, int64_t ldv, const void *center,
                       double *h_g, int64_t ldg);
#define LBFGSB_QN_EIG_CUT 1e-8
int lbfgsb_hip_qn_eig(lbfgsb_hip_ctx *ctx, int mode, int32_t cap, int32_t *h_r, double *h_bulk, double *h_lambda);
int lbfgsb_hip_qn_eigvec(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const int32_t *h_which, void *out, int64_t ldo);
int lbfgsb_hip_qn_shift_set(lbfgsb_hip_ctx *ctx, const void *d, double mu, int64_t *h_pinned);
int lbfgsb_hip_qn_shift_solve(lbfgsb_hip_ctx *ctx, int64_t k, const void *v, int64_t ldv, void *out, int64_t ldo);
int lbfgsb_hip_qn_shift_logdet(lbfgsb_hip_ctx *ctx, double *h_logdet);
int lbfgsb_hip_qn_shift_diag(lbfgsb_hip_ctx *ctx, void *out);
int lbfgsb_hip_qn_shift_sqrt(lbfgsb_hip_ctx *ctx, int64_t k, const void *v, int64_t ldv, void *out, int64_t ldo);
int lbfgsb_hip_qn_shift_draw(lbfgsb_hip_ctx *ctx, int64_t k, uint64_t seed, int64_t first, const void *mean,
                             double scale, void *out, int64_t ldo);
int lbfgsb_hip_qn_shift_draw_logpdf(lbfgsb_hip_ctx *ctx, int64_t k, uint64_t seed, int64_t first, const void *mean,
                                    double scale, void *out, int64_t ldo, double *h_logp);
int lbfgsb_hip_qn_shift_quad(lbfgsb_hip_ctx *ctx, int64_t k, const void *v, int64_t ldv, const void *center,
                             double *h_q);
int lbfgsb_hip_qn_shift_logpdf(lbfgsb_hip_ctx *ctx, int64_t k, const void *x, int64_t ldx, const void *mean,
                               double scale, double *h_logp);
#define LBFGSB_QN_IDX_MAXK 4096
int lbfgsb_hip_qn_rows(lbfgsb_hip_ctx *ctx, int64_t k, const int64_t *h_idx, double *h_rows, int64_t ldr);
int lbfgsb_hip_qn_block(lbfgsb_hip_ctx *ctx, int mode, int64_t ka, const int64_t *h_ia, int64_t kb,
                        const int64_t *h_ib, double *h_a, int64_t lda);
int lbfgsb_hip_qn_cols(lbfgsb_hip_ctx *ctx, int mode, int64_t k, const int64_t *h_idx, void *out, int64_t ldo);
int lbfgsb_hip_qn_shift_block(lbfgsb_hip_ctx *ctx, int64_t ka, const int64_t *h_ia, int64_t kb, const int64_t *h_ib,
                              double *h_a, int64_t lda);
int lbfgsb_hip_qn_shift_cols(lbfgsb_hip_ctx *ctx, int64_t k, const int64_t *h_idx, void *out, int64_t ldo);
#define LBFGSB_QN_PATH_MAXK 64
int lbfgsb_hip_qn_path_set(lbfgsb_hip_ctx *ctx, const int8_t *status, int code_mask, int64_t *h_pinned);
int lbfgsb_hip_qn_path_logdet(lbfgsb_hip_ctx *ctx, int64_t k, const double *h_mu, double *h_logdet, int32_t *h_info);
int lbfgsb_hip_qn_path_solve(lbfgsb_hip_ctx *ctx, const void *v, int64_t k, const double *h_mu, void *out,
                             int64_t ldo, double *h_norm2, double *h_vx);
int lbfgsb_hip_qn_path_trust(lbfgsb_hip_ctx *ctx, const void *g, double delta, double rtol, int max_it, void *step,
                             double *h_res /*[4]*/, int32_t *h_iters);
int lbfgsb_hip_qn_pairs_get(lbfgsb_hip_ctx *ctx, int32_t cap, int32_t *h_col, double *h_theta, void *S, int64_t lds,
                            void *Y, int64_t ldy);
int lbfgsb_hip_qn_pairs_set(lbfgsb_hip_ctx *ctx, int32_t k, const void *S, int64_t lds, const void *Y, int64_t ldy,
                            double theta);
int lbfgsb_hip_qn_pairs_push(lbfgsb_hip_ctx *ctx, const void *s, const void *y, double theta, int32_t *h_stored);

/* -------------------------------------------------------------------------
 * The active set, the bound multipliers and the projected gradient as device data.
 * lbfgsb_hip_kkt is ONE pass over the caller's x, l, u, nbd, g (device pointers to this rank's n_local rows, of the
 * context's real kind; 36 bytes per row in fp64) -- the arrays handed in, not the context's snapshot of the bounds.
 * It needs no run on the context: only its stream, real kind, communicator and row0.  Per row i, in this order of
 * precedence (the order of `active`, src/lbfgsb.f90:994-1028; codes as iwhere's, :348-355):
 *   status  -1  nbd == 0 (unbounded)
 *            3  nbd == 2 and u - l <= 0 (always fixed)
 *            1  the row has a lower bound (nbd 1 or 2) and x <= l
 *            2  the row has an upper bound (nbd 2 or 3) and x >= u
 *            0  otherwise (free, bounded)
 *   pg      the signed projected gradient: gi of projgr (:2610-2618) before the abs, by the device function
 *           lbfgsb_hip_projgr's kernel uses.  REAL32: operands widened to double as there, the result rounded to fp32
 *           on store.
 *   mult    the signed bound multiplier (reduced cost): g on a status-3 row, g on a status-1 row when g > 0 (the
 *           bound holds the row from below), g on a status-2 row when g < 0, +0 everywhere else.  A nonzero entry is
 *           an exact copy of g.
 * A bound that nbd says does not exist is never looked at (NaN in an unused l or u changes nothing).
 * pg_out, mult_out (reals of the context's kind) and status_out (one byte per row) may each be NULL: that output is
 * then neither computed into memory nor addressed.
 * The summary is complete over all ranks and identical on each:
 *   h_cnt[LBFGSB_KKT_N_UNBOUNDED .. LBFGSB_KKT_N_FIXED]  rows of status -1, 0, 1, 2, 3 (index = code + 1)
 *   h_cnt[LBFGSB_KKT_N_BINDING]  status 1 with g > 0, or status 2 with g < 0
 *   h_cnt[LBFGSB_KKT_N_WEAK]     status 1 or 2 and |g| <= tol (degenerate: active only weakly)
 *   h_cnt[LBFGSB_KKT_N_LEAVING]  status 1 with g < -tol, or status 2 with g > tol (at a bound and wants to leave it)
 *   h_cnt[LBFGSB_KKT_N_OUTSIDE]  the row has the bound and x < l or x > u strictly (a line-search step can leave the
 *                                iterate an ulp outside the box)
 *   h_val[LBFGSB_KKT_PG_MAX]     max |pg|: bit for bit what lbfgsb_hip_projgr returns on the same arrays, hence
 *                                dsave(13) at a NEW_X or convergence return
 *   h_val[LBFGSB_KKT_MULT_MAX]   max |mult|
 *   h_val[LBFGSB_KKT_OUT_MAX]    the largest distance outside the box, max(l - x, x - u) over the bounds a row has
 *                                (0 if no row is outside)
 *   h_val[LBFGSB_KKT_GFREE_MAX]  max |g| over the rows of status -1 and 0
 *
 * lbfgsb_hip_kkt_list writes the GLOBAL 0-based indices (row0 + i) of this rank's rows whose status byte is selected,
 * in ascending order, as device int64: bit (code + 1) of code_mask selects a code (0b01100: the rows at a lower or an
 * upper bound; 0b00011: the free rows).  status is any device int8 array of n_local codes -1 .. 3 (other values
 * select nothing); it need not come from lbfgsb_hip_kkt.  At most cap indices are written and nothing behind them is
 * touched; *h_count is this rank's full count even when it exceeds cap (cap = 0 with idx_out = NULL: the counting
 * call).  The order is deterministic: a stable compaction, no atomic hands out positions.  Per rank, not collective.
 *
 * Both are valid whenever no deferred line-search set-up is live and no built-in objective's value is still on the
 * device: LBFGSB_E_STATE then, changing nothing.  LBFGSB_E_ARG: a NULL input or summary, tol negative or NaN,
 * code_mask outside 0 .. 31, cap < 0, cap > 0 without idx_out.
 * Calling them changes nothing a run computes: every return is bit-identical with or without the calls.
 * Streams: as lbfgsb_hip_qn_apply -- the inputs are read on the context's stream; the summaries are host data, so the
 * calls wait for that stream and the device outputs are complete at return.  Several ranks: lbfgsb_hip_kkt is called
 * collectively, each rank with its own rows; the summary is reduced as the iteration's sums are (rank order / the
 * host reducer).
 * ------------------------------------------------------------------------- */
#define LBFGSB_KKT_N_UNBOUNDED 0 /* h_cnt: status -1 */
#define LBFGSB_KKT_N_FREE 1      /*        status  0 */
#define LBFGSB_KKT_N_LOWER 2     /*        status  1 */
#define LBFGSB_KKT_N_UPPER 3     /*        status  2 */
#define LBFGSB_KKT_N_FIXED 4     /*        status  3 */
#define LBFGSB_KKT_N_BINDING 5
#define LBFGSB_KKT_N_WEAK 6
#define LBFGSB_KKT_N_LEAVING 7
#define LBFGSB_KKT_N_OUTSIDE 8
#define LBFGSB_KKT_NCNT 9
#define LBFGSB_KKT_PG_MAX 0 /* h_val */
#define LBFGSB_KKT_MULT_MAX 1
#define LBFGSB_KKT_OUT_MAX 2
#define LBFGSB_KKT_GFREE_MAX 3
#define LBFGSB_KKT_NVAL 4
int lbfgsb_hip_kkt(lbfgsb_hip_ctx *ctx, const void *x, const void *l, const void *u, const int32_t *nbd,
                   const void *g, double tol, void *pg_out, void *mult_out, int8_t *status_out, int64_t *h_cnt,
                   double *h_val);
int lbfgsb_hip_kkt_list(lbfgsb_hip_ctx *ctx, const int8_t *status, int code_mask, int64_t *idx_out, int64_t cap,
                        int64_t *h_count);

/* -------------------------------------------------------------------------
 * Per-kernel entry points (one per row of SURVEY.md 8a), for parity tests
 * and profiling.  All pointers are DEVICE pointers unless named h_*.
 * Reduction results come back in host doubles, already complete across
 * ranks.  Each returns LBFGSB_OK or an error code.
 * ------------------------------------------------------------------------- */

/* projgr, src/lbfgsb.f90:2594-2622 */
int lbfgsb_hip_projgr(lbfgsb_hip_ctx *ctx, const void *x, const void *l, const void *u,
                      const int32_t *nbd, const void *g, double *h_sbgnrm);

/* W'v : out[j] = sum_i Wy(i,col_j) v_i (j < col), out[col+j] = sum_i Ws(i,col_j) v_i,
 * logical column order (head .. head+col-1 mod m).  The WS/WY correction-pair
 * matvec of matupd (:2333-2338), cauchy (:1300-1304) and subsm (:2742-2754).
 * Works on the context's own Ws/Wy. */
int lbfgsb_hip_wtv(lbfgsb_hip_ctx *ctx, const void *v, int col, int head, double *h_out);

/* load host column-major W (n x m each, leading dimension n) into the context */
int lbfgsb_hip_set_w(lbfgsb_hip_ctx *ctx, const void *h_ws, const void *h_wy);

/* formk's inner products from scratch (src/lbfgsb.f90:1756-1851): one masked Gram pass over W
 * with the context's current iwhere (free = iwhere <= 0).  h_out receives 2 col^2 + col sums:
 *   [i(i+1)/2 + j]        i >= j : sum_free Wy_i Wy_j
 *   [T + i(i+1)/2 + j]    i >= j : sum_act  Ws_i Ws_j          (T = col (col+1) / 2)
 *   [2T + i col + j]      all    : sum over (i > j ? active : free) rows of Ws_i Wy_j
 * lbfgsb_hip_set_iwhere loads iwhere (host int32[n_local], the reference's values). */
int lbfgsb_hip_set_iwhere(lbfgsb_hip_ctx *ctx, const int32_t *h_iwhere);
int lbfgsb_hip_formk_gram(lbfgsb_hip_ctx *ctx, int col, int head, double *h_out);

/* -------------------------------------------------------------------------
 * Routine doors: ONE routine of the reference each, on the STATE of the
 * context -- Ws, Wy, Sy, Ss, Wt, WN, WN1 (snd), z, r, d, t, xp, the 8m work vectors, iwhere,
 * Index, Indx2: what lbfgsb_hip_import_state loads and lbfgsb_hip_export_state reads back, in the
 * reference's wa / iwa layout.  A parity test loads the inputs of a routine with import_state,
 * calls the door, and compares export_state (and the door's scalar results) with the CPU twin
 * run on the same arrays (tests/test_gpu_routines.py).  x, l, u, nbd, g and every *_out / *_in
 * vector are DEVICE pointers of n values; everything else is host memory.  Single-rank
 * contexts; every door ends with the stream synchronised.  The doors drive the library's own
 * code (cauchy is the function the iteration calls; freev and matupd share their halves with
 * the iteration; cmprlb, subsm and matupd's n-length sums run through the unfused tile functions
 * that carry m > 32, valid for every m); the fused passes of the hot path are covered call by
 * call by the one-step parity tests.
 * ------------------------------------------------------------------------- */

/* The reference's n-length level-1 BLAS call sites (src/lbfgsb_blas_module.F90:37-277: dcopy / dscal /
 * daxpy / ddot as called from mainlb, lnsrlb, matupd) are terms of the fused passes inside an iteration;
 * the three primitives SURVEY.md 8(b)(4) names have doors of their own all the same.  Device vectors of
 * n_local values of the context's real kind, on the context's stream; no state of the context is read
 * or changed, any number of ranks.
 *   vec_sub    out = a - b            (src/lbfgsb.f90:720-722 d = z - x, :812-816 y = g - r); out may be a or b
 *   vec_scale  v = alpha v            (dscal, :822 s = stp d); alpha is rounded to the context's kind first
 *   dot        *h_result = a'b        (ddot, :816 / :2196 / :2244 / :2335) accumulated in fp64 in the library's
 *              fixed order -- not the reference's groups of five (src/lbfgsb_blas_module.F90:187-202): equal
 *              to it within rounding -- and summed over all ranks of the context (one all-gather, a host
 *              sync); the other two return with the stream synchronised */
int lbfgsb_hip_vec_sub(lbfgsb_hip_ctx *ctx, const void *a, const void *b, void *out);
int lbfgsb_hip_vec_scale(lbfgsb_hip_ctx *ctx, double alpha, void *v);
int lbfgsb_hip_dot(lbfgsb_hip_ctx *ctx, const void *a, const void *b, double *h_result);

/* active, src/lbfgsb.f90:965-1040: x projected onto the box IN PLACE, iwhere initialised;
 * h_flags[0..2] = prjctd, cnstnd, boxed */
int lbfgsb_hip_active(lbfgsb_hip_ctx *ctx, void *x, const void *l, const void *u, const int32_t *nbd,
                      int32_t *h_flags);
/* errclb, :1601-1643: task (60 chars) is left alone if the input is valid, else 'ERROR: ...',
 * *h_info = -6 / -7 and *h_k = the 1-based index the reference would report */
int lbfgsb_hip_errclb(lbfgsb_hip_ctx *ctx, const void *l, const void *u, const int32_t *nbd, double factr,
                      char *task, int32_t *h_info, int64_t *h_k);
/* cauchy, :1157-1532: reads W, Sy, Wt, iwhere; leaves the Cauchy point in z (and in xcp_out if not
 * NULL), iwhere, p / c / wbp / v in the work vectors (wa8m(1:8m) of export_state), *h_nseg, *h_info */
int lbfgsb_hip_cauchy(lbfgsb_hip_ctx *ctx, const void *x, const void *l, const void *u, const int32_t *nbd,
                      const void *g, double theta, int col, int head, double sbgnrm, void *xcp_out,
                      int32_t *h_nseg, int32_t *h_info);
/* freev, :1980-2059: from iwhere and the previous free set (Index(1:nfree) of the imported state);
 * Index / Indx2 are rebuilt in contexts created with LBFGSB_F_MIRROR_INDEX */
int lbfgsb_hip_freev(lbfgsb_hip_ctx *ctx, int iter, int cnstnd, int updatd, int64_t *h_nfree,
                     int64_t *h_nenter, int64_t *h_ileave, int32_t *h_wrk);
/* formk, :1681-1908: WN1's inner products FROM SCRATCH over the free / active rows of iwhere (the
 * reference keeps them incrementally: the same sums in another order), WN assembled and factorised
 * on the host; *h_info = 0, -1 or -2 */
int lbfgsb_hip_formk(lbfgsb_hip_ctx *ctx, int col, int head, double theta, int32_t *h_info);
/* cmprlb, :1548-1586: r = -Z'(B(xcp - x) + g) from z (= xcp), W, Sy, Wt, c (work vector 2), iwhere;
 * r_out: r scattered to its rows, 0 on the rows that are not free (the reference packs r by Index) */
int lbfgsb_hip_cmprlb(lbfgsb_hip_ctx *ctx, const void *x, const void *g, double theta, int col, int head,
                      int cnstnd, void *r_out, int32_t *h_info);
/* subsm, :2676-2885: r_in as lbfgsb_hip_cmprlb writes it, WN of the state, z = xcp in;
 * z = the subspace minimiser out (and xhat_out if not NULL), xp = xcp, *h_iword, *h_info */
int lbfgsb_hip_subsm(lbfgsb_hip_ctx *ctx, const void *x, const void *l, const void *u, const int32_t *nbd,
                     const void *g, const void *r_in, double theta, int col, int head, void *xhat_out,
                     int32_t *h_iword, int32_t *h_info);
/* lnsrlb, :2174-2275, with mainlb's d = z - x (:720-722) on the first call of an iteration's search.
 * h_sc[8] = fold, gd, gdold, stp, dnorm, dtd, xstep, stpmx; h_ic[7] = iter, ifun, iback, nfgv, info,
 * boxed, cnstnd; task, csave (60 chars), h_isave2[2], h_dsave13[13] as the reference's.  z, d, t, r are
 * the state's; x receives the trial point. */
int lbfgsb_hip_lnsrlb(lbfgsb_hip_ctx *ctx, void *x, const void *l, const void *u, const int32_t *nbd,
                      const void *g, double f, double *h_sc, int32_t *h_ic, char *task, char *csave,
                      int32_t *h_isave2, double *h_dsave13);
/* mainlb :812-824 + matupd, :2291-2346: y = g - r, s = stp d stored in W; Sy, Ss updated.
 * h_ip[4] = iupdat (already counted up, :836), col, head, itail in / out; *h_theta = y'y / dr */
int lbfgsb_hip_matupd(lbfgsb_hip_ctx *ctx, const void *g, double stp, double dr, double dtd, int32_t *h_ip,
                      double *h_theta);

int lbfgsb_hip_sync(lbfgsb_hip_ctx *ctx);

/* built-in device objectives: evaluate f, g on the
 * context's stream.  kind 0 = separable bounded quadratic,
 * kind 1 = extended Rosenbrock (test/driver1.f90:274-289; sharded: the 1-element halo x(row0-1), x(row0+n) is all-gathered through the communicator).
 * *h_f receives the GLOBAL value (reduced over ranks).  h_f == NULL defers it: the value stays
 * on the device and the NEXT lbfgsb_hip_setulb_dev call on this context -- which must be the
 * 'FG...' re-entry for this evaluation -- brings it over with the sums of its own first pass
 * (one host sync and one all-reduce less per evaluation) and stores it through its f argument. */
int lbfgsb_hip_objective(lbfgsb_hip_ctx *ctx, int kind, const void *x, void *g, double *h_f);

/* Per-context options for measurements and tests (A/B timings of fallback paths, forcing rarely
 * taken routes).  Nothing in the library reads tuning switches from the environment: a context
 * behaves as created unless this is called.  Names (value):
 *   "two_pass" (0/1)        the two-pass iteration with W'Z r in closed form; 0 = always the
 *                           cmprlb_wtv pass (three passes over W)
 *   "two_pass_maxcol" (0..32)  largest col that takes the two-pass iteration (default 32; beyond 21 pairs the update
 *                           pass runs as two launches over half of the columns each; 20 = three passes there)
 *   "lean" (0/1)            z and d = x - t left implicit by the storing pass
 *   "spec_capture" (0/1)    the update pass hands the next walk's first breakpoints over
 *                           (not where one launch cannot for ALL rows: > 10 old pairs; "compact_w", > 5, n % 128 != 0)
 *   "pg_min" (count)        LBFGSB_F_PARALLEL_GCP: walks with more breakpoints in reach than this
 *                           go to the sort + scans
 *   "exact_always" (0/1)    every Cauchy walk in the reference's heap order from its start (tests)
 *   "defer_lnsrch" (0/1)    LBFGSB_F_DEFER_LNSRCH switched on / off for the iterations that follow (the
 *                           caller must honour that flag's contract)
 *   "spin" (0/1)            results of a phase reach the host through mapped memory + a polled sequence
 *                           word (default) / through a D2H copy + hipStreamSynchronize
 *   "fold_finalize" (0/1)   reductions nobody waits for yet (a deferred f, a deferred set-up) leave their
 *                           finalize to the next launch (default 1)
 *   "eager_patch" (0/1)     formk's patch sums are queued behind freev's counting pass and fetched with its
 *                           counts (default 1) / after a host round trip of their own
 *   "spec_freev" (0/1)      while the free set changes from iteration to iteration, freev's counting pass and
 *                           the patch are queued speculatively behind the evaluation of a trial point and
 *                           used if the point is accepted and the next walk fixes no row (default 0: measured,
 *                           does not pay)
 *   "skip_reuse" (0/1)      after a skipped BFGS update, cauchy's n-loop sums come from the pass that evaluated
 *                           the accepted point (+ a one-column scan when the memory is full) (default 1) /
 *                           from a scan over all of W
 *   "wide_fused" (0/1)      m > 32: matupd's, cauchy's and formk's sums from the update pass (split over the columns,
 *                           one pass over W) in front of the unfused subspace steps (default 1) / all unfused
 *   "wide_closed" (0/1)     m > 32: W'Z r in closed form and cmprlb's + subsm's updates of r as one pass over W
 *                           (default 1) / a W'r pass and two updates
 *   "wide_tail" (0/1)       m > 32: cmprlb's start and subsm's projected step + the line-search set-up folded into the first /
 *                           last tile of that pass (default 1) / as kernels of their own
 *   "win_slack" (>= 0)      the first window of a breakpoint walk asks (1 + win_slack) x as far ahead as the walk needs
 *                           when it starts (default 0.25; 0: exactly as far -- a second window pass usually follows)
 *   "spec_trial2" (0/1)     the SECOND trial point of a line search (an interpolated step after a rejected first one) is
 *                           evaluated by the update pass too, whose sums serve the NEW_X entry if it is accepted
 *                           (default 1) / by the two-sum evaluation kernel, the update pass follows at NEW_X
 *   "wide_one" (0/1)        m > 32, col <= 96: that pass as ONE launch over all columns, the pending pair committed by
 *                           it (default 1) / one launch per tile of 32 columns behind pair_commit
 *   "wide_incr" (0/1)       m > 32: formk adds the new pair's row and column to WN1 while no row changes status
 *                           (default 1) / from scratch whenever it runs
 *   "nt" (0/1)              nontemporal loads in the passes over W (default: by the size of W)
 *   "cw_dense" (0/1)        "compact_w": the storing pass and the lane-pair update pass (m = 10, > 5 pairs) fetch a
 *                           tile's run of layout-free entries of each stored column by 16-byte loads and hand them to
 *                           the lanes that own the rows through LDS (default 1) / two 8-byte loads per column in which
 *                           every lane takes part: the same values, the same sums, bit for bit
 *   "cw_ub" (0/1)           "cw_dense", all three bound arrays uniform (lbfgsb_hip_uniform_bounds: mask 7, no dictionary),
 *                           m = 10 with the memory full: the lane-pair update pass reads l, u and nbd once per workgroup
 *                           from the 64-byte buffers (default 1) / every row loads them, three loads of one address per
 *                           trip: the same values, every result bit for bit (lbfgsb_hip_ub_launches counts the former)
 *   "qn_basis" (0/1)       qn_eigvec writes all its vectors in one pass over W per tile of 16 pairs (default 1) / goes
 *                           through qn_apply's expansion, 4 vectors a pass: the same products summed in another order
 *   "uniform_bounds" (0/1)  detect bound arrays that hold one value each (lbfgsb_hip_uniform_bounds)
 *   "dict_bounds" (0/1)     dictionary-code bound arrays with <= 8 distinct values each (same place; default 1)
 *   "bounds_check" (0..)    compare the caller's l, u, nbd with the context's snapshot after the first iteration and
 *                           then every k-th (default 32; 0 = never): 'ERROR: BOUNDS CHANGED DURING RUN'
 *   "wgrid" (0..2047)       workgroups of the passes over W (default 0: what is resident for the kernel
 *                           launched, 256 ... 768)
 *   "pipe" (-1/0/1)         two trips of loads in flight per wave: default rule (m = 20, fp32 m = 10) / off /
 *                           the default rule again (the other shapes are not compiled with it)
 *   "pair" (0/1/2)          MC = 20 update pass: lane pairs share accumulators (off / 1 trip / 2 trips)
 *   "split" (10/20)         update pass with formk's new-row sums: split over the columns beyond 20 old pairs into
 *                           parts of <= 16 (default) / beyond 10 into parts of <= 10 (measurement: slower at m = 20)
 *   "gram_rows" (0/1)       formk from scratch with the LDS-slab kernel instead of the quad kernel
 * Returns LBFGSB_E_ARG for an unknown name or a value out of range. */
int lbfgsb_hip_set_option(lbfgsb_hip_ctx *ctx, const char *name, double value);

/* Uniform and few-valued bounds.  Bound arrays that hold ONE value each -- the box [a, b]^n, x >= 0 -- are the
 * common case, and on a bandwidth-bound device streaming 2 x 8 + 1 constant bytes per row through each of the
 * two passes over W of an iteration is 8 % of its traffic.  At task 'START' the pass that validates the bounds
 * (errclb, src/lbfgsb.f90:1601-1643) also checks, bit for bit, whether every l_i equals l_1, every u_i equals
 * u_1, every nbd_i equals nbd_1 (among this rank's rows); the passes over W then read the value from a 64-byte
 * buffer instead of the array -- same arithmetic, same results bit for bit.
 * Arrays with a FEW distinct values -- the reference's own test box, l alternating 1 / -100 with u = 100
 * (test/driver3.f90:102-120); a box with some variables on another box -- are dictionary-coded: if l and u hold
 * at most 8 distinct values each (bit patterns; found by a few probing passes at START, identical on all ranks),
 * the one-byte copy of nbd the passes stream anyway carries  nbd | l-index << 2 | u-index << 5  and the values
 * come from two 8-entry tables held in LDS: 1 byte per row instead of 17.  Same values, same arithmetic.
 * *mask: bit 0 = l, bit 1 = u, bit 2 = nbd is treated as uniform in the current run; bit 3 (with bits 0 and 1):
 * l and u are dictionary-coded.  Passing OTHER array pointers than at 'START' switches the corresponding bits
 * off (any of the three for the dictionary).  Options "uniform_bounds" = 0 / "dict_bounds" = 0
 * (lbfgsb_hip_set_option, before START) disable the detection / the dictionary. */
int lbfgsb_hip_uniform_bounds(lbfgsb_hip_ctx *ctx, int32_t *mask);

/* Announce an edit of l, u or nbd made since the last call (with or without LBFGSB_F_FOLLOW_BOUNDS): the next
 * entry rebuilds the snapshot without comparing, and continues as LBFGSB_F_FOLLOW_BOUNDS does on a difference.
 * Costs nothing unless it is called.  Sharded runs without the flag: every rank announces, before the same call
 * (with the flag an announcement on some ranks is enough: it rides in the reduced count).  Refused
 * (LBFGSB_E_STATE) at an 'FG_LNSRCH' return whose line-search set-up is deferred (LBFGSB_F_DEFER_LNSRCH): that
 * set-up would meet the new bounds where the reference used the old ones; edit at a 'NEW_X' return instead.
 * Without the flag an edit that is NOT announced is still reported by the "bounds_check" comparison. */
int lbfgsb_hip_bounds_changed(lbfgsb_hip_ctx *ctx);

/* Profiling clocks, counters and bare-kernel timing doors (bench.py, profiles/scripts, tests) are declared in
 * lbfgsb_hip_debug.h: measurement instruments of the same library, not part of the drop-in surface. */

#ifdef __cplusplus
}
#endif
#endif
