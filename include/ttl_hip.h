/*
 * ttl_hip.h -- C ABI of libttl_hip.so: the MI355X (gfx950) tractography
 * environment step.
 *
 * The reference (levje/TrackToLearn @ 2024-10-24) is pure Python and has no
 * FFI layer; the drop-in boundary is the Python class surface of
 * TrackToLearn/environments/{env,tracking_env,noisy_tracking_env}.py.  The
 * Python host classes in tracktolearn_amd/environments keep that surface and
 * bind the entry points below through ctypes (INTEGRATION.md shows the stub).
 * Each entry point cites the reference code it replaces (paths relative to the
 * reference root, TTL = TrackToLearn).
 *
 * Conventions
 *   - plain C: pointers, sizes, no C++/torch types; return 0 on success, a
 *     negative TTL_ERR_* otherwise, message via ttl_last_error() (thread
 *     local).  Nothing throws or aborts across the ABI.
 *   - every device pointer is BORROWED: the caller (torch, or any hipMalloc
 *     owner) allocates and outlives the handle.  The library allocates no
 *     device memory.
 *   - every call is asynchronous on the caller's HIP stream (`hip_stream` is
 *     a hipStream_t, NULL = default stream).  The only host-visible outputs
 *     are the 4-byte counters written through `host_counts` (pinned memory
 *     supplied by the caller), valid after the stream is synchronised.
 *   - one host thread per handle; handles share nothing.
 */
#ifndef TTL_HIP_H
#define TTL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: only the entry points marked
 * TTL_API below are exported (nm -D shows exactly these). */
#if defined(__GNUC__) || defined(__clang__)
#define TTL_API __attribute__((visibility("default")))
#else
#define TTL_API
#endif

#define TTL_ABI_VERSION 13

#define TTL_OK 0
#define TTL_ERR_INVALID (-1) /* bad argument / shape / alignment             */
#define TTL_ERR_HIP (-2)     /* a HIP runtime call failed                    */
#define TTL_ERR_STATE (-3)   /* call order violated (e.g. step before reset) */
#define TTL_ERR_UNSUPPORTED (-4) /* the configuration has no such path (free-running steps) */

/* Direction arithmetic, TTL/environments/env.py:493-502:
 *   F32      normalise, scale and add in float32 (training env, float32
 *            affine; also any affine under numpy 1.x).
 *   F64DIR   NoisyTrackingEnvironment (noisy_tracking_env.py:65-77): float64
 *            noise is added first, so normalise/scale/add run in float64 and
 *            the new point is float32(float64(p) + d).
 *   F32NORM  float32 normalise, float64 scale/add: what numpy >= 2 computes
 *            for the plain TrackingEnvironment when step_size is np.float64
 *            (float64 affine). */
#define TTL_MODE_F32 0
#define TTL_MODE_F64DIR 1
#define TTL_MODE_F32NORM 2

/* StoppingFlags, TTL/environments/stopping_criteria.py:10-20 */
#define TTL_FLAG_MASK 1
#define TTL_FLAG_LENGTH 2
#define TTL_FLAG_CURVATURE 4
#define TTL_FLAG_ORACLE 64

/* Row order of the state rows written by ttl_env_step():
 *   ORDER_ACTIVE    row i of the output = i-th active streamline (the order
 *                   of continue_idx), exactly tracking_env.py:214-221.
 *   ORDER_PARTITION survivors first (stable), then the streamlines that just
 *                   stopped (stable): rows [0, n_continue) are already the
 *                   harvest() result, so harvest copies nothing.  row_dest[i]
 *                   maps active row i to its output row. */
#define TTL_ORDER_ACTIVE 0
#define TTL_ORDER_PARTITION 1

typedef struct ttl_env_desc {
    uint32_t abi_version;  /* TTL_ABI_VERSION */
    int32_t mode;          /* TTL_MODE_*      */

    /* SH volume, packed by ttl_pack_sh_volume(): voxel records of coef_pitch
     * f32, in the order sh_layout says */
    int32_t sh_dim[3];
    int32_t n_coef;        /* C (45 for SH order 8)                          */
    int32_t coef_pitch;    /* floats per voxel record, multiple of 4, >= C   */
    const float *sh_packed;
    float sh_coord_shift;  /* added to coordinates before the gather; 0.0    */
                           /* (voxel i sits at coordinate i)  */
    int32_t sh_layout;     /* TTL_SH_LINEAR or TTL_SH_BRICK4                 */

    /* tracking mask: cubic B-spline coefficients, [X][Y][Z] f64
     * (scipy.ndimage.spline_filter(order=3), stopping_criteria.py:58-59)    */
    int32_t mask_dim[3];
    const double *mask_coef;
    double mask_threshold; /* env_dto['binary_stopping_threshold']           */
    /* optional [X][Y][Z] u8 from ttl_mask_classes(mask_coef, mask_dim,
     * mask_threshold): cells where the spline cannot cross the threshold are
     * decided without evaluating it (same decisions, bit for bit); or NULL  */
    const uint8_t *mask_classes;

    /* fODF peaks for the alignment reward: [X][Y][Z][15] f32, or NULL       */
    int32_t peaks_dim[3];
    const float *peaks;
    int32_t compute_reward;
    double alignment_weighting;

    /* tracking parameters (env.py:196-213) */
    int32_t n_dirs;        /* K previous directions in the state             */
    int32_t max_nb_steps;  /* int(max_length / step_size_mm)                 */
    double step_size_vox;  /* convert_length_mm2vox(step_size_mm, affine)    */
    float neigh_radius_vox;/* neighbourhood radius (float32, env.py:207-213) */
    int32_t curvature_enabled;
    float curv_dot_max;    /* too curvy  <=>  -1 <= dot <= curv_dot_max; the
                              host derives it from numpy's own float32 arccos
                              (utils.py:172-173), see curvature_threshold()  */

    /* per-streamline state, capacity n_max rows (tracking_env.py:110-124)   */
    int32_t n_max;
    float *streamlines;    /* [n_max][max_nb_steps+1][3] f32                 */
    int32_t *flags;        /* [n_max] StoppingFlags bitmask                  */
    int32_t *lengths;      /* [n_max]                                        */
    uint8_t *dones;        /* [n_max]                                        */
    int32_t *idx_a;        /* [n_max] continue_idx, double buffered          */
    int32_t *idx_b;        /* [n_max]                                        */
    void *workspace;       /* ttl_env_workspace_bytes(n_max) bytes           */
    size_t workspace_bytes;
} ttl_env_desc;

typedef struct ttl_env ttl_env;

/* Bytes of device scratch the handle needs for n_max streamlines. */
TTL_API size_t ttl_env_workspace_bytes(int32_t n_max);

/* Order of the packed voxel records:
 *   TTL_SH_LINEAR  [X][Y][Z] as the source volume;
 *   TTL_SH_BRICK4  4x4x4-voxel bricks, each 64 consecutive records
 *                  ([X/4][Y/4][Z/4] bricks, [4][4][4] voxels inside; dims
 *                  rounded up to multiples of 4, padding records zero): the
 *                  4x4x4 neighbourhood one streamline gathers then lives in
 *                  at most 8 contiguous 64-record runs instead of 16 runs of
 *                  4 records spread over Y*Z- and Z-record strides. */
#define TTL_SH_LINEAR 0
#define TTL_SH_BRICK4 1

/* Number of voxel records ttl_pack_sh_volume() writes for a volume. */
TTL_API int64_t ttl_sh_volume_records(const int32_t *dim /*[3]*/, int32_t layout);

/* Device memory for a volume the step gathers from (the packed SH volume):
 * try_contiguous 0: plain hipMalloc; 1: physically contiguous
 * (hipExtMallocWithFlags, hipDeviceMallocContiguous) when the driver grants it;
 * 2: through the virtual-memory API (hipMemCreate + hipMemMap at the
 * recommended granularity), hipMalloc when that fails; *contiguous_out says
 * which was granted (measurement showed no kind to be better placed than
 * another; the host classes use 0).  device < 0: the calling thread's
 * current device.  These two entry points are the only ones that own device
 * memory; everything else is borrowed.  They exist because WHERE the 170 MB
 * volume of the bench lands in physical memory moves the state gather between
 * 0.18 and 0.20 ms on the same GPU, and so does where the state rows land
 * (DESIGN.md 3.3): the host classes put a subject's volume and a ring of state
 * buffers into a few allocations obtained here, time the step's own gather on
 * every pair at the first large reset and keep the fastest; the caching
 * allocator would hand the same block back every time. */
TTL_API int ttl_volume_alloc(int32_t device, size_t bytes, int32_t try_contiguous, void **out,
                     int32_t *contiguous_out);
TTL_API int ttl_volume_free(void *ptr);


/* Repack an SH volume [X][Y][Z][C] f32 (the layout of
 * TTL/environments/env.py:169-180 `data_volume`) into 16-byte aligned voxel
 * records of coef_pitch floats, zero padded, in `layout` order; dst holds
 * ttl_sh_volume_records(dim, layout) records.  Once per subject. */
TTL_API int ttl_pack_sh_volume(const float *src, float *dst, const int32_t *dim /*[3]*/,
                       int32_t n_coef, int32_t coef_pitch, int32_t layout,
                       void *hip_stream);

/* Per-cell shortcut table for the mask test (see ttl_env_desc.mask_classes):
 * 1 = all 64 spline taps of the cell are >= threshold, 2 = all are below,
 * 0 = undecided.  Once per subject and threshold. */
TTL_API int ttl_mask_classes(const double *mask_coef, const int32_t *dim /*[3]*/,
                     double threshold, uint8_t *classes_out, void *hip_stream);

/* Validates the descriptor and creates a handle (no device work).
 * Replaces the per-subject setup of BaseEnv.load_subject, env.py:143-281. */
TTL_API int ttl_env_create(const ttl_env_desc *desc, ttl_env **out);
TTL_API void ttl_env_destroy(ttl_env *env);

/* TrackingEnvironment.reset / nreset (tracking_env.py:91-133 / 47-89):
 * n seeds (float32 [n][3], voxel space) become streamlines 0..n-1 of one
 * point; flags 0, lengths 1, dones 0, continue_idx = arange(n); writes the
 * first state rows ([n][state_pitch] f32, state_pitch >= 7*C + 3*K).
 * processing_order (device int32 [n], a permutation of 0..n-1, or NULL) does
 * not change any result: it only chooses which streamlines one workgroup of
 * the state gather handles together.  Passing the seeds sorted by spatial
 * brick lets neighbouring workgroups share voxels through L2; the library
 * keeps the order compacted as streamlines stop.  TTL_ORDER_BY_POSITION asks
 * the library to build that order itself (as ttl_env_refresh_processing_order
 * does later in the episode). */
#define TTL_ORDER_BY_POSITION ((const int32_t *)(uintptr_t)1)
TTL_API int ttl_env_reset(ttl_env *env, const float *seeds, int32_t n,
                  const int32_t *processing_order, float *state_out,
                  int64_t state_pitch, void *hip_stream);

/* Bidirectional tracking (TTL_HAS_RETRACK).  The reference tracks one
 * way from the seed (Tracker.track: reset -> validation_episode -> get_streamlines);
 * this call turns a finished batch round so that the ordinary step loop grows the
 * other half.  For every streamline g of the last ttl_env_reset, with f = lengths[g],
 * minus the point a CURVATURE / MASK stop drops (the rule of get_streamlines,
 * tracking_env.py:263-284; f >= 1):
 *   - the first f points of its history row are reversed in place (one wavefront
 *     per row), so that it reads forward end .. seed; init_len[g] = f;
 *   - flags 0, lengths 1, dones 0, continue_idx = arange(n), length 1, as after a
 *     reset; the first state rows ([n][state_pitch] f32) are those of the forward
 *     ends.  processing_order as for ttl_env_reset.
 * Until the next ttl_env_reset the handle is in retrack mode: a step that finds a
 * row at a length L < init_len[g] REPLAYS it -- the new point is hist[g][L] as it
 * stands, nothing is written to the history, action, noise (none is drawn, noise_out
 * keeps its row) and first-step flip are ignored, only the LENGTH criterion is
 * evaluated, the reward is 0; done_out, the survivor counts and the state rows are
 * written as always.  The stored points passed CURVATURE and MASK on the way out
 * (reversed, the curvature test multiplies the same numbers), except the seed, which
 * no criterion has seen and which may lie outside the mask: stopping there would
 * cost the streamline its seed.  From L >= init_len[g] on the row is an ordinary
 * row; one with f == 1 never replays and takes the ordinary first step, flip
 * included.  The batch stays in lock-step (one length for all rows) and ends with
 * whole streamlines, forward end .. seed .. backward end, the seed at point
 * init_len[g] - 1, of at most max_nb_steps points.
 *   init_len  device int32 [n], written here, BORROWED until the next ttl_env_reset.
 * TTL_ERR_INVALID for a null handle or buffer or a state_pitch too small;
 * TTL_ERR_STATE unless every row of the last reset has stopped and been harvested
 * and the count read (so: also before the first reset, between a step and its
 * harvest, and while free-running).  In retrack mode ttl_env_freerun_begin returns
 * TTL_ERR_UNSUPPORTED (a captured graph carries the kernel variant). */
#define TTL_HAS_RETRACK 1
TTL_API int ttl_env_reset_backward(ttl_env *env, int32_t *init_len,
                                   const int32_t *processing_order, float *state_out,
                                   int64_t state_pitch, void *hip_stream);

/* TrackingEnvironment.step (tracking_env.py:135-221) for the n_active
 * streamlines of continue_idx (n_active must equal the count the last
 * reset/harvest reported):
 *   actions   [n_active][3] f32 (row i belongs to continue_idx[i])
 *   noise     [n_active][3] f64 added to the action first (F64DIR mode,
 *             noisy_tracking_env.py:73-77), or NULL for +0.0
 *   state_out [n_active][state_pitch] f32, row order per `order`
 *   reward_out[n_active] f64 or NULL  (row i = active row i, always)
 *   done_out  [n_active] u8           (row i = active row i, always)
 *   host_counts pinned host memory, 4 x int32, or NULL: receives
 *             {n_continue, n_stopped, sequence, reserved}.  When the buffer is
 *             device-visible (hipHostMalloc / torch pin_memory) the kernel
 *             that computes the counts -- k_prefix, before the state gather
 *             has even started, or the one-launch tail of batches of at most
 *             16384 rows -- writes them and then a process-unique sequence
 *             number (bit 30 set, so that it can never equal the "steps done"
 *             count a free-running episode leaves in the same word) straight
 *             into it, and ttl_env_wait_counts() polls that
 *             word: the host can queue the next step while this one's gather
 *             is still running, with no copy kernel competing for the CUs.
 *             Otherwise (or with TTL_POLL_COUNTS=0) the counts are copied on
 *             a side stream as soon as the stopping decisions are final.
 * Normalise + scale the action, first-step flip, grow by one point, LENGTH /
 * CURVATURE / MASK stopping tests, flags and dones, alignment reward, new
 * state.  continue_idx itself only changes in ttl_env_harvest(). */
TTL_API int ttl_env_step(ttl_env *env, const float *actions, const double *noise,
                 int32_t n_active, int32_t order, float *state_out,
                 int64_t state_pitch, double *reward_out, uint8_t *done_out,
                 int32_t *host_counts, void *hip_stream);

/* The same step in two halves, for stopping criteria evaluated outside the
 * library (OracleStoppingCriterion, stopping_criteria.py:85-154, needs the new
 * points and a transformer forward):
 *   ttl_env_step_begin  actions -> new points, LENGTH/CURVATURE/MASK
 *                       decisions, reward, done_out;
 *   (caller computes extra_flags[n_active] u8, e.g. TTL_FLAG_ORACLE per row)
 *   ttl_env_step_end    ORs extra_flags (may be NULL) into flags / dones /
 *                       done_out, compacts, writes the state rows.
 * ttl_env_step() == begin + end(NULL). */
TTL_API int ttl_env_step_begin(ttl_env *env, const float *actions, const double *noise,
                       int32_t n_active, double *reward_out, uint8_t *done_out,
                       void *hip_stream);
TTL_API int ttl_env_step_end(ttl_env *env, const uint8_t *extra_flags, int32_t order,
                     float *state_out, int64_t state_pitch, int32_t *host_counts,
                     void *hip_stream);

/* Blocks the calling host thread until the host_counts of the last
 * ttl_env_step() have landed (not until the step has finished).  Called after
 * ttl_env_harvest() it also tells the handle the exact survivor count, and
 * the next ttl_env_step() is then refused unless n_active equals it. */
TTL_API int ttl_env_wait_counts(ttl_env *env);

/* Between a step that was given host_counts and its harvest: waits for the
 * counts like ttl_env_wait_counts() (without consuming them) and returns the
 * rows that stopped in that step, compacted in active-row order -- what
 * OracleReward scores (oracle_reward.py:78-90: idx = arange(N)[dones]):
 * stop_list[2 q] = active row, stop_list[2 q + 1] = streamline id (row of the
 * history buffer) of the q-th of them, q < *n_stopped.  Device memory owned by
 * the handle, rewritten by the next step. */
TTL_API int ttl_env_stopped(ttl_env *env, const int32_t **stop_list, int32_t *n_stopped);

/* TrackingEnvironment.harvest (tracking_env.py:223-245): lengths of the
 * streamlines that stopped in the last step, continue_idx <- survivors
 * (stable).  If the last step used ORDER_ACTIVE and state_out != NULL the
 * survivors' rows are copied from state_in (the step's output) to the first
 * n_continue rows of state_out.  After an ORDER_PARTITION step nothing is
 * launched (the lengths were written by the step itself). */
TTL_API int ttl_env_harvest(ttl_env *env, const float *state_in, float *state_out,
                    int64_t state_pitch, void *hip_stream);

/* ttl_env_harvest() followed by ttl_env_wait_counts() in one call (one trip
 * through the FFI instead of two; small batches are host bound): returns the
 * survivor count through n_continue_out.  The last step must have been given
 * host_counts. */
TTL_API int ttl_env_harvest_wait(ttl_env *env, const float *state_in, float *state_out,
                         int64_t state_pitch, void *hip_stream,
                         int32_t *n_continue_out);

/* Free-running steps (ABI v7).  The tracking loops of the reference
 * (RLAlgorithm.validation_episode, rl.py:58-106, driven by Tracker.track,
 * tracker.py:110-116) run policy -> step -> harvest until every streamline of
 * the batch has stopped; with the default --n_actor (10 000) a step is a few
 * microseconds of GPU work and the loop is bound by the host's launches and by
 * the survivor count it fetches every step.  Between ttl_env_freerun_begin()
 * and ttl_env_freerun_end() the number of active rows, the current length and
 * the live continue_idx buffer are kept in device memory and advanced by the
 * step's own kernels, so ttl_env_freerun_step() is nothing but launches with
 * fixed arguments: it may be captured in a HIP graph (together with the policy
 * network that turns state rows into actions) and replayed until the pinned
 * words report no survivor.  Results are those of ttl_env_step(ORDER_PARTITION)
 * + ttl_env_harvest() on the same actions, row for row.
 *
 * begin: after a reset or a harvested step whose count was read; batches of at
 *   most 16 384 rows (TTL_ERR_UNSUPPORTED otherwise, also for a neighbourhood
 *   radius outside (0, 1) voxel).  host_counts (may be NULL): 4 int32 of
 *   pinned, device-visible memory; every step writes {n_continue, n_stopped,
 *   steps done since begin} there.
 * step: covers rows 0..n_rows-1: actions [n_rows][3] f32, state_out
 *   [n_rows][state_pitch] f32, reward_out [n_rows] f64 or NULL, done_out
 *   [n_rows] u8.  n_rows is at most the row count at begin and must not be less
 *   than the number of rows active now -- the count a previous step reported
 *   through host_counts is such a bound (counts only fall), so a host loop may
 *   shrink its action batches with the survivors without ever waiting for the
 *   GPU; a step launched for too few rows does nothing but count itself.
 *   Rows 0..n_active-1 (n_active as the previous step left it) are the active
 *   rows; state rows come out survivors first (stable), then the rows that
 *   stopped in this step; rows that left earlier get done = 1, reward = 0 and
 *   keep their old state row.  No Gaussian action noise from the caller
 *   (TTL_MODE_F64DIR adds +0.0) unless ttl_env_set_noise installed keyed noise,
 *   which the step then draws itself.
 * end: waits for the stream, reads the device words back into the handle
 *   (which then continues as after a harvest) and returns them. */
TTL_API int ttl_env_freerun_begin(ttl_env *env, int32_t *host_counts, void *hip_stream);
TTL_API int ttl_env_freerun_step(ttl_env *env, const float *actions, int32_t n_rows,
                         float *state_out, int64_t state_pitch, double *reward_out,
                         uint8_t *done_out, void *hip_stream);
TTL_API int ttl_env_freerun_end(ttl_env *env, int32_t *n_active_out, int32_t *length_out,
                        int32_t *steps_out, void *hip_stream);
/* Keyed action noise (TTL_HAS_KEYED_NOISE).  Instead of reading
 * noise rows from the caller, the step's first kernel draws them: the three
 * float64 normals of a streamline at a step are a pure function of
 * (seed, id, step), so a tractogram no longer depends on how its seeds were cut
 * into batches, shards or loop flavours.
 *   generator  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
 *              0x9E3779B9 / 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32),
 *              counter = (id & 0xffffffff, id >> 32, step, j), j = 0, 1;
 *   uniforms   output words c0..c3 of call j: u1 = ((c1:c0 >> 11) + 0.5) * 2^-53,
 *              u2 likewise from c3:c2;
 *   normals    r = sqrt(-2 log u1), z[2j] = r cos(2 pi u2), z[2j+1] = r sin(2 pi u2),
 *              all in float64; a streamline uses z[0], z[1], z[2];
 *   id         id_base + g, g = the streamline's row of the history buffer;
 *   step       the length the step finds (1 at the first step after a reset).
 * The noise of a row is z * sigma_row: sigma_row = sigma, or with an FA map
 * max(0, (1 - FA) * sigma) (noisy_tracking_env.py:65-72; the clamp is a stated
 * deviation: a spline can overshoot FA > 1), FA = map_coordinates(fa_coef,
 * trunc_int32(p) - 0.5, order=3, mode='constant', prefilter=False) at the
 * streamline's newest point p before the step.
 *   fa_coef    device f64 [fa_dim[0]][fa_dim[1]][fa_dim[2]] cubic B-spline
 *              coefficients (scipy.ndimage.spline_filter(order=3)), or NULL;
 *   noise_out  device f64 [n_total][3] or NULL: row g receives the noise (sigma_row
 *              included) streamline g was given in the step that advanced it.
 * ttl_env_set_noise(env, NULL) switches it off.  TTL_MODE_F64DIR only
 * (TTL_ERR_INVALID otherwise, as for a negative or non-finite sigma, a negative
 * id_base or a misaligned table); TTL_ERR_STATE between a step and its harvest
 * and while free-running.  With keyed noise set, ttl_env_step / ttl_env_step_begin
 * refuse a non-NULL `noise` (TTL_ERR_INVALID), ttl_env_freerun_step draws as well,
 * and sigma == 0 adds +0.0.  Host state only: no device work. */
#define TTL_HAS_KEYED_NOISE 1
typedef struct ttl_noise_desc {
    uint64_t seed;
    int64_t id_base;
    double sigma;
    const double *fa_coef;
    int32_t fa_dim[3];
    double *noise_out;
} ttl_noise_desc;
TTL_API int ttl_env_set_noise(ttl_env *env, const ttl_noise_desc *desc);

/* The standard normals above for arbitrary ids (device int64 [n], >= 0) at one
 * step (>= 0): out [n][3] f64, device.  The same device function as the step's
 * draw: callers replay the noise of a finished run with it. */
TTL_API int ttl_noise_normals(uint64_t seed, const int64_t *ids, int32_t n, int32_t step,
                              double *out, void *hip_stream);

/* Measurement only: ttl_scripted_actions() for a free-running step -- the row
 * count, the step number (length - 1) and the live continue_idx buffer are
 * read from the device words; rows 0..min(n_active, n_rows)-1 are written. */
TTL_API int ttl_env_freerun_scripted_actions(ttl_env *env, const float *state, int64_t state_pitch,
                                     int32_t dir_offset, int32_t n_rows, uint32_t seed,
                                     float wobble, float *actions_out, void *hip_stream);

/* BaseEnv._compute_stopping_flags (env.py:567-603) on caller-supplied points:
 * tail [n][3][3] f32 holds the last three points (oldest first) of n
 * streamlines that have n_points points each (with n_points == 2 the first
 * entry of a tail is ignored, with n_points == 1 the first two are).
 * flags_out[n] u8 = OR of TTL_FLAG_* (0 = keeps going).  Touches no env state. */
TTL_API int ttl_env_stopping_flags(ttl_env *env, const float *tail, int32_t n,
                           int32_t n_points, uint8_t *flags_out,
                           void *hip_stream);

/* Replaces the processing order of the state gather between a harvest and the
 * next step: order[n] (device, int32) is a permutation of the n currently
 * active rows.  Like the order given to ttl_env_reset it is a scheduling hint
 * only (which rows a workgroup gathers together; tracking_env.py fixes the
 * ROW order, not this): results do not depend on it.  The host classes
 * refresh it every few steps from the streamlines' current positions, because
 * an order sorted by seed position decays as the streamlines travel. */
TTL_API int ttl_env_set_processing_order(ttl_env *env, const int32_t *order, int32_t n,
                                 void *hip_stream);

/* The same, computed by the library: active rows sorted by the 8^3-voxel brick
 * of their streamline's newest point (key kernel + counting sort on workspace
 * memory, no allocation).  Between a harvest and the next step, after the
 * survivor count has been read back. */
TTL_API int ttl_env_refresh_processing_order(ttl_env *env, void *hip_stream);

/* Slots of the processing order as it stands (0: no order in use): the active
 * rows plus the holes that stopped streamlines have left since the order was
 * last rebuilt.  *instep_out (may be NULL) receives the period of the in-step
 * re-bucket: with TTL_ORDER_INSTEP=P in the environment at ttl_env_create, the
 * steps that run the one-launch tail rebuild the order by brick themselves on
 * every P-th step of an episode (half of a counting sort inside that tail, one
 * short kernel behind it; the order has no holes afterwards), and the caller
 * need not call ttl_env_refresh_processing_order periodically.  0: off, or the
 * volume has too many bricks for it. */
TTL_API int ttl_env_order_slots(ttl_env *env, int32_t *n_slots_out, int32_t *instep_out);

/* Riders of the gather launch (TTL_HAS_TAIL_RIDERS).  Two parts of a step
 * with the one-launch tail are needed by nothing before the next step: the order
 * scatter of an in-step re-bucket and the row maps (continue_idx of the next step,
 * row_dest, lengths, the stopped list).  They run as extra workgroups behind the state
 * gather's own, inside its launch, and are complete when the step's launches are.
 * TTL_TAIL_RIDERS in the environment at ttl_env_create: 1 (default) both, 0 none (the
 * separate launches), 2 / 3 the order scatter / the row maps alone.  *kinds_out: bit 0
 * the order scatter, bit 1 the row maps, as the knob asks; *last_step_out (may be
 * NULL): the same bits for what rode in the last ttl_env_step / ttl_env_step_end (0
 * where that step took another tail, a persistent gather grid, or, for bit 0, was no
 * re-bucket step or has a brick raster whose scan needs more than 16 KB of LDS).
 * *order_out (may be NULL; for the tests): the processing order the next step will
 * read, device int32 [n_slots of ttl_env_order_slots] of active rows with -1 for a
 * hole, owned by the handle and final once the stream has run the last step; NULL
 * where no order is in use.  Host state only. */
#define TTL_HAS_TAIL_RIDERS 1
TTL_API int ttl_env_tail_riders(ttl_env *env, int32_t *kinds_out, int32_t *last_step_out,
                                const int32_t **order_out);

/* Current continue_idx buffer (device, int32 [n_active]) and, after a step,
 * the active-row -> output-row map (device, int32 [n_active]). */
TTL_API int ttl_env_view(ttl_env *env, const int32_t **continue_idx,
                 const int32_t **row_dest, int32_t *length);

/* Measurement support (bench.py): while profiling is on, every kernel launched
 * by ttl_env_step() is bracketed by HIP events on the caller's stream.
 * ttl_env_profile_end() synchronises those events and returns, per kernel
 * class {0: advance, 1: prefix, 2: state gather, 3: processing-order
 * compaction (ABI v9)}, the summed duration in ms and the number of launches,
 * then switches profiling off. */
#define TTL_PROFILE_CLASSES 4
TTL_API int ttl_env_profile_begin(ttl_env *env, int32_t max_launches,
                          int32_t class_mask /* bit k = time class k */);
TTL_API int ttl_env_profile_end(ttl_env *env, double *total_ms /*[TTL_PROFILE_CLASSES]*/,
                        int32_t *n_launches /*[TTL_PROFILE_CLASSES]*/);

/* Scripted, policy-free actions for "env.step only" runs (stands in
 * for agent.select_action, TTL/algorithms/rl.py:91): step 0 -> a random
 * vector; later -> unit(previous segment) + wobble * noise, the previous
 * segment being state[i][dir_offset .. dir_offset+2] (dir_offset = 7*C).  The
 * noise is a counter-based hash of (seed, step, continue_idx[i], component),
 * reproduced bit for bit by oracle/scripted_policy.py. */
TTL_API int ttl_scripted_actions(const float *state, int64_t state_pitch,
                         int32_t dir_offset, const int32_t *continue_idx,
                         int32_t n, uint32_t seed, uint32_t step, float wobble,
                         float *actions_out, void *hip_stream);

/* fODF policy (TTL_HAS_ODF_POLICY): classical tracking from the
 * fODF as a policy, state rows -> actions.  Per row i:
 *   sh[c]  = state[i][c], c < n_coef (the SH coefficients interpolated at the
 *            streamline's head: block 0 of the neighbourhood);
 *   p      = state[i][dir_offset .. dir_offset + 2], the newest previous
 *            direction (zero at the first step of an episode);
 * per call: sf_matrix [n_coef][n_vertices] f32; dirs [n_vertices][3] f32, unit
 * vectors of one hemisphere in the env's voxel axes (the library knows no
 * affine); cos_theta, the cosine of the cone's half angle; rel_threshold; mode;
 * seed.  All arithmetic in float32, one rounding per multiply and per add, sums
 * serial (c ascending, then v ascending); tests/ref_odf_policy.py restates it.
 *   sf[v]      = sum_c sh[c] * B[c][v]; gmax = max_v sf[v], by `>` from -inf (a
 *                comparison with NaN is false: a NaN never wins);
 *   cone       only when p != 0: vertex v is in the cone when
 *                |p . d_v| >= cos_theta * ||p||  (inclusive, two-sided: a
 *                hemisphere vertex stands for +-d), p . d = (px dx + py dy) + pz dz,
 *                ||p|| = sqrt((px px + py py) + pz pz);
 *   admissible in the cone (or p == 0), sf[v] > 0 and sf[v] >= rel_threshold * gmax
 *                (relative to the whole hemisphere's maximum, not the cone's);
 *   TTL_ODF_DET  the admissible vertex of largest sf, ties to the lowest index;
 *   TTL_ODF_PROB cdf[v] = sum of sf over the admissible vertices <= v (serial); the
 *                pick is the first v with cdf[v] > u * cdf[V - 1];
 *   u          Philox4x32-10 as for the keyed noise, key = the two halves of
 *                `seed`, counter = (id low, id high, step, TTL_ODF_STREAM);
 *                u = (output word 0 >> 8) * 2^-24, in [0, 1);
 *                id = ids_base + continue_idx[i] (the keyed noise's id), so a
 *                pick depends on neither batch size, row order nor loop flavour;
 *   action     d_v, negated when p . d_v < 0 (+ when it is 0 or p == 0);
 *   fallback   no admissible vertex: the action is p as given (straight on; the
 *                mask or the curvature test ends the row), dirs[0] when p == 0;
 *                vertex_out = -1.
 * state [n][state_pitch] f32, continue_idx [n] int32, actions_out [n][3] f32,
 * vertex_out [n] int32 or NULL (the chosen vertex), all device.  TTL_ERR_INVALID
 * for a null pointer, n < 0, n_coef outside 1 .. TTL_ODF_MAX_COEF, n_vertices < 1,
 * dir_offset < 0, a state_pitch below n_coef or dir_offset + 3, an unknown mode
 * or ids_base < 0; n == 0 launches nothing.  One lane per row; a launch has at most
 * TTL_ODF_GRID_CAP workgroups, each taking groups of 256 rows in a loop, with
 * sf_matrix and dirs staged in LDS (in chunks of vertices where they do not fit:
 * n_vertices has no upper limit; TTL_ERR_UNSUPPORTED where the device gives a
 * workgroup too little LDS for one chunk). */
#define TTL_HAS_ODF_POLICY 1
#define TTL_ODF_DET 0
#define TTL_ODF_PROB 1
#define TTL_ODF_MAX_COEF 64        /* the widest SH record of the deduplicating gather */
#define TTL_ODF_GRID_CAP 1024
#define TTL_ODF_STREAM 0x4F444650u /* counter word 3 ("ODFP"); the keyed noise uses 0 and 1 */
TTL_API int ttl_odf_actions(const float *state, int64_t state_pitch, int32_t n_coef,
                            int32_t dir_offset, const float *sf_matrix, const float *dirs,
                            int32_t n_vertices, float cos_theta, float rel_threshold,
                            int32_t mode, uint64_t seed, int64_t ids_base,
                            const int32_t *continue_idx, int32_t n, uint32_t step,
                            float *actions_out, int32_t *vertex_out, void *hip_stream);
/* The same for a free-running step (capturable in the step's graph): the row
 * count, the step number (length - 1) and the live continue_idx buffer are
 * read from the device words; rows 0..min(n_active, n_rows)-1 are written.
 * n_rows in 1 .. the rows at ttl_env_freerun_begin; TTL_ERR_STATE unless
 * free-running. */
TTL_API int ttl_env_freerun_odf_actions(ttl_env *env, const float *state, int64_t state_pitch,
                                        int32_t n_coef, int32_t dir_offset,
                                        const float *sf_matrix, const float *dirs,
                                        int32_t n_vertices, float cos_theta,
                                        float rel_threshold, int32_t mode, uint64_t seed,
                                        int64_t ids_base, int32_t n_rows, float *actions_out,
                                        int32_t *vertex_out, void *hip_stream);

/* Anatomically constrained stopping (TTL_HAS_ACT): the tissue-map
 * criteria of ACT (dipy's ActStoppingCriterion) and CMC (Girard 2014, dipy's
 * CmcStoppingCriterion) as stopping bits for ttl_env_step_end(extra_flags).
 * include / exclude: device f32 [X][Y][Z] maps of equal dims (z fastest), e.g.
 * grey matter and CSF.  tests/ref_act.py restates the definition.
 * Sampling, for row r < n:
 *   g    = ids[r] (r when ids is NULL); p = point n_points - 1 of history row g
 *          (history [.][row_pitch] f32, three floats per point);
 *   x_c  = (double)p_c + coord_shift;
 *   inside iff x_c >= -0.5 and x_c < dim_c - 0.5 for every c (NaN compares false:
 *          NaN and +-Inf are outside).  Outside: include = exclude = 0 and no bit
 *          (the tracking mask ends such a row);
 *   inside: i_c = floor(x_c), f_c = x_c - i_c, lo_c = clamp(i_c, 0, dim_c - 1),
 *          hi_c = clamp(i_c + 1, 0, dim_c - 1); all in float64, every multiply and
 *          every add rounded once, in this order:
 *            along z: c_ab = v[a][b][lo_z] * (1 - f_z) + v[a][b][hi_z] * f_z,
 *                     a in {lo_x, hi_x}, b in {lo_y, hi_y};
 *            along y: c_a  = c_a,lo * (1 - f_y) + c_a,hi * f_y;
 *            along x: val  = c_lo * (1 - f_x) + c_hi * f_x;
 *   values_out (or NULL) [r][0] = include, [r][1] = exclude, for every row.
 * Suppression: with init_len != NULL a row with n_points <= init_len[g] gets
 *   flags_out[r] = 0: in a backward pass (ttl_env_reset_backward) only points the
 *   pass itself created are judged, never the replayed half or the seed (`<=`, where
 *   the oracle criterion has `>`: a seed inside grey matter must not end its own
 *   backward half).
 * TTL_ACT_THRESHOLD: TTL_FLAG_TARGET iff include > 0.5, otherwise TTL_FLAG_EXCLUDE
 *   iff exclude > 0.5, otherwise 0: include first, never both bits.
 * TTL_ACT_CMC: s = include + exclude; not s > 0: 0.  num = 1 - s, 0 when negative;
 *   den = num + s; rho = num / den; P = pow(rho, exponent) in float64 (rho itself
 *   for exponent == 1).  Philox4x32-10 as at ttl_env_set_noise, key = the two halves
 *   of `seed`, counter = (id low, id high, n_points, TTL_ACT_STREAM), id = ids_base
 *   + g; u1 = (word 0 >> 8) * 2^-24, u2 = (word 1 >> 8) * 2^-24.  The row stops iff
 *   u1 >= P (s >= 1 always stops); a stopped row is TTL_FLAG_TARGET iff
 *   u2 < include / s, else TTL_FLAG_EXCLUDE.
 * TTL_ERR_INVALID before any launch, flags_out untouched: a null desc, map, history
 * or flags pointer, a dim < 1, an unknown mode, n < 0, n_points < 1, row_pitch <
 * 3 * n_points, ids_base < 0, in CMC mode an exponent not finite and positive.
 * n == 0 launches nothing.  One lane per row, workgroups of 256. */
#define TTL_HAS_ACT 1
#define TTL_FLAG_TARGET  8      /* StoppingFlags.STOPPING_TARGET: ended by the include map */
#define TTL_FLAG_EXCLUDE 128    /* no StoppingFlags member: ended by the exclude map       */
#define TTL_ACT_THRESHOLD 0
#define TTL_ACT_CMC       1
#define TTL_ACT_STREAM 0x41435420u   /* Philox counter word 3; noise uses 0/1, the fODF policy 0x4F444650 */
typedef struct ttl_act_desc {
    const float *include, *exclude;  /* device f32 [X][Y][Z], same dims */
    int32_t dim[3]; int32_t mode;
    double coord_shift;              /* added to a coordinate before sampling; 0: voxel i centred at i */
    double exponent;                 /* CMC: step_size_mm / mean voxel size; > 0, finite */
    uint64_t seed; int64_t ids_base;
} ttl_act_desc;
TTL_API int ttl_act_flags(const ttl_act_desc *desc, const float *history, int64_t row_pitch,
                          const int32_t *ids, const int32_t *init_len, int32_t n,
                          int32_t n_points, uint8_t *flags_out, double *values_out,
                          void *hip_stream);

/* The same criterion inside the step (TTL_HAS_ACT_IN_STEP): installed on
 * the handle once, as keyed noise is (ttl_env_set_noise), and applied in-stream by
 * every flavour of the step -- ttl_env_step, ttl_env_step_begin / _end,
 * ttl_env_freerun_step, a graph captured from it, a backward pass -- with no host in
 * between.  The descriptor is copied; the two maps are BORROWED until the next
 * ttl_env_set_act or ttl_env_destroy.  ttl_env_set_act(env, NULL) switches it off.
 * With a criterion installed, a step that finds the batch at length L leaves every
 * buffer of the handle and every output -- flags, dones, lengths, stop, done_out,
 * reward_out, continue_idx after the harvest, the state rows and their order,
 * host_counts -- exactly as this sequence leaves them:
 *   ttl_env_step_begin;
 *   ttl_act_flags(desc, history, pitch, ids = the live continue_idx, init_len = the
 *                 handle's in retrack mode else NULL, n = n_active, n_points = L + 1);
 *   ttl_env_step_end(extra_flags = those bits).
 * A row that another criterion stopped as well keeps those bits and gets the new ones
 * (the rule of ttl_env_step_end's extra_flags); rows beyond n_active are not judged;
 * extra_flags given to ttl_env_step_end are OR-ed on top as without a criterion.  The
 * criterion is applied by ttl_env_step_begin (one launch behind the one that moves the
 * points: done_out is final for it when that call's launches have run).
 * Free-running: n_active, L and the live continue_idx buffer are those the step's
 * first kernel snapshots; a step launched for fewer rows than are active judges
 * nothing.  ttl_env_freerun_begin leaves the criterion of the episode -- maps, mode,
 * exponent, seed, ids_base, or "none" -- in device memory of the handle, where the
 * step reads it: a graph captured from ttl_env_freerun_step with a criterion installed
 * stays valid when ttl_env_set_act is called again between episodes, with other values
 * or with NULL (its hook then changes nothing).  A graph captured with NO criterion
 * installed holds no hook and does not apply one installed later: capture again.
 * With nothing installed every entry point issues the launches it issued before.
 * TTL_ERR_INVALID as ttl_act_flags refuses a descriptor (a null map, a dim < 1, an
 * unknown mode, ids_base < 0, in CMC mode an exponent not finite and positive);
 * TTL_ERR_STATE between a step and its harvest and while free-running; a refused call
 * leaves the installed criterion as it was.  Host state only: no device work. */
#define TTL_HAS_ACT_IN_STEP 1
TTL_API int ttl_env_set_act(ttl_env *env, const ttl_act_desc *desc);

/* fODF peaks of an SH volume (replaces the per-voxel Python loop of
 * TrackToLearn/environments/env.py:405-432: sh_to_sf_matrix + get_maximas per
 * voxel, 5 peaks scaled by value / first value).  sh: [n_voxels][n_coef] f32;
 * sf_matrix: [n_coef][n_vertices] f32 (SF = SH @ matrix); vertices:
 * [n_vertices][3] unit vectors of one hemisphere; neighbours:
 * [n_vertices][degree] vertex indices of the hemisphere graph (rows padded with
 * the vertex itself).  A direction is a peak if its SF value (values below
 * absolute_threshold count as 0) is >= all neighbours, > one of them and > 0;
 * peaks are taken in decreasing order among the max_candidates largest, kept
 * while value - max(min SF, 0) >= relative_threshold * that of the first and
 * |cos| to every kept peak <= min_separation_cos.  peaks_out:
 * [n_voxels][3*npeaks] f32, zeros for voxels whose coefficients sum to 0 and
 * for missing peaks.  All pointers are device memory. */
TTL_API int ttl_peaks_from_sh(const float *sh, int64_t n_voxels, int32_t n_coef,
                      const float *sf_matrix, const float *vertices,
                      const int32_t *neighbours, int32_t n_vertices, int32_t degree,
                      int32_t npeaks, float relative_threshold, float absolute_threshold,
                      float min_separation_cos, int32_t max_candidates, float *peaks_out,
                      void *hip_stream);

/* TractOracle-Net forward (TrackToLearn/oracles/transformer_oracle.py:77-92 under the
 * autocast of oracles/oracle.py:76): scores[i] = sigmoid(head(encoder(embed([CLS; dirs[i]]))[0]))
 * for n sequences of 127 segment vectors, ONE launch (csrc/ttl_oracle_net.hip): one
 * workgroup per streamline for n <= 512, one wavefront per streamline above (the environment
 * variable TTL_ORACLE_NET_WG = 1 / 0 forces the first / the second).  Each kernel is
 * deterministic and scores a row independently of its batch; the two agree to the rounding of
 * the fp16 score (the order of one float32 sum differs).  d_model 32, 128 tokens, n_head in
 * {1, 2, 4}, ReLU post-norm layers, ff_dim a multiple of 32, at most 8192 (TTL_ERR_UNSUPPORTED
 * otherwise).  b_1 of two layers is staged in LDS, 8 ff_dim bytes on top of the workgroup
 * kernel's 56 KB: the sum is checked against the device's limit per workgroup before the
 * launch (120 KB of the MI355X's 160 KB at 8192; TTL_ERR_UNSUPPORTED where it does not fit).
 * The weights come packed by
 * tracktolearn_amd/oracles/fused_net.py:pack_oracle_net (fp16 MFMA fragments in the k order an
 * accumulator tile presents, per-row vectors in accumulator row order):
 *   packed_half  [n_layers][8 + 4 ff_dim / 32][64][8] f16: W_q, W_k, W_v, W_o, W_1 chunks, W_2 chunks
 *   packed_float [n_layers][288 + ff_dim] f32: b_q, b_k, b_v, b_o, LN1 gain / bias, b_2,
 *                LN2 gain / bias, b_1 chunks
 *   embed [2][16][4], cls [3], pos_enc [4][64][16], head [33].
 * dirs: [n][127][3] f32; scores: [n] f32.  Device pointers. */
TTL_API int ttl_oracle_net_forward(const float *dirs, int64_t n, const void *packed_half,
                                   const float *packed_float, const float *embed,
                                   const float *cls, const float *pos_enc, const float *head,
                                   int32_t n_layers, int32_t n_head, int32_t ff_dim,
                                   float *scores, void *hip_stream);

/* Arc-length resampling of a padded batch of streamlines to nb_points points
 * each (the oracle's input, TrackToLearn/oracles/oracle.py:52,70: dipy
 * set_number_of_points).  points: [n] rows of row_pitch floats holding up to
 * max_len xyz points; lengths32 or lengths64 (exactly one non-null): valid
 * points per row; out: [n][nb_points][3] f32.  First and last point are kept,
 * the others sit at arc length k * total / (nb_points - 1) (float64), linearly
 * interpolated inside their segment.  Device pointers. */
TTL_API int ttl_resample_streamlines(const float *points, int64_t row_pitch,
                             const int32_t *lengths32, const int64_t *lengths64,
                             int32_t n, int32_t max_len, int32_t nb_points, float *out,
                             void *hip_stream);

/* The env's oracle path in one launch (oracle_reward.py:78-90,
 * stopping_criteria.py:132-150 -> oracles/oracle.py:52-72): for streamline
 * ids[r * id_stride] (NULL: r) of the history buffer, r < n, take its first
 * n_points points, map them with the row-major 3x3 matrix lin (host memory,
 * p' = p @ lin; NULL: none), resample to nb_points along the arc length as
 * ttl_resample_streamlines() does, and write the nb_points - 1 segment vectors:
 * dirs_out [n][nb_points - 1][3] float32, the network's input. */
TTL_API int ttl_oracle_segments(const float *history, int64_t row_pitch, const int32_t *ids,
                                int32_t id_stride, int32_t n, int32_t n_points,
                                const float *lin, int32_t nb_points, float *dirs_out,
                                void *hip_stream);

/* The oracle validator's input (ABI v12; TrackToLearn/experiment/oracle_validator.py:
 * 41-46, oracles/oracle.py:52-72) for a ragged tractogram: streamline i is
 * points [offsets[i], offsets[i + 1]) (points: [M][3] f32, offsets: [n + 1] int64), of any
 * length >= 2.  It is resampled to nb_points along the arc length exactly as
 * ttl_resample_streamlines() resamples it laid out padded (the same bits), and the
 * nb_points - 1 float32 differences go to dirs_out [n][nb_points - 1][3] f32.  One wavefront
 * per streamline; LDS does not grow with the length (the cumulative arc length is recomputed
 * from 64 lane prefixes).  A row of fewer than 2 points gives zero vectors.  Device pointers. */
TTL_API int ttl_oracle_segments_packed(const float *points, const int64_t *offsets, int32_t n,
                                       int32_t nb_points, float *dirs_out, void *hip_stream);

/* The oracle validator's coverage map (ABI v12; oracle_validator.py:48-53: scilpy
 * compute_tract_counts_map, binarised): for every streamline i < n of the ragged layout
 * above with scores[i] > threshold (scores: device f32 [n], or NULL to take every
 * streamline), visited[(x * Y + y) * Z + z] = 1 for the voxels it passes through
 * (dims = {X, Y, Z}, host memory; visited: device u8 [X * Y * Z], zeroed by the caller,
 * only ones are written).  Points are float32 voxel coordinates with corner origin: voxel
 * v spans [v, v + 1).  Walk, in float64: mark floor(c_0); for each segment a -> b with
 * va = floor(a), vb = floor(b), d = b - a, axis i crosses the integer planes between va_i
 * and vb_i (va_i + 1 .. vb_i when d_i > 0, va_i .. vb_i + 1 when d_i < 0), plane beta at
 * t = (beta - a_i) / d_i; crossings in increasing t, the lower axis first on ties; each one
 * steps that axis's index by sign(d_i) and marks the new voxel.  Voxels outside [0, dims)
 * are skipped, not clamped, and cost no work: per segment the work is the voxels marked
 * plus O(log dims).  Segments with a non-finite end mark nothing.  One wavefront per
 * streamline, one lane per segment; plain byte stores, no atomics.
 * Edges (tests/test_coverage_reference.py): the gate is a float32 `>`, so a streamline
 * with scores[i] == threshold or a NaN score is rejected and +Inf is accepted; a
 * non-finite point costs only its own two segments (and its own mark when it is the
 * first point), the rest of the streamline is walked; a row of 0 points marks nothing,
 * a row of 1 point marks floor(c_0); ends may lie at any finite float32 distance. */
TTL_API int ttl_tract_coverage(const float *points, const int64_t *offsets, int32_t n,
                               const float *scores, float threshold, const int32_t *dims,
                               uint8_t *visited, void *hip_stream);

/* The Tractometer validator (TrackToLearn/experiment/tractometer_validator.py: scilpy's
 * segment_tractogram_from_roi and compute_tractometry with compute_ic = False, unique = True;
 * scilpy's source is absent: restated here, parity unpinned).  Input is the
 * ragged layout of ttl_tract_coverage: corner-origin voxel coordinates of the Tractometer's
 * reference anatomy, dims = {X, Y, Z} (host memory).  The B = n_bundles bundles (1 .. 64,
 * the order of scil_scoring_config.json) live in bit planes, uint64 [X * Y * Z] each, word
 * (x * Y + y) * Z + z, bit b = bundle b: head, tail, all (all_mask; a bundle without one
 * has its bit set in every word), any (any_mask), gt (gt_mask).  has_all / has_any name the
 * bundles that have such a mask.  limits: device double [B][TTL_TRACTOMETER_LIMITS] =
 * {length lo, hi; dir x lo, hi, y .., z ..; absdir x lo, hi, y .., z ..; angle; unused},
 * -inf / +inf where the config sets none.  lin: host double [9], row-major linear part of
 * the reference's voxel -> RAS mm affine.
 *
 * For streamline s with points c_0 .. c_{L-1} (float32 read as float64, all sums float64):
 *   ends      e0 = floor(c_0), e1 = floor(c_{L-1}) (floor, not truncation: -0.3 is voxel
 *             -1); an end that is non-finite or outside [0, dims) lies in no ROI.
 *   connects(b) = (head_b[e0] & tail_b[e1]) | (tail_b[e0] & head_b[e1]).
 *   V(s)      the in-volume voxels of the walk of ttl_tract_coverage: floor(c_0) and the
 *             voxel entered at every plane crossing, same order, same ties.
 *   within(b) every voxel of V(s) has bit b in all (tested for the bundles of has_all);
 *   touches(b) some voxel of V(s) has bit b in any (tested for the bundles of has_any).
 *   v_j = lin (c_{j+1} - c_j), each row ((m0 x + m1 y) + m2 z); length = sum |v_j|,
 *   dir_k = |sum_j v_jk|, absdir_k = sum_j |v_jk|; limits are inclusive, lo <= x <= hi.
 *   winding   dipy's, on the voxel coordinates: q_j = c_j - mean(c), S = sum q_j q_j^T,
 *             u1, u2 the unit eigenvectors of its two largest eigenvalues (cyclic Jacobi,
 *             a fixed number of sweeps), p_j = (q_j . u1, q_j . u2), winding = (180 / pi)
 *             sum_j acos(clip(p_j . p_j+1 / (|p_j| |p_j+1|), -1, 1)); the bundle passes iff
 *             winding < angle (strict: a winding equal to the angle fails, and so does a
 *             NaN, which a p_j = 0 gives, against every finite angle).  A bundle with
 *             angle = +inf sets no angle: the criterion is skipped, the winding is not
 *             computed for it, and a NaN passes.
 *   valid(b)  = connects(b) and every criterion above that bundle b sets.
 * ttl_tractometer_classify writes bundle[s] = the lowest b with valid(b), else -1, and
 * connected[s] = the bit set of b with connects(b) (int32 [n], uint64 [n], device).  A row
 * of fewer than 2 points gives -1 and 0; a row with a non-finite point gives -1 (and the
 * connected set of its ends when both are finite).  One wavefront per streamline: the ends
 * first (four words; a row that connects nothing leaves here), then the sums and the limits
 * (lane b tests bundle b), then the walk if a surviving bundle has an all / any mask, then
 * the winding if one sets an angle.  The sums are butterfly reductions over the lanes, so a
 * quantity within rounding of a limit may decide differently than another summation order.
 *
 * ttl_tractometer_overlap: every row with 0 <= bundle[s] < B ORs bit bundle[s] into
 * visited_bits (uint64 [X * Y * Z], zeroed by the caller; only ones are ORed in, by
 * device-wide atomics, so the result does not depend on the order) for the voxels of V(s);
 * then counts[b] = {|M_b & G_b|, |M_b \ G_b|} (int64 [B][2], overwritten), M_b = the voxels
 * with bit b in visited_bits, G_b = those with bit b in gt: integer atomics, exact.
 * Both: device pointers unless stated; TTL_ERR_INVALID for a null pointer, n < 0, B outside
 * 1 .. 64 or a dim < 1; n == 0 is a successful no-op (overlap still counts). */
#define TTL_TRACTOMETER_LIMITS 16
TTL_API int ttl_tractometer_classify(const float *points, const int64_t *offsets, int32_t n,
                                     const int32_t *dims, int32_t n_bundles,
                                     const uint64_t *head, const uint64_t *tail,
                                     const uint64_t *all, const uint64_t *any,
                                     uint64_t has_all, uint64_t has_any, const double *limits,
                                     const double *lin, int32_t *bundle, uint64_t *connected,
                                     void *hip_stream);
TTL_API int ttl_tractometer_overlap(const float *points, const int64_t *offsets, int32_t n,
                                    const int32_t *bundle, const int32_t *dims,
                                    int32_t n_bundles, const uint64_t *gt,
                                    uint64_t *visited_bits, int64_t *counts, void *hip_stream);

/* The Tractometer's invalid connections (TTL_HAS_TRACTOMETER_IC; scilpy's
 * compute_ic = True; its source is absent: this project's own statement, parity unpinned).
 * The R = n_rois ROIs (2 .. TTL_TRACTOMETER_MAX_ROIS) are the distinct head / tail files of
 * the scoring set, sorted as strings: rois = sorted(set(gt_tails + gt_heads)); a file that
 * serves several bundles is one ROI.  D_r is ROI r's mask, dilated like the heads and tails
 * of ttl_tractometer_classify.  valid(i, j) holds when some bundle has {head, tail} =
 * {rois[i], rois[j]};  P = [(i, j) : 0 <= i < j < R, not valid(i, j)] in lexicographic
 * order is the list of invalid pairs.
 *   roi    device uint64 [X * Y * Z][W], W = (R + 63) / 64: bit r % 64 of word r / 64 of
 *          voxel (x * Y + y) * Z + z is D_r there; the words of a voxel are adjacent (and
 *          16-byte aligned when W = 2), so an end costs one 8- or 16-byte load.
 *   valid  device uint64 [R][W]: bit j of row i when valid(i, j) or i == j.
 *   bundle device int32 [n], as ttl_tractometer_classify wrote it.
 * Streamline s is a candidate when bundle[s] < 0 and it has L >= 2 points (a row that
 * connects a bundle's own ROIs but fails its criteria, connected[s] != 0, is a candidate
 * too).  Its ends e0, e1 are those of ttl_tractometer_classify (floor; an end that is
 * non-finite or outside [0, dims) lies in no ROI); interior points are not read.  With
 * A = {r : D_r[e0]}, B = {r : D_r[e1]} and
 *   connects(i, j) = (i in A and j in B) or (j in A and i in B),
 * pair[s] = i * R + j for the first (i, j) of P with connects(i, j), else -1 (int32 [n],
 * device).  A row with a bundle or with fewer than 2 points gets -1; so does a row whose
 * ends lie in one ROI and nowhere else (i == j is no pair).
 * One thread per streamline, grid-stride over at most 2048 workgroups; a row reads two
 * offsets, its bundle, two points and 2 W words.  The first pair is found without a loop
 * over P: for the set bits i of A | B in ascending order, J_i = ((i in A ? B : 0) |
 * (i in B ? A : 0)) & ~valid[i] & (bits above i); the first non-zero J_i gives j, its
 * lowest bit (a pair of P that connects has its smaller index in A | B, and J_i is the set
 * of its partners).  No atomics: counts per pair are the caller's histogram of pair.
 * TTL_ERR_INVALID for a null pointer, n < 0, R outside 2 .. 128 or a dim < 1; n == 0 is a
 * successful no-op. */
#define TTL_HAS_TRACTOMETER_IC 1
#define TTL_TRACTOMETER_MAX_ROIS 128
TTL_API int ttl_tractometer_invalid(const float *points, const int64_t *offsets, int32_t n,
                                    const int32_t *bundle, const int32_t *dims, int32_t n_rois,
                                    const uint64_t *roi, const uint64_t *valid, int32_t *pair,
                                    void *hip_stream);

/* The structural connectome (TTL_HAS_CONNECTOME): the node of a parcellation
 * at either end of every streamline, and the node x node matrices of streamline counts and
 * summed lengths.  This project's own statement; the reference has no counterpart.  Input
 * is the ragged layout of ttl_tract_coverage: corner-origin voxel coordinates of the label
 * image's grid (voxel v spans [v, v + 1), its centre is v + 0.5), dims = {X, Y, Z}, lin
 * (double [9], row-major linear part of voxel -> RAS mm) and reach (int32 [3]) in host
 * memory.  labels: device int32 [X * Y * Z], word (x * Y + y) * Z + z; the values 1 .. N =
 * n_nodes name a node, every other value (negatives and values above N included) is no node.
 *
 * ttl_connectome_assign, for streamline s with points c_0 .. c_{L-1} (float32 read as
 * float64, all arithmetic float64 in the written order):
 *   not scored  node[s] = (-1, -1), length[s] = 0 when L < 2, when a point is non-finite or
 *               when the length below is not < 2^40 mm.
 *   length[s]   = sum_j |v_j|, v_j = lin (c_{j+1} - c_j), each row ((m0 x + m1 y) + m2 z),
 *               |v| = sqrt((vx^2 + vy^2) + vz^2) (ttl_tractometer_classify's expressions);
 *               a butterfly sum over the lanes, so the order of the sum over j is the kernel's.
 *   node of an end p (c_0 for column 0, c_{L-1} for column 1; interior points are not read
 *               for it), e = floor(p) (floor, not truncation: -0.3 is voxel -1):
 *               1. e in [0, dims) and labels[e] a node: that node (the point is inside it);
 *               2. otherwise the candidates are the in-volume voxels v with |v_i - e_i| <=
 *                  reach_i on every axis, labels[v] a node and d2(v) <= radius_mm^2
 *                  (inclusive), w = lin (p - (v + 0.5)), d2 = (wx^2 + wy^2) + wz^2; the node
 *                  is the label of the candidate with the smallest d2, on equal d2 the one
 *                  with the smallest word index; 0 without a candidate.
 *               An end outside the volume is neither clamped nor rejected: the voxels within
 *               reach of it are still candidates; one so far out that no voxel of its box
 *               is in the volume gets 0 and costs no work (the box is cut to the volume in
 *               float64, before any conversion to an integer).  radius_mm = 0 with reach =
 *               {0, 0, 0} is therefore "the label of the end's own voxel".
 *   node[s]     = (node of c_0, node of c_{L-1}), in streamline order, not sorted (device
 *               int32 [n][2]; length: device double [n]).
 * One wavefront per streamline: lanes over the segments, then, for an end that step 1 did
 * not settle, lanes over the voxels of the box, z fastest, and a wave-wide minimum of
 * (d2, index) (non-negative doubles order as their bit patterns).  No atomics.
 *
 * ttl_connectome_accumulate: count and length_q are device int64 [N + 1][N + 1], ADDED TO,
 * not overwritten: the caller zeroes them once and streams batches in.  A row with
 * node[s][0] < 0 is skipped (and so is one that names a node above N); otherwise, with a =
 * min, b = max of its two nodes (0 = unassigned), count[a][b] += 1 and, when length is
 * non-null, length_q[a][b] += llrint(length[s] * TTL_CONNECTOME_LENGTH_SCALE), rounded half
 * to even.  Only the upper triangle (row 0 and the diagonal included) is touched.  Integer
 * atomics of device scope, exact: the matrices do not depend on the order or the split of
 * the rows.  One thread per row, grid-stride over at most 2048 workgroups; the rows of a
 * wavefront that share a cell are summed first: one atomic per distinct cell, wave and matrix.
 * Both: TTL_ERR_INVALID, before any HIP call, for a null pointer (except length of
 * accumulate, and hip_stream), n < 0, n_nodes outside 1 .. TTL_CONNECTOME_MAX_NODES, a dim
 * < 1, a reach_i outside 0 .. TTL_CONNECTOME_MAX_REACH, a radius_mm that is negative or
 * non-finite; n == 0 is a successful no-op. */
#define TTL_HAS_CONNECTOME 1
#define TTL_CONNECTOME_MAX_NODES 4096
#define TTL_CONNECTOME_MAX_REACH 8
#define TTL_CONNECTOME_LENGTH_SCALE 1048576.0   /* 2^20 units per mm */
TTL_API int ttl_connectome_assign(const float *points, const int64_t *offsets, int32_t n,
                                  const int32_t *labels, const int32_t *dims, int32_t n_nodes,
                                  const double *lin, double radius_mm, const int32_t *reach,
                                  int32_t *node /*[n][2]*/, double *length /*[n]*/,
                                  void *hip_stream);
TTL_API int ttl_connectome_accumulate(const int32_t *node, const double *length, int32_t n,
                                      int32_t n_nodes, int64_t *count, int64_t *length_q,
                                      void *hip_stream);

/* Weighted connectome edges (TTL_HAS_TRACT_SAMPLE, TTL_HAS_CONNECTOME_METRIC):
 * the mean of a scalar volume (FA, MD, AFD) along every streamline, and its sum per edge.
 * This project's own statement; the reference has no counterpart.  Input is the ragged layout
 * of ttl_connectome_assign, in the corner-origin voxel coordinates of the volume's grid
 * (voxel v spans [v, v + 1), its centre is v + 0.5); dims = {X, Y, Z} and lin (double [9],
 * row-major linear part of voxel -> RAS mm) in host memory.  volume: device float32
 * [X * Y * Z], word (x * Y + y) * Z + z.  Floats are read as float64 and all arithmetic is
 * float64 in the written order.
 *
 * ttl_tract_sample_mean, for streamline s with points c_0 .. c_{L-1}:
 *   sample s_j  at p = c_j: u = p - 0.5, i = floor(u) (floor, not truncation: -0.5 is voxel
 *               -1), f = u - i, g = 1 - f per axis.  The eight corners are i + {0, 1}^3, each
 *               index clamped to [0, dims_k - 1] (edge replicate; a dimension of 1 reads the
 *               same voxel twice).  With V(a, b, c) the value at corner (x: a, y: b, z: c),
 *               z pairs first, then y, then x:
 *                 Z(a, b) = V(a, b, 0) * gz + V(a, b, 1) * fz
 *                 Y(a)    = Z(a, 0) * gy + Z(a, 1) * fy
 *                 s_j     = Y(0) * gx + Y(1) * fx
 *   not sampled a point that is non-finite, that has some p_k < 0 or p_k > dims_k (the closed
 *               volume [0, dims] is inside; decided in float64 before any conversion to an
 *               integer, so a point at 1e30 is simply outside), or with a non-finite value
 *               among its eight corners (a corner of weight 0 included).
 *   weights     the trapezoid rule over the arc length in mm: |v_j| is
 *               ttl_connectome_assign's segment length of lin (c_{j+1} - c_j), but 0 when
 *               either end is non-finite; |v_{-1}| = |v_{L-1}| = 0; w_j = (|v_{j-1}| + |v_j|)
 *               * 0.5, so the two end points weigh half their one segment.
 *   weight[s]   = sum over the sampled j of w_j;
 *   mean[s]     = (sum over the sampled j of w_j * s_j) / weight[s];
 *               mean[s] = NaN and weight[s] = 0 when L < 2 or the sum of weights is not > 0
 *               (nothing sampled, or every sampled point between segments of length 0).
 *               Both sums are lane partial sums (lane l adds its points j = l, l + 64, ... in
 *               that order) and then a butterfly, so the order over j is the kernel's.
 *   tolerance   against the definition in exact arithmetic, with u = 2^-53, B_j the segment
 *               length taken with |lin| and |c_{j+1} - c_j| (magnitudes, as DESIGN 3.15's A_s),
 *               W_j = (B_{j-1} + B_j) / 2, S_j = the trilinear sum of |V| and, over the sampled
 *               j, A = sum W_j, M = sum W_j S_j:  a segment length carries 8 roundings (3.15),
 *               w_j one more, s_j 9 (g, product and sum on each of three levels), w_j * s_j
 *               one, a sum of L terms at most L - 1 on any path, the division one:
 *                 |weight - exact| <= (L + 9) u A
 *                 |mean - exact|   <= u ((L + 19) M + (L + 9) A M / weight) / weight.
 * One wavefront per streamline, lanes over the points, 64 a round.  A lane measures |v_j| and
 * takes |v_{j-1}| from the lane below by a shuffle; lane 0 takes the last lane's of the round
 * before, carried in a register (the bits a recomputation would give).  The two corners along
 * z of a pair are adjacent floats (the same float when clamped).  No atomics, no LDS, plain
 * stores by lane 0.  mean, weight: device double [n].
 *
 * ttl_connectome_accumulate_metric: metric_q and metric_n are device int64 [N + 1][N + 1],
 * ADDED TO, with the cell rule of ttl_connectome_accumulate (a = min, b = max of the row's
 * nodes, upper triangle, row 0 = unassigned).  A row is skipped when node[s][0] < 0 or it
 * names a node above N, when mean[s] is non-finite, or when |mean[s] * scale| >= 2^40;
 * otherwise metric_q[a][b] += llrint(mean[s] * scale) (half to even) and metric_n[a][b] += 1.
 * scale is a power of two in 2^-60 .. 2^60, so the product is exact short of underflow.  The
 * mean of an edge is metric_q / scale / metric_n: the mean over its streamlines of their
 * means.  The wave-level election and the device-scope integer atomics of
 * ttl_connectome_accumulate: exact, independent of the order and the split of the rows.
 * Both: TTL_ERR_INVALID, before any HIP call, for a null pointer (except hip_stream), n < 0,
 * a dim < 1, n_nodes outside 1 .. TTL_CONNECTOME_MAX_NODES, a scale that is not such a power
 * of two; n == 0 is a successful no-op. */
#define TTL_HAS_TRACT_SAMPLE 1
#define TTL_HAS_CONNECTOME_METRIC 1
TTL_API int ttl_tract_sample_mean(const float *points, const int64_t *offsets, int32_t n,
                                  const float *volume, const int32_t *dims, const double *lin,
                                  double *mean /*[n]*/, double *weight /*[n]*/, void *hip_stream);
TTL_API int ttl_connectome_accumulate_metric(const int32_t *node, const double *mean, int32_t n,
                                             int32_t n_nodes, double scale,
                                             int64_t *metric_q, int64_t *metric_n,
                                             void *hip_stream);

/* Track density maps (TTL_HAS_TRACT_DENSITY): per voxel, the number of
 * streamlines passing through it, the mm of streamline lying in it (in total and per RAS
 * axis: the direction-encoded density) and the number of streamline ends in it -- scilpy's
 * compute_tract_counts_map / MRtrix's tckmap.  This project's own statement; the reference
 * has no counterpart.  Input is the ragged layout of ttl_tract_coverage: points are float32
 * corner-origin voxel coordinates of the MAP's grid (a super-resolution map is fed points
 * already scaled to its grid), offsets int64 [n + 1]; dims = {X, Y, Z} with X * Y * Z <
 * 2^31 - 1, lin = double [9], row-major linear part of voxel -> RAS mm.  Floats are read as
 * float64 and all arithmetic is float64 in the written order.
 *
 * For streamline s with points c_0 .. c_{L-1}:
 *   not added   status[s] = -1 and no map changes when L < 2, when a point is non-finite or
 *               when the length sum_j |v_j| is not < 2^40 mm (ttl_connectome_assign's
 *               expressions and butterfly sum); decided before the row adds anything.
 *   pieces      the walk is ttl_tract_coverage's: same crossings, order and ties.  Per segment
 *               j (a = c_j, b = c_{j+1}, d = b - a) the merged crossing order cuts [0, 1]
 *               into pieces; a piece lies in the voxel the walk occupies between two
 *               consecutive crossings.  The first piece starts at t = 0 in floor(a), the last
 *               ends at t = 1; only pieces whose voxel is inside the volume exist.  In the
 *               bounded walk: a visited voxel is entered at its crossing's t and left at the
 *               t of the next crossing of the merged order -- the next visit, or the crossing
 *               X that leaves the volume -- or at 1 when there is none; floor(a)'s piece
 *               starts at 0 when a lies inside, and when a lies outside the first piece
 *               starts at E.  Every t is (plane - a_i) / d_i.  Tied crossings give pieces of
 *               length 0 in the voxels between them; those voxels are still visited.
 *   v_j         = lin d, each row ((m0 x + m1 y) + m2 z); |v_j| = sqrt((vx^2 + vy^2) + vz^2).
 * The maps are device arrays of [X * Y * Z] words, word (x * Y + y) * Z + z, ADDED TO: the
 * caller zeroes them once.  Each pointer may be NULL, not all of them.
 *   count       int32: += 1 for every voxel of V(s), the SET of voxels the row visits
 *               (floor(c_0) when inside, and every voxel entered); a voxel left and entered
 *               again, at once or later, counts once.
 *   length_q    int64: per piece += llrint(((t_hi - t_lo) * |v_j|) * TTL_CONNECTOME_LENGTH_SCALE),
 *               rounded half to even.
 *   dec_q       int64 [X * Y * Z][3]: per piece and k in {x, y, z}
 *               += llrint(((t_hi - t_lo) * fabs(v_jk)) * TTL_CONNECTOME_LENGTH_SCALE).
 *   ends        int32: += 1 at floor(c_0) and at floor(c_{L-1}), each when inside the volume;
 *               two ends in one voxel add 2.
 * All sums are integer atomics of device scope: the maps do not depend on the order of the
 * rows, their split into calls or the grid.  On rows that are added, (count > 0) is
 * ttl_tract_coverage's map.
 *   tolerance   of a piece against the definition in exact arithmetic, u = 2^-53: each t
 *               carries 3 roundings (plane - a_i, d_i, the division) and is <= 1, their
 *               difference one more: |(t_hi - t_lo) - exact| <= 7u; |v_j| carries 8 (DESIGN
 *               3.15) against B_j, the length taken with |lin| and |d|; the product one.  To
 *               first order |piece - exact| <= 16 u B_j, and 12 u B_jk for a component (4
 *               roundings per term of a row of lin).  In units of 2^-20 mm, with one unit for
 *               a llrint that falls on the other side: 1 + 17 u B_j 2^20 (13 for dec_q; the
 *               17th and 13th cover the second-order terms), summed over a voxel's pieces.
 *
 * The set and status (device int32 [n], overwritten).  Only count needs the set; the other
 * maps are added piece by piece.  With |V(s)| the number of distinct voxels:
 *    0   |V(s)| <= wave_slots / 2: counted through the wave's set in LDS (also: count NULL)
 *    1   otherwise, |V(s)| <= spill_slots / 2 and a workspace was given: counted by the
 *        spill pass of the same call
 *    2   otherwise: count got NOTHING from this row (all or nothing); the other three maps
 *        got everything.  The caller calls again for those rows with only count non-null
 *        and a larger workspace.
 *   -1   not added.
 * The thresholds are exact: the tier is a function of |V(s)| alone.  wave_slots: a power of
 * two in 64 .. TTL_DENSITY_MAX_WAVE_SLOTS, 0 = the default (2048); 4 * wave_slots * 4 bytes
 * of LDS per workgroup, refused (TTL_ERR_INVALID, after the device was asked: the one refusal
 * that follows a HIP call, as for ttl_resample_streamlines) when the device does not have them.  spill_slots: 0 or a
 * power of two in 64 .. 2^26.  workspace: NULL, or device memory of at least
 * ttl_tract_density_workspace_bytes(spill_slots, n) bytes (0 for arguments out of range),
 * zeroed once by the caller; every call leaves it zeroed.  With count NULL there is no set
 * and no spill pass: a workspace is checked as always and then neither read nor written.
 * Calls that share a workspace must be ordered (one stream).
 * One wavefront per row, lanes over the segments; open addressing with at most table-size
 * probes, and no insertion once more than half the table is new keys, so a full table ends
 * a row's count and never holds a lane.  No float atomics.  TTL_ERR_INVALID, before any HIP
 * call (but for the LDS above), for a null desc / points / offsets / status, n < 0, bad dims, no map, slots out of
 * range, a workspace without spill_slots or too small; n == 0 is a successful no-op. */
#define TTL_HAS_TRACT_DENSITY 1
#define TTL_DENSITY_MAX_WAVE_SLOTS 8192
typedef struct {
    int32_t dims[3];
    double lin[9];
    int32_t *count;
    int64_t *length_q, *dec_q;
    int32_t *ends;
    int32_t wave_slots;   /* power of two, 64 .. TTL_DENSITY_MAX_WAVE_SLOTS; 0 = default */
    int32_t spill_slots;  /* power of two, or 0 */
    void *workspace;
    size_t workspace_bytes;
} ttl_density_desc;
TTL_API size_t ttl_tract_density_workspace_bytes(int32_t spill_slots, int32_t n_max);
TTL_API int ttl_tract_density(const ttl_density_desc *desc, const float *points,
                              const int64_t *offsets, int32_t n, int32_t *status,
                              void *hip_stream);

/* Bundle profiles (TTL_HAS_BUNDLE_PROFILE): the mean and the spread of a scalar
 * volume at K stations along a bundle -- AFQ's tract profile, scil_bundle_mean_std
 * --per_point.  This project's own statement; the reference has no counterpart.  Input is
 * the ragged layout of ttl_tract_coverage in the corner-origin voxel coordinates of the
 * volume's grid; bundle: device int32 [n], the bundle number of every row
 * (ttl_tractometer_classify's, or any other); n_bundles = B in 1 .. TTL_PROFILE_MAX_BUNDLES,
 * nb_points = K in 2 .. TTL_PROFILE_MAX_POINTS; lin (host double [9], row-major linear part
 * of voxel -> RAS mm) and dims = {X, Y, Z} in host memory.  Floats are read as float64 and
 * all arithmetic is float64 in the written order.
 *
 * Stations.  r_0 .. r_{K-1} of a row are the float32 points ttl_resample_streamlines gives
 * for it at nb_points = K, the same bits (the one resampler, with the cumulative arc
 * length replayed from 64 lane prefixes): equidistant in arc length IN VOXEL UNITS.  On an
 * anisotropic grid they are not equidistant in mm.
 *
 * ttl_bundle_orient.  model: device float32 [B][K][3], a model line per bundle, in the
 * rows' coordinates.  Row s with b = bundle[s] and L points TAKES PART iff 0 <= b < B,
 * L >= 2, every point is finite and every resampled coordinate has |r_kc * scale| < 2^40.
 * Any other row: flip[s] = 0, mdf[s] = NaN, nothing is added.  A row that takes part:
 *   d(a, m)   = |lin (a - m)|: with e = a - m per axis, v_i = (lin_i0 e_0 + lin_i1 e_1) +
 *               lin_i2 e_2, sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2) -- ttl_tract_sample_mean's
 *               segment length of m -> a, without its test for non-finite ends;
 *   D         = (sum_k d(r_k, m_k)) / K,   F = (sum_k d(r_{K-1-k}, m_k)) / K, each sum as
 *               lane partial sums (lane l adds k = l, l + 64, ... in that order) and then
 *               ttl_tract_sample_mean's butterfly;
 *   flip[s]   = F < D, strictly: a tie, or a comparison with a NaN, leaves the row as it is;
 *   mdf[s]    = flip ? F : D, the mean distance to the model in mm;
 *   o_k       = flip ? r_{K-1-k} : r_k;
 *   sum_q[b][k][c] += llrint((double)o_kc * scale) (half to even; the product is exact),
 *   sum_n[b]  += 1.
 * A model with a non-finite entry follows from this: D and F both contain that station, so
 * both are NaN or +Inf, F < D is false, flip is 0, mdf is that non-finite value (NaN for a
 * NaN entry), and the row is still summed.
 *   tolerance against the definition in exact arithmetic, u = 2^-53, A the mean over k of
 *               the distance taken with magnitudes (|lin| and |a - m|, as DESIGN 3.15's
 *               A_s): a distance carries 8 roundings (3.15's segment), a sum of K terms at
 *               most K - 1 on any path, the division one: |D - exact| <= (K + 8) u A, and
 *               the same for F with its own A.  flip is decided when |D - F| exceeds the sum
 *               of the two bounds.
 * sum_q: device int64 [B][K][3], sum_n: device int64 [B], both ADDED TO; flip: device int32
 * [n]; mdf: device double [n].  The centroid of bundle b is sum_q[b] / scale / sum_n[b].
 *
 * ttl_bundle_profile.  volume: device float32 [X * Y * Z], word (x * Y + y) * Z + z.  A row
 * takes part iff 0 <= b < B, L >= 2 and every point is finite.  Station k of the row is o_k
 * = flip[s] != 0 ? r_{K-1-k} : r_k; its value v is ttl_tract_sample_mean's sample s_j at
 * p = o_k with that function's not-sampled rules (the closed volume, edge replicate, a
 * non-finite corner).  A station COUNTS iff it is sampled, |v * scale| < 2^40 and
 * |(v * v) * scale_sq| < 2^40; then
 *   sum_q[b][k]  += llrint(v * scale),
 *   sum_qq[b][k] += llrint((v * v) * scale_sq)   (the square of v, not of the rounded value),
 *   count[b][k]  += 1.
 * All three: device int64 [B][K], ADDED TO.  values: device double [n][K] or NULL; v where
 * the station is sampled (counted or not), NaN elsewhere; rows that take no part all NaN.
 * mean = sum_q / scale / count, variance = sum_qq / scale_sq / count - mean^2.
 *
 * Both: scale (and scale_sq) a power of two in 2^-60 .. 2^60, the rule of
 * ttl_connectome_accumulate_metric.  TTL_ERR_INVALID, before any HIP call, for a null
 * pointer (except values and hip_stream), n < 0, B or K out of range, a dim < 1, a scale
 * that is not such a power of two; n == 0 is a successful no-op.
 *
 * One wavefront per streamline over a capped grid; the row is resampled into the wave's LDS
 * (64 * 8 bytes of prefixes + 12 K bytes of stations, whatever the row's length); the model
 * row is read from global memory by lane k.  The gates of a row (all points finite, every
 * coordinate in range) are wave-wide ballots taken before the first add: a row is added
 * completely or not at all.  Lane k owns stations k, k + 64, ...; a wave takes a contiguous
 * range of the call's rows and keeps its lanes' integer sums in registers while consecutive
 * rows have the same bundle; device-scope 64-bit atomics are issued when the bundle changes
 * and after the wave's last row.  Integer sums: the result is that of one atomic per
 * addend, whatever the flush points, the order or the split of the rows. */
#define TTL_HAS_BUNDLE_PROFILE 1
#define TTL_PROFILE_MAX_POINTS 256
#define TTL_PROFILE_MAX_BUNDLES 64
TTL_API int ttl_bundle_orient(const float *points, const int64_t *offsets, int32_t n,
                              const int32_t *bundle, int32_t n_bundles, int32_t nb_points,
                              const float *model, const double *lin, double scale,
                              int32_t *flip /*[n]*/, double *mdf /*[n]*/, int64_t *sum_q,
                              int64_t *sum_n, void *hip_stream);
TTL_API int ttl_bundle_profile(const float *points, const int64_t *offsets, int32_t n,
                               const int32_t *bundle, const int32_t *flip, int32_t n_bundles,
                               int32_t nb_points, const float *volume, const int32_t *dims,
                               double scale, double scale_sq, int64_t *sum_q, int64_t *sum_qq,
                               int64_t *count, double *values /*[n][K] or NULL*/,
                               void *hip_stream);

/* Bundle recognition (TTL_HAS_BUNDLE_RECOGNIZE): for every streamline the
 * nearest of M model lines by the minimum-average-direct-flip distance (MDF), the direction
 * and the nearest model of another bundle -- the assignment step of RecoBundles /
 * QuickBundles.  This project's own statement; the reference has no counterpart.  Input is
 * the ragged layout and the coordinates of ttl_bundle_orient; models: device float32
 * [M][K][3] in the rows' coordinates, n_models = M in 1 .. TTL_RECOGNIZE_MAX_MODELS,
 * nb_points = K in 2 .. TTL_PROFILE_MAX_POINTS; label: device int32 [M], the bundle of every
 * model, any values (negative and repeated ones too), or NULL: label_m = m; lin: host
 * double [9] as above.
 *
 * Row s with L points TAKES PART iff L >= 2 and every point is finite (no fixed-point gate:
 * nothing is summed into integers).  Its stations r_0 .. r_{K-1} are ttl_bundle_orient's,
 * the same bits.  For a row that takes part and model m, with ttl_bundle_orient's d(a, b):
 *   D_m       = (sum_k d(r_k, m_k)) / K,   F_m = (sum_k d(r_{K-1-k}, m_k)) / K, each sum
 *               sequential: ((d_0 + d_1) + d_2) + ... in increasing k from 0.0 + d_0, which
 *               is d_0 -- K - 1 roundings, then the division;
 *   f_m       = F_m < D_m, strictly: a tie, or a comparison with a NaN, gives 0;
 *   delta_m   = f_m ? F_m : D_m.
 *   tolerance ttl_bundle_orient's, unchanged: |D_m - exact| <= (K + 8) u A, F_m with its own
 *               A; f_m is decided when |D_m - F_m| exceeds the sum of the two bounds.
 * A model with a non-finite station has D_m and F_m both NaN or +Inf, as there.
 *   best[s]      = the m of the smallest delta_m that is not a NaN; among equal delta_m the
 *                  lowest m.  +Inf may win.
 *   flip[s]      = f_best,   mdf[s] = delta_best;
 *   runner_up[s] = the smallest delta_m that is not a NaN over the m with label_m !=
 *                  label_best; NaN when there is none.
 * A row that takes no part, or for which every delta_m is a NaN: best = -1, flip = 0, mdf =
 * NaN, runner_up = NaN.  best, flip: device int32 [n]; mdf: device double [n]; runner_up:
 * device double [n] or NULL.  Every output is written for every row.  The minimum of
 * doubles is exact and the sums are per (row, model) pair, so the outputs are the same bits
 * whatever the order of the rows, the split into calls or, with indices mapped back and no
 * tie, the order of the models.
 *
 * TTL_ERR_INVALID, before any HIP call, for a null pointer (except label, runner_up and
 * hip_stream), n < 0, M or K out of range; n == 0 is a successful no-op.
 *
 * A workgroup of 256 threads takes 8 consecutive rows, 2 per wave, resampled into the
 * wave's LDS (64 * 8 bytes of prefixes + 2 * 12 K bytes of stations); the models pass
 * through an LDS tile of 64 models x min(K, 32) stations, station-major ([k][c][model], 65
 * words per line), shared by the 4 waves: a lane owns a model, keeps the 2 sums of each of
 * its wave's 2 rows in registers across the station chunks, and every model station read
 * feeds 4 distances.  Lane states (nearest, nearest of another label) are merged by a
 * butterfly of the lexicographic (delta, m) minimum. */
#define TTL_HAS_BUNDLE_RECOGNIZE 1
#define TTL_RECOGNIZE_MAX_MODELS 4096
TTL_API int ttl_bundle_recognize(const float *points, const int64_t *offsets, int32_t n,
                                 const float *models /*[M][K][3]*/,
                                 const int32_t *label /*[M] or NULL*/, int32_t n_models,
                                 int32_t nb_points, const double *lin /*host [9]*/,
                                 int32_t *best /*[n]*/, int32_t *flip /*[n]*/,
                                 double *mdf /*[n]*/, double *runner_up /*[n] or NULL*/,
                                 void *hip_stream);

/* Streamline-based linear registration, the cost (TTL_HAS_BUNDLE_REGISTER):
 * the bundle-minimum distance (BMD; Garyfallidis 2015) between A fixed and B moving lines
 * under each of T candidate transforms, in one launch -- the function and, by a central
 * difference, the gradient that a quasi-Newton optimiser asks for.  This project's own
 * statement; the reference has no counterpart.  fixed: device float32 [A][K][3], moving:
 * device float32 [B][K][3], stations already resampled to nb_points = K in 2 ..
 * TTL_PROFILE_MAX_POINTS, both in the corner-origin voxel coordinates of one grid;
 * n_fixed = A and n_moving = B in 1 .. TTL_REGISTER_MAX_LINES; xf: DEVICE double [T][12],
 * n_xf = T in 1 .. TTL_REGISTER_MAX_TRANSFORMS, xf[t] a row-major 3 x 4 affine x in those
 * coordinates; lin: host double [9] as above.  Floats are read as float64 and all
 * arithmetic is float64 in the written order, nothing fused.
 *
 * Station k of moving line j under transform t, per axis c, NOT rounded to float32:
 *   m'_c      = ((x_c0 m_0 + x_c1 m_1) + x_c2 m_2) + x_c3.
 * A fixed line TAKES PART iff its K stations are finite; a moving line takes part under t
 * iff its K stations are finite and so is every m' of it.  A transform with a non-finite
 * entry leaves no moving line that takes part.  For a fixed line i and a moving line j that
 * take part, with ttl_bundle_orient's d(a, b) and ttl_bundle_recognize's sums (sequential in
 * k from 0.0 + d_0, then the division), the fixed line's stations a_k in the place of the
 * row's and m'_k in the place of the model's:
 *   D         = (sum_k d(a_k, m'_k)) / K,   F = (sum_k d(a_{K-1-k}, m'_k)) / K,
 *   delta_ij  = F < D (strictly) ? F : D.
 *   row_min[t][i] = the smallest delta_ij that is not a NaN over the j that take part,
 *   col_min[t][j] = the smallest delta_ij that is not a NaN over the i that take part;
 *               NaN (0x7ff8000000000000) for a line that takes no part or has no such
 *               partner.  A minimum of doubles is exact, so both are the same bits
 *               whatever the order of the lines or the split of the T transforms into calls.
 *   cost[t]   = 0.25 * (s * s), s = mean(row_min[t]) + mean(col_min[t]), each mean over the
 *               entries that are not NaN: lane partial sums (lane l of 64 adds entries l,
 *               l + 64, ... in that order), ttl_tract_sample_mean's butterfly, the division
 *               by their number; NaN when either side has none.  cost depends on the order
 *               of the lines through these sums only.
 *   tolerance against the definition in exact arithmetic, u = 2^-53, magnitudes as for
 *               ttl_bundle_orient: a coordinate of m' carries at most 4 roundings on any
 *               path (a product and three adds), stated with room for the higher orders as
 *               |m'_c - exact| <= 6 u M_c, M_c = (|x_c0||m_0| + |x_c1||m_1|) + |x_c2||m_2| +
 *               |x_c3|; d is 1-Lipschitz in |lin| e, so with G the mean over k of
 *               |(|lin| M_k)| and A the mean over k of the distance taken with magnitudes,
 *               |D - exact| <= b_D = (K + 8) u A + 6 u G, F with its own A: delta_ij lies in
 *               [min(D - b_D, F - b_F), min(D + b_D, F + b_F)] of the exact D and F, and
 *               row_min and col_min between the minima of those lower and of those upper
 *               ends over their pairs, an interval of width w.  A mean of n entries
 *               carries at most ceil(n / 64) + 6 roundings: with e_r = mean(w) + (ceil(A /
 *               64) + 6) u mean(row_min), e_c likewise and e_s = e_r + e_c + u s,
 *               |cost - exact| <= (2 s e_s + e_s e_s) / 4 + 2 u cost.
 * row_min: device double [T][A]; col_min: device double [T][B]; cost: device double [T];
 * every output is written for every t.
 *
 * TTL_ERR_INVALID, before any HIP call, for a null pointer (except hip_stream), A, B, T or
 * K out of range.
 *
 * Three stream-ordered steps: col_min is set to the all-ones pattern, which is above the
 * bits of every distance (distances are +0 or larger: their order as doubles is their
 * order as unsigned integers); a workgroup of 256 threads takes 8 consecutive fixed lines
 * of one transform, 2 per wave, their stations in the wave's LDS (2 * 12 K bytes); the
 * moving set passes through an LDS tile of 64 lines x min(K, 32) float64 stations (16 for K
 * > 128), station-major ([k][c][line], 65 doubles per line), transformed while it is
 * staged; a lane owns a moving line and keeps the 2 sums of each of its wave's 2 fixed
 * lines across the station chunks.  row_min is a butterfly of the lanes' running minima and
 * a plain store; col_min is the minimum over the 4 waves in LDS and one 64-bit atomic
 * unsigned minimum per moving line and workgroup.  A closing launch of one wave per
 * transform turns the columns nothing lowered into the NaN and computes cost. */
#define TTL_HAS_BUNDLE_REGISTER 1
#define TTL_REGISTER_MAX_TRANSFORMS 64
#define TTL_REGISTER_MAX_LINES 1048576
TTL_API int ttl_bundle_register_cost(const float *fixed /*[A][K][3]*/, int32_t n_fixed,
                                     const float *moving /*[B][K][3]*/, int32_t n_moving,
                                     int32_t nb_points, const double *xf /*device [T][12]*/,
                                     int32_t n_xf, const double *lin /*host [9]*/,
                                     double *row_min /*[T][A]*/, double *col_min /*[T][B]*/,
                                     double *cost /*[T]*/, void *hip_stream);

/* OracleReward's sparse bonus (oracle_reward.py:84-93) for the rows of
 * ttl_env_stopped(): term[0 .. n_active) = 0, then term[row_q] = bonus where
 * scores[q] > 0.5 (q < n_scored <= n_stopped; the rest was not scored), and
 * reward[row_q] += term[row_q]. */
TTL_API int ttl_oracle_bonus(const float *scores, int32_t n_scored, const int32_t *stop_list,
                             int32_t n_stopped, double bonus, int32_t n_active, double *term,
                             double *reward, void *hip_stream);

/* Ragged pack of tracked streamlines (ABI v8), the device side of
 * TrackingEnvironment.get_streamlines (tracking_env.py:263-284) and of the
 * multi-GPU collate: history [n] rows of row_pitch floats (the env's
 * `streamlines` buffer, row_pitch = 3 * (max_nb_steps + 1)); keep[i] points of
 * row i (int64; lengths minus the point a CURVATURE / MASK stop drops) are
 * copied to points_out + 3 * offsets[i] (offsets = exclusive prefix of keep,
 * int64).  One wave per streamline, coalesced; device pointers. */
TTL_API int ttl_pack_streamlines(const float *history, int64_t row_pitch, const int64_t *keep,
                         const int64_t *offsets, int32_t n, float *points_out,
                         void *hip_stream);

/* The tracker's output stage (ABI v13): length filter, optional compression
 * and ragged pack of a finished batch, on the env's buffers in place.  Device pointers;
 * n == 0 is a successful no-op.
 *
 * ttl_tract_select, one wavefront per row of history ([n] rows of row_pitch floats, as
 * for ttl_pack_streamlines; T = row_pitch / 3 points):
 *  1. keep = lengths[i] - 1 if flags[i] has TTL_FLAG_CURVATURE or TTL_FLAG_MASK, else
 *     lengths[i] (clamped to [0, T]).
 *  2. arc = sum over the keep - 1 segments of sqrt(dx*dx + dy*dy + dz*dz) in float64, d =
 *     the float32 difference of consecutive points widened to float64, squares added left
 *     to right.  Lane l adds segments l, l + 64, ... in order and a fixed butterfly adds
 *     the 64 partial sums: the bits depend on the points and keep alone.  keep < 2 gives
 *     0.  The row is accepted iff min_arc <= arc <= max_arc.
 *  3. An accepted row with tol_error > 0 and keep > 2 is compressed greedily
 *     (tractogram.compress_streamline): prev = 0; for nxt = 2 .. keep-1: a = p[prev], b =
 *     p[nxt] in float64, ab = b - a, L = sqrt(ab.x^2 + ab.y^2 + ab.z^2); the chord is
 *     admissible iff L <= max_segment_length and every q = p[j] - a, prev < j < nxt, has
 *     sqrt(|q - t ab|^2) <= tol_error with t = clamp((q . ab) / (L L), 0, 1) (|q| <=
 *     tol_error when L == 0); if it is not, point nxt-1 is kept and prev = nxt-1.  Points
 *     0 and keep-1 are always kept.  The lanes test the interior points of one chord, 64
 *     at a time, and a ballot decides it.  No operation is fused.  With tol_error == 0, or
 *     keep <= 2, every kept point survives.
 *  Out: counts[i] = surviving points (0 for a rejected row), accepted[i] = 0 / 1, and
 *  mask[i][ttl_tract_mask_words(row_pitch)]: bit j & 63 of word j >> 6 set iff point j
 *  survives (all zero for a rejected row).  Rows of up to ttl_tract_stage_points() points
 *  are staged in the LDS and read from memory once; longer rows are read in place.
 *
 * ttl_tract_emit, one wavefront per row, after the caller's inclusive prefix sums
 * count_ends / accept_ends (int64) over counts / accepted: accepted row i is output row k
 * = accept_ends[i] - 1; counts_out[k] = counts[i], rows_out[k] = i, and its survivors go,
 * in order, to points_out + 3 * (count_ends[i] - counts[i]).  points_out holds
 * count_ends[n-1] points, counts_out and rows_out accept_ends[n-1] entries. */
TTL_API int32_t ttl_tract_mask_words(int64_t row_pitch);
TTL_API int32_t ttl_tract_stage_points(void);
TTL_API int ttl_tract_select(const float *history, int64_t row_pitch, const int32_t *lengths,
                             const int32_t *flags, int32_t n, double min_arc, double max_arc,
                             double tol_error, double max_segment_length, int32_t *counts,
                             int32_t *accepted, uint64_t *mask, void *hip_stream);
TTL_API int ttl_tract_emit(const float *history, int64_t row_pitch, int32_t n,
                           const int32_t *counts, const int32_t *accepted,
                           const int64_t *count_ends, const int64_t *accept_ends,
                           const uint64_t *mask, float *points_out, int64_t *counts_out,
                           int32_t *rows_out, void *hip_stream);

/* The file body of a batch, built by the pack (TTL_HAS_TRACT_FILE).  Both
 * tractogram formats are flat streams of little-endian 4-byte words whose records do not
 * depend on where they sit in the file, so the bodies of successive batches (or ranks)
 * concatenate.  ttl_tract_emit_file takes ttl_tract_emit's inputs and writes, for accepted
 * input row i (output row k = accept_ends[i] - 1, b = count_ends[i] - counts[i] points
 * before it, P = n_props):
 *   TTL_TRACT_FILE_TRK  at word k (1 + P) + 3 b: counts[i] as int32, the converted points,
 *                       then for P == 3 float32(seeds[i][c] - 0.5), c = 0..2, the
 *                       subtraction in float64;
 *   TTL_TRACT_FILE_TCK  at word 3 (b + k): the converted points, then three words
 *                       0x7fc00000 (a float32 NaN triplet).  The format has no
 *                       properties: n_props is validated and otherwise ignored, and the
 *                       closing inf triplet belongs to the file, not to a batch.
 * A point p (float32 x, y, z) is converted by the steps the descriptor switches on, in
 * this order, each in plain IEEE arithmetic with nothing fused:
 *   pre     v_c = float32(float64(float32(p_c + 0.5f)) * pre_scale), widened to float64
 *           (without it v_c = float64(p_c));
 *   maps    n_maps <= 2 affine maps m, 3 x 4 row-major float64, one after the other:
 *           out_i = ((x m[i][0] + y m[i][1]) + z m[i][2]) + m[i][3];
 *   post    v_i = (v_i + 0.5) * post_scale[i];
 * and v is rounded to float32 once.  seeds is device f64 [n][3], indexed by input row, or
 * NULL; desc is host memory; words_out holds ttl_tract_file_words(format, n_props,
 * accept_ends[n-1], count_ends[n-1]) words and is written with 4-byte stores only (record
 * starts are 4-byte aligned).  One wavefront per row; one lane converts one point.
 * TTL_ERR_INVALID, before any launch, for an unknown format, n_props other than 0 or 3,
 * n_props == 3 without seeds, or n_maps outside [0, 2]; ttl_tract_file_words returns -1
 * for the first two.  n == 0 is a successful no-op, and so is a batch without an accepted
 * row (words_out may then be NULL). */
#define TTL_HAS_TRACT_FILE 1
#define TTL_TRACT_FILE_TRK 0
#define TTL_TRACT_FILE_TCK 1
typedef struct ttl_tract_file_desc {
    int32_t format;       /* TTL_TRACT_FILE_* */
    int32_t n_props;      /* 0 or 3 (the seed) */
    int32_t has_pre;
    int32_t n_maps;
    int32_t has_post;
    int32_t reserved;     /* 0 */
    double pre_scale;
    double maps[2][12];
    double post_scale[3];
} ttl_tract_file_desc;
TTL_API int64_t ttl_tract_file_words(int32_t format, int32_t n_props, int64_t k, int64_t M);
TTL_API int ttl_tract_emit_file(const float *history, int64_t row_pitch, int32_t n,
                                const int32_t *counts, const int32_t *accepted,
                                const int64_t *count_ends, const int64_t *accept_ends,
                                const uint64_t *mask, const double *seeds,
                                const ttl_tract_file_desc *desc, uint32_t *words_out,
                                void *hip_stream);

TTL_API const char *ttl_last_error(void);
TTL_API uint32_t ttl_abi_version(void);
/* sizeof(ttl_env_desc) as compiled: a binding checks its own struct against it */
TTL_API size_t ttl_env_desc_size(void);

#ifdef __cplusplus
}
#endif
#endif /* TTL_HIP_H */
