// ttl_internal.h -- shared by the translation units of libttl_hip.so (not
// part of the ABI).
#ifndef TTL_INTERNAL_H
#define TTL_INTERNAL_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ttl_hip.h"

// records the message returned by ttl_last_error() (thread local) and
// returns `code`
int ttl_detail_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail ttl_detail_fail

#define HIP_TRY(expr)                                                        \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess)                                                \
            return fail(TTL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr int TTL_BLOCK = 256;   // threads per workgroup of every kernel

// Device-side view of the environment (a flat copy of the descriptor).
struct EnvParams {
    int mode;
    int sh_dim[3];
    int n_coef;
    int coef_pitch;
    const float *sh;
    float sh_shift;
    int sh_brick;          // TTL_SH_BRICK4 record order (see ttl_hip.h)
    unsigned sh_sx, sh_sy; // records per unit of x / y: linear Y*Z, Z; bricked: per brick step
    int mask_dim[3];
    const double *mask_coef;
    const uint8_t *mask_cls;  // per-cell class (see k_mask_classes) or null
    double mask_thr;
    int peaks_dim[3];
    const float *peaks;
    int compute_reward;
    float align_w;
    int n_dirs;
    int max_nb_steps;
    double step64;
    float step32;
    float radius;
    int curv_enabled;
    float curv_dot_max;
    float *hist;
    int *flags;
    int *lengths;
    uint8_t *dones;
    // workspace
    uint8_t *stop;     // [n_max] 1 = stopped in the last step
    float *head;       // [n_max][4] newest point of every active row (row order), .w = bits of idx[row]
    int *pos_dest;     // [n_max][2] {surv_pos, row_dest} of every active row, packed for k_proc_scatter
    float *last2;      // [n_max][8] per streamline id: {p[L-2], pad, p[L-1], pad}, the two newest points
    int *rank;         // [n_max] survivors before this row inside its block
    int *surv_pos;     // [n_max] position among survivors, -1 if stopped
    int *row_dest;     // [n_max] state row written for this active row
    int *stop_list;    // [n_max][2] {active row, streamline id} of the rows that stopped in the last step, in row order
    int *block_counts; // [ceil(n_max/BLOCK)] survivors per block
    int *proc_rank;    // [n_max] rank of a kept slot of the processing order
    int *proc_counts;  // [ceil(n_max/BLOCK)] kept slots per block
    float *slot_head;  // [n_max][4] per slot of the processing order: newest point, .w = bits of idx[row]
    int *slot_dest;    // [n_max] per slot of the processing order: row_dest[row]
    int slot_rec;      // the gather reads the slot records (0: resolves proc -> idx/row_dest/head itself)
    int store_flavour; // cache policy of the state-row stores (TTL_STORE_FLAVOUR, see store16)
    int xcd_remap;     // XCD-contiguous ranges of the processing order (TTL_XCD_REMAP)
    int xcd_rot;       // XCD x gathers range (x + xcd_rot) & 7 of the processing order
    int *counts;       // {n_continue, n_stopped}; 64 ints: the free-running step's words live here too
    int fuse_max_rows; // largest batch of the one-launch step tail (TTL_FUSE_MAX_ROWS, <= TTL_FUSE_MAX_BLOCKS * 256)
    int persist_rows;  // gathers of at most this many rows run as one resident round (TTL_GATHER_PERSIST_ROWS, 0 = off)
};

// the one-launch tail scans at most this many per-block counts (one wave, four per lane)
constexpr int TTL_FUSE_MAX_BLOCKS = 256;

// free-running step (ttl_env_freerun_*): int offsets into EnvParams::counts of
// {n_active, length, cur, steps done} -- live (between steps) and the snapshot
// a step works from
constexpr int TTL_FR_LIVE = 8;
constexpr int TTL_FR_SNAP = 16;
// ... and of the keyed-noise record of a free-running episode (56 bytes, 8-byte
// aligned: counts is 256-byte aligned), written by ttl_env_freerun_begin
constexpr int TTL_FR_NOISE = 32;

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): the counter-based
// generator of the keyed action noise (ttl_hip.hip) and of the fODF policy's
// uniforms (ttl_odf_policy.hip); tests/ref_noise.py restates it in NumPy.
__device__ __forceinline__ void philox4x32_10(uint32_t &c0, uint32_t &c1, uint32_t &c2,
                                              uint32_t &c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// What a policy kernel of a free-running step reads (ttl_env_freerun_*): the live
// words {n_active, length, cur, steps done} and the two continue_idx buffers
// (cur picks); cap = rows at ttl_env_freerun_begin, 0: not free-running
struct FreerunView {
    const int *live, *idx_a, *idx_b;
    int cap;
};
void ttl_detail_freerun_view(const ttl_env *env, FreerunView *out);

// Record index of voxel (x, y, z) = vox_x(x) + vox_y(y) + vox_z(z), for both
// record orders (separable, so the gather keeps per-axis partial offsets).
__device__ __forceinline__ unsigned vox_x(const EnvParams &P, int x) {
    return P.sh_brick ? (unsigned)(x >> 2) * P.sh_sx + (unsigned)(x & 3) * 16u
                      : (unsigned)x * P.sh_sx;
}
__device__ __forceinline__ unsigned vox_y(const EnvParams &P, int y) {
    return P.sh_brick ? (unsigned)(y >> 2) * P.sh_sy + (unsigned)(y & 3) * 4u
                      : (unsigned)y * P.sh_sy;
}
__device__ __forceinline__ unsigned vox_z(const EnvParams &P, int z) {
    return P.sh_brick ? (unsigned)(z >> 2) * 64u + (unsigned)(z & 3) : (unsigned)z;
}

// ---------------------------------------------------------------------------
// What every step tail (k_prefix, k_tail, k_prefix_state[_fr]) does once the
// scan of the per-block survivor counts has given a row its position `pos`
// among the `total` survivors.
// ---------------------------------------------------------------------------
// State row of active row `row`: its own under TTL_ORDER_ACTIVE; under
// TTL_ORDER_PARTITION the survivors first, the stopped rows behind them, both
// in row order
__device__ __forceinline__ int step_row_dest(int order, int row, bool stop, int pos, int total) {
    int dest = row;
    if (order == TTL_ORDER_PARTITION) dest = stop ? total + (row - pos) : pos;
    return dest;
}

// The row map of active row `row` (streamline g): continue_idx of the next
// step and the active-row -> state-row map.  Returns the state row.
__device__ __forceinline__ int step_map_row(const EnvParams &P, int row, int g, bool stop,
                                            int pos, int total, int order, int n_pts,
                                            int *idx_next) {
    const int dest = step_row_dest(order, row, stop, pos, total);
    if (!stop) idx_next[pos] = g;
    // ORDER_PARTITION has no separate harvest kernel: record the final length
    // of the streamlines that just stopped here (tracking_env.py:236)
    if (stop && order == TTL_ORDER_PARTITION) P.lengths[g] = n_pts;
    P.surv_pos[row] = stop ? -1 : pos;
    // the rows that stopped, compacted in row order (ttl_env_stopped: the
    // oracle reward scores exactly these, oracle_reward.py:78-90)
    if (stop) *reinterpret_cast<int2 *>(P.stop_list + 2 * (size_t)(row - pos)) = int2{row, g};
    P.row_dest[row] = dest;
    return dest;
}

// {n_continue, n_stopped} of the step, by one thread of the launch: into device
// memory and, when the caller's pinned buffer is device-visible (host_word),
// straight into it with the step's sequence number last -- the host polls that
// word (await_counts: it reads the counts only after it has seen `seq`, hence
// the release) and can queue the next step while the state gather of this one
// is still running
__device__ __forceinline__ void step_publish_counts(const EnvParams &P, int total, int n_active,
                                                    int *host_word, int seq) {
    P.counts[0] = total;
    P.counts[1] = n_active - total;
    if (host_word) {
        __hip_atomic_store(host_word + 0, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_word + 1, n_active - total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_word + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Stable survivor ranks of one 256-thread block: 64-bit ballot per wavefront,
// popcount of the lanes below, then the 4 wave totals through LDS.  Writes
// rank[i] (survivors before row i inside the block) and the block's count.
__device__ __forceinline__ void block_ranks(int *__restrict__ rank_out,
                                            int *__restrict__ counts_out, int i,
                                            bool active, bool keep) {
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    __shared__ int wave_total[TTL_BLOCK / 64];
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < TTL_BLOCK / 64; ++w)
        if (w < wave) before += wave_total[w];
    if (active) rank_out[i] = before + below;
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < TTL_BLOCK / 64; ++w) tot += wave_total[w];
        counts_out[blockIdx.x] = tot;
    }
}

__device__ __forceinline__ void block_survivor_ranks(const EnvParams &P, int i,
                                                     bool active, bool keep) {
    block_ranks(P.rank, P.block_counts, i, active, keep);
}

// ---------------------------------------------------------------------------
// One wavefront per row (ttl_resample.hip, ttl_coverage.hip, ttl_peaks.hip,
// ttl_tract.hip): the lanes of a wave hand values to each other through LDS
// that no other wave touches.
// ---------------------------------------------------------------------------
// Orders this wave's LDS accesses before the barrier against those behind it
// (the LDS executes one wave's instructions in order; this keeps the compiler
// from moving them across)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// body(row) for the rows of this wave: row = its number in the grid, then in
// steps of the grid's waves (a `continue` of the loop is a `return` of body)
template <class F>
__device__ __forceinline__ void wave_rows(int n, F body) {
    const int waves = (TTL_BLOCK / 64) * gridDim.x;
    for (int row = blockIdx.x * (TTL_BLOCK / 64) + (threadIdx.x >> 6); row < n; row += waves)
        body(row);
}

// ... and the grid of such a launch: a wave for each of n rows, at most `cap` workgroups
inline unsigned ttl_detail_wave_grid(long long n, int cap) {
    const long long want = (n + (TTL_BLOCK / 64) - 1) / (TTL_BLOCK / 64);
    return (unsigned)(want < cap ? want : cap);
}

// ---------------------------------------------------------------------------
// The voxel walk of a streamline (ttl_coverage.hip, ttl_tractometer.hip),
// stated once: include/ttl_hip.h, ttl_tract_coverage.
// ---------------------------------------------------------------------------
struct WalkDims {
    int d[3];
};

// visit(x, y, z) when the voxel lies inside the volume
template <class Visit>
__device__ __forceinline__ void walk_visit(const WalkDims &D, long long x, long long y,
                                           long long z, Visit &visit) {
    if (x < 0 || y < 0 || z < 0 || x >= D.d[0] || y >= D.d[1] || z >= D.d[2]) return;
    visit((int)x, (int)y, (int)z);
}

// crossing order: increasing t, the lower axis first on ties
__device__ inline bool walk_before(double t0, int ax0, double t1, int ax1) {
    return t0 < t1 || (t0 == t1 && ax0 < ax1);
}

// floor of a finite coordinate, clamped to [-1, dim]: every test below (inside at the
// start, first / last in-volume plane, leaving the volume) sees the same answer as with
// the unclamped index, and the value fits an int
__device__ inline long long walk_clamped_floor(double v, int dim) {
    return (long long)fmin(fmax(floor(v), -1.0), (double)dim);
}

// The voxel of a streamline's first point: visited when the point is finite and inside.
template <class Visit>
__device__ __forceinline__ void walk_first_point(const float *__restrict__ p, const WalkDims &D,
                                                 Visit visit) {
    const double x = p[0], y = p[1], z = p[2];
    if (isfinite(x) && isfinite(y) && isfinite(z))
        walk_visit(D, walk_clamped_floor(x, D.d[0]), walk_clamped_floor(y, D.d[1]),
                   walk_clamped_floor(z, D.d[2]), visit);
}

// The walk of segment a -> b (ttl_hip.h): the voxel entered at every integer-plane
// crossing, crossings in increasing t = (plane - a_i) / d_i (float64, straight from the
// formula), the lower axis first on ties.  Only the crossings during which all three
// indices stay inside the volume are visited: on each axis the planes whose crossing
// leaves that index inside form one run; the in-volume crossings are the part of the
// merged order after the last axis enters (E) and up to the first axis leaving (X).  The
// runs start at E by binary search (t is monotone along a run), so the work is the
// voxels visited plus O(log dim).  visit(x, y, z, t) gets the in-volume voxels in walk
// order, each with the t of the crossing that enters it.  Returns the t at which the last
// voxel visited is left when the walk ends: X's, or 1 when no axis leaves the volume (the
// pieces of ttl_tract_density; 1 as well when nothing is visited).
template <class Visit>
__device__ double walk_segment_pieces(const float *__restrict__ pa, const float *__restrict__ pb,
                                      const WalkDims &D, Visit visit) {
    double a[3], b[3], d[3];
    long long idx[3], cur[3], left[3];
    int step[3];
    double et = -INFINITY, xt = INFINITY;      // entry E / exit X: (t, axis)
    int eax = -1, xax = 3;
    for (int i = 0; i < 3; ++i) {
        const double ai = pa[i], bi = pb[i];
        if (!isfinite(ai) || !isfinite(bi)) return 1.0;
        a[i] = ai;
        b[i] = bi;
        d[i] = bi - ai;
    }
    for (int i = 0; i < 3; ++i) {
        const int dim = D.d[i];
        const long long va = walk_clamped_floor(a[i], dim), vb = walk_clamped_floor(b[i], dim);
        const bool inside = va >= 0 && va < dim;
        idx[i] = va;
        left[i] = 0;
        if (va == vb) {
            if (!inside) return 1.0;           // this index never enters the volume
            continue;
        }
        long long first, last, exit_plane = -2;
        if (vb > va) {                         // planes va+1 .. vb, index after = plane
            step[i] = 1;
            first = max(va + 1, 0LL);
            last = min(vb, (long long)dim - 1);
            if (vb >= dim) exit_plane = dim;
        } else {                               // planes va .. vb+1, index after = plane - 1
            step[i] = -1;
            first = min(va, (long long)dim);
            last = max(vb + 1, 1LL);
            if (vb < 0) exit_plane = 0;
        }
        const long long count = (last - first) * step[i] + 1;
        left[i] = count > 0 ? count : 0;
        cur[i] = first;
        if (!inside) {
            if (left[i] == 0) return 1.0;
            const double t = ((double)first - a[i]) / d[i];
            if (walk_before(et, eax, t, i)) {
                et = t;
                eax = i;
            }
        }
        if (exit_plane != -2) {
            const double t = ((double)exit_plane - a[i]) / d[i];
            if (walk_before(t, i, xt, xax)) {
                xt = t;
                xax = i;
            }
        }
    }
    if (eax >= 0) {                            // skip the crossings before E on every axis
        for (int i = 0; i < 3; ++i) {
            if (left[i] == 0) continue;
            long long lo = 0, hi = left[i];    // first position with (t, i) >= E
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                const double t = ((double)(cur[i] + mid * step[i]) - a[i]) / d[i];
                if (walk_before(t, i, et, eax)) lo = mid + 1;
                else hi = mid;
            }
            if (lo > 0) {
                const long long plane = cur[i] + (lo - 1) * step[i];
                idx[i] = step[i] > 0 ? plane : plane - 1;
                cur[i] += lo * step[i];
                left[i] -= lo;
            }
        }
    }
    double tn[3];
    for (int i = 0; i < 3; ++i)
        tn[i] = left[i] ? ((double)cur[i] - a[i]) / d[i] : 0.0;
    for (;;) {
        int m = -1;
        for (int i = 0; i < 3; ++i)
            if (left[i] && (m < 0 || walk_before(tn[i], i, tn[m], m))) m = i;
        if (m < 0 || walk_before(xt, xax, tn[m], m)) break;
        idx[m] = step[m] > 0 ? cur[m] : cur[m] - 1;
        const double t = tn[m];
        auto visit_at = [&](int x, int y, int z) { visit(x, y, z, t); };
        walk_visit(D, idx[0], idx[1], idx[2], visit_at);
        cur[m] += step[m];
        if (--left[m]) tn[m] = ((double)cur[m] - a[m]) / d[m];
    }
    return xax < 3 ? xt : 1.0;
}

// ... and for a visitor that needs no t: visit(x, y, z)
template <class Visit>
__device__ void walk_segment(const float *__restrict__ pa, const float *__restrict__ pb,
                             const WalkDims &D, Visit visit) {
    walk_segment_pieces(pa, pb, D, [&](int x, int y, int z, double) { visit(x, y, z); });
}

// row-major index of voxel (x, y, z)
__device__ __forceinline__ size_t walk_index(const WalkDims &D, int x, int y, int z) {
    return ((size_t)x * (size_t)D.d[1] + (size_t)y) * (size_t)D.d[2] + (size_t)z;
}

// ---------------------------------------------------------------------------
// Statements that several row kernels share, in a namespace of their own: the
// files that keep a Lin or a wave_sum of theirs are not disturbed.
// ---------------------------------------------------------------------------
namespace ttl_shared {
// The arc-length resampling of a row (ttl_resample.hip, ttl_bundle_profile.hip),
// stated once: include/ttl_hip.h, ttl_resample_streamlines.
// Dynamic LDS of a launch whose waves keep `per_wave` bytes each, and this wave's part of it
__host__ __device__ inline size_t wave_lds_bytes(size_t per_wave) {
    return (size_t)(TTL_BLOCK / 64) * ((per_wave + 15) & ~(size_t)15);
}
__device__ __forceinline__ char *wave_lds(size_t per_wave) {
    extern __shared__ __align__(16) char lds_all[];
    return lds_all + (size_t)(threadIdx.x >> 6) * ((per_wave + 15) & ~(size_t)15);
}
// ... and the LDS the workgroup shares, behind the waves' parts
__device__ __forceinline__ char *shared_lds(size_t per_wave) {
    return wave_lds(per_wave) + (size_t)(TTL_BLOCK / 64 - (threadIdx.x >> 6)) *
                                    ((per_wave + 15) & ~(size_t)15);
}

// float64 length of segment j of the float32 points p
template <class I>
__device__ __forceinline__ double seg_len(const float *__restrict__ p, I j) {
    const double dx = (double)p[3 * (j + 1) + 0] - (double)p[3 * j + 0];
    const double dy = (double)p[3 * (j + 1) + 1] - (double)p[3 * j + 1];
    const double dz = (double)p[3 * (j + 1) + 2] - (double)p[3 * j + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// the sum of `local` over the lanes below this one: inclusive Hillis-Steele scan
// over the lanes, minus the lane's own
__device__ __forceinline__ double lanes_below(double local, int lane) {
    double before = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_up(before, off);
        if (lane >= off) before = before + up;
    }
    return before - local;
}

// The cumulative arc length cum[0 .. nseg] of a row, by a blocked scan: lane l owns the
// contiguous segments [l per, (l + 1) per), cum[j + 1] = local_j + before, where local_j
// is the lane's running sum and `before` the sum of the lower lanes.  Two ways to keep it,
// with the same members: build() from the points, at(m) = cum[m], and count_le(target,
// nseg) = #{m in [0, nseg) : cum[m + 1] <= target} as the binary search finds it.
//
// Stored: every value in this wave's LDS.
struct CumStored {
    using Index = int;
    double *cum;                                // [nseg + 1]
    __device__ __forceinline__ void build(const float *__restrict__ p, int nseg, int lane) {
        const int per = (nseg + 63) >> 6;
        const int lo = min(lane * per, nseg), hi = min(lo + per, nseg);
        double local = 0.0;
        for (int j = lo; j < hi; ++j) {
            local = local + seg_len(p, j);
            cum[j + 1] = local;                 // within-block prefix for now
        }
        const double before = lanes_below(local, lane);
        for (int j = lo; j < hi; ++j) cum[j + 1] = cum[j + 1] + before;
        if (lane == 0) cum[0] = 0.0;
    }
    __device__ __forceinline__ double at(int m) const { return cum[m]; }
    __device__ __forceinline__ int count_le(double target, int nseg) const {
        int a = 0, b = nseg;
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (cum[mid + 1] <= target) a = mid + 1;
            else b = mid;
        }
        return a;
    }
};

// Replayed, for rows of any length: LDS holds the 64 exclusive lane prefixes only.  A
// value cum[m] is recomputed on demand by re-walking its owner lane's block, which gives
// the bits CumStored stores (local_j + before).  The target search replays CumStored's
// binary search probe by probe while the interval spans several lane blocks (cum may step
// back by an ulp at a block boundary, where `before` comes from a subtraction); inside
// one block cum is non-decreasing, so the rest of that search is the first m with
// cum[m + 1] > target, found by one walk of the block.
struct CumReplayed {
    using Index = long long;
    double *pre;                                // [64]
    const float *p = nullptr;                   // the row and its segments per lane: build()
    long long per = 1;
    __device__ __forceinline__ void build(const float *__restrict__ points, long long nseg,
                                          int lane) {
        p = points;
        per = nseg > 0 ? (nseg + 63) >> 6 : 1;
        const long long lo = min((long long)lane * per, nseg), hi = min(lo + per, nseg);
        double local = 0.0;
        for (long long j = lo; j < hi; ++j) local = local + seg_len(p, j);
        pre[lane] = lanes_below(local, lane);
    }
    __device__ __forceinline__ double at(long long m) const {
        if (m < 1) return 0.0;
        const long long seg = m - 1, owner = seg / per;
        double local = 0.0;
        for (long long j = owner * per; j <= seg; ++j) local = local + seg_len(p, j);
        return local + pre[owner];
    }
    __device__ __forceinline__ long long count_le(double target, long long nseg) const {
        long long a = 0, b = nseg;
        while (a < b) {
            if (a / per == (b - 1) / per) {     // one block: cum is monotone here
                const long long owner = a / per;
                double acc = 0.0;
                long long first = b;
                for (long long j = owner * per; j < b; ++j) {
                    acc = acc + seg_len(p, j);
                    if (j >= a && acc + pre[owner] > target) {
                        first = j;
                        break;
                    }
                }
                return first;
            }
            const long long mid = (a + b) >> 1;
            if (at(mid + 1) <= target) a = mid + 1;
            else b = mid;
        }
        return a;
    }
};

// One wave resamples the nseg + 1 points p to nb points at equal arc length: 3 nb floats
// to dst (LDS or global), visible to the whole wave on return; `cum` may then be rebuilt.
template <class Cum>
__device__ __forceinline__ void resample_row(Cum cum, const float *__restrict__ p,
                                             typename Cum::Index nseg, int nb, float *dst,
                                             int lane) {
    using Index = typename Cum::Index;
    cum.build(p, nseg, lane);
    wave_sync();
    const double total = cum.at(nseg);
    for (int k = lane; k < nb; k += 64) {
        float x, y, z;
        if (k == nb - 1 || nseg == 0) {         // the last point is kept exactly
            x = p[3 * nseg + 0];
            y = p[3 * nseg + 1];
            z = p[3 * nseg + 2];
        } else {
            const double target = total * ((double)k / (double)(nb - 1));
            const Index j = min(cum.count_le(target, nseg), nseg - 1);
            const double c0 = cum.at(j), c1 = cum.at(j + 1);
            const double den = c1 - c0;
            const double r = den > 0.0 ? (target - c0) / den : 0.0;
            const double ax = p[3 * j + 0], ay = p[3 * j + 1], az = p[3 * j + 2];
            const double bx = p[3 * j + 3], by = p[3 * j + 4], bz = p[3 * j + 5];
            x = (float)(ax + r * (bx - ax));
            y = (float)(ay + r * (by - ay));
            z = (float)(az + r * (bz - az));
        }
        dst[3 * k + 0] = x;
        dst[3 * k + 1] = y;
        dst[3 * k + 2] = z;
    }
    wave_sync();
}

// The trilinear sample and the mm length of a segment (ttl_tract_sample.hip,
// ttl_bundle_profile.hip), stated once: include/ttl_hip.h, ttl_tract_sample_mean.
struct Lin {
    double m[9];
};

// butterfly: a + b == b + a, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// row r of lin applied to d: ((m0 x + m1 y) + m2 z)
__device__ __forceinline__ double lin_row(const Lin &A, int r, const double (&d)[3]) {
    return (A.m[3 * r] * d[0] + A.m[3 * r + 1] * d[1]) + A.m[3 * r + 2] * d[2];
}

__device__ __forceinline__ bool finite3(const double (&c)[3]) {
    return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}

// |lin (c1 - c0)| in mm, 0 when an end is non-finite
__device__ __forceinline__ double segment_mm(const Lin &A, const double (&c0)[3],
                                             const double (&c1)[3]) {
    if (!finite3(c0) || !finite3(c1)) return 0.0;
    const double e[3] = {c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]};
    const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
    return sqrt((vx * vx + vy * vy) + vz * vz);
}

// The trilinear sample at p; false when p is not sampled (ttl_hip.h).  The inside
// test comes before any conversion to an integer; every index is clamped, so no
// load leaves the volume.
__device__ __forceinline__ bool sample_at(const double (&p)[3], const float *__restrict__ volume,
                                          const WalkDims &D, double &value) {
    int lo[3], hi[3];
    double f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(p[k] >= 0.0 && p[k] <= (double)D.d[k])) return false;     // a NaN fails too
        const double u = p[k] - 0.5, i = floor(u);
        f[k] = u - i;
        const int v = (int)i, last = D.d[k] - 1;                        // -1 .. dims - 1
        lo[k] = v < 0 ? 0 : v;
        hi[k] = v + 1 > last ? last : v + 1;
    }
    const double gx = 1.0 - f[0], gy = 1.0 - f[1], gz = 1.0 - f[2];
    double cy[2];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        double cz[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float *line = volume + walk_index(D, a ? hi[0] : lo[0], b ? hi[1] : lo[1], 0);
            const double v0 = line[lo[2]], v1 = line[hi[2]];
            finite = finite && isfinite(v0) && isfinite(v1);
            cz[b] = v0 * gz + v1 * f[2];
        }
        cy[a] = cz[0] * gy + cz[1] * f[1];
    }
    value = cy[0] * gx + cy[1] * f[0];
    return finite;
}

// The minimum-average-direct-flip distance between lines of K stations
// (ttl_bundle_profile.hip, ttl_bundle_recognize.hip, ttl_bundle_register.hip), stated
// once: include/ttl_hip.h, ttl_bundle_orient; DESIGN 3.19.
constexpr unsigned long long QUIET_NAN_BITS = 0x7ff8000000000000ull;
__device__ __forceinline__ double quiet_nan() {
    return __longlong_as_double((long long)QUIET_NAN_BITS);
}

// every point of the row finite: the same answer in every lane
__device__ __forceinline__ bool row_is_finite(const float *__restrict__ p, long long L, int lane) {
    bool bad = false;
    for (long long j = lane; j < L; j += 64) {
        const float *q = p + 3 * j;
        bad |= !isfinite(q[0]) || !isfinite(q[1]) || !isfinite(q[2]);
    }
    return !__ballot(bad);
}

// d(a, m) = |lin (a - m)|: segment_mm's expression for the segment m -> a, without its
// test for non-finite ends (a non-finite station gives a non-finite distance)
__device__ __forceinline__ double distance_mm(const Lin &A, const float *a, double mx, double my,
                                              double mz) {
    const double e[3] = {(double)a[0] - mx, (double)a[1] - my, (double)a[2] - mz};
    const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
    return sqrt((vx * vx + vy * vy) + vz * vz);
}

// From the two K-term sums of a pair of lines, direct (d) and against one reversed (f)
struct Mdf {
    double delta;
    bool flipped;
};
__device__ __forceinline__ Mdf mdf_of(double d, double f, int K) {
    const double D = d / (double)K, F = f / (double)K;
    const bool flipped = F < D;                 // strict: a tie or a NaN keeps the row
    return Mdf{flipped ? F : D, flipped};
}

// The tile walk: every wave meets its ROWS_PER_WAVE rows of K stations in
// `res` with all n_lines lines, MDF_TILE_LINES at a time, through the station-major LDS
// tile [k][c][line] of MDF_TILE_PITCH words per (k, c), a lane owning one line.  The two
// K-term sums of a (row, line) pair stay in registers across the chunks of at most tile_k
// stations: k = 0, 1, .. K - 1 in that order.  Per tile, in every thread: begin(m0) before
// its first barrier, stage(m0, in_tile, k0, kc) fills the tile between the two barriers of
// a chunk, fold(m0, d, f) takes the sums of line m0 + lane.
constexpr int MDF_TILE_LINES = 64;
constexpr int MDF_TILE_PITCH = MDF_TILE_LINES + 1;
template <int ROWS_PER_WAVE, class T, class Begin, class Stage, class Fold>
__device__ __forceinline__ void mdf_tile_walk(const Lin &A, const float *res, int K, int n_lines,
                                              const T *tile, int tile_k, Begin begin, Stage stage,
                                              Fold fold) {
    const int lane = threadIdx.x & 63;
    for (int m0 = 0; m0 < n_lines; m0 += MDF_TILE_LINES) {
        const int in_tile = min(MDF_TILE_LINES, n_lines - m0);
        begin(m0);
        double d[ROWS_PER_WAVE], f[ROWS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) d[r] = f[r] = 0.0;
        for (int k0 = 0; k0 < K; k0 += tile_k) {
            const int kc = min(tile_k, K - k0);
            __syncthreads();                    // the tile before this one has been read
            stage(m0, in_tile, k0, kc);
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
                const T *t = tile + 3 * kk * MDF_TILE_PITCH + lane;
                const double mx = t[0], my = t[MDF_TILE_PITCH], mz = t[2 * MDF_TILE_PITCH];
                const int k = k0 + kk;
#pragma unroll
                for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                    const float *row = res + (size_t)r * 3 * K;
                    d[r] = d[r] + distance_mm(A, row + 3 * k, mx, my, mz);
                    f[r] = f[r] + distance_mm(A, row + 3 * (K - 1 - k), mx, my, mz);
                }
            }
        }
        fold(m0, d, f);
    }
}
}  // namespace ttl_shared

// ttl_resample.hip: the one place that reserves dynamic LDS.  Static + dynamic
// LDS of `kernel` against what the device gives a workgroup, BEFORE the launch:
// the runtime does not reject a launch that asks for more -- the queue aborts.
// room->fits = false: nothing was set, the caller refuses in its own words.
// Otherwise hipFuncAttributeMaxDynamicSharedMemorySize is raised when the call
// needs more than any before it.  What the kernel and the device report is read
// once per thread, device and kernel (callers are on the training step's path).
struct LdsRoom {
    size_t fixed, limit;   // the kernel's static LDS, the device's limit per workgroup
    bool fits;
};
int ttl_detail_reserve_lds(const void *kernel, size_t dynamic, LdsRoom *room);
// ... for the entry `who` of a kernel whose LDS grows with its nb_points stations
inline int ttl_detail_reserve_stations(const void *kernel, size_t dynamic, const char *who,
                                       int nb_points) {
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds(kernel, dynamic, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "%s: %d stations exceed the LDS", who, nb_points);
    return TTL_OK;
}

// the kernels' Lin (ttl_shared's, or a file's own) of the ABI's 9 row-major doubles
template <class L>
inline L ttl_detail_lin(const double *lin) {
    L A;
    for (int i = 0; i < 9; ++i) A.m[i] = lin[i];
    return A;
}

// a fixed-point scale is a finite power of two in 2^-60 .. 2^60: frexp gives exactly 0.5,
// and (0.5, e) is 2^(e - 1)
inline bool ttl_detail_bad_scale(double scale) {
    int exponent = 0;
    return !std::isfinite(scale) || std::frexp(scale, &exponent) != 0.5 || exponent - 1 < -60 ||
           exponent - 1 > 60;
}

// records of the packed SH volume (padding records of the bricked order included)
inline size_t ttl_detail_sh_records(const EnvParams &P) {
    if (!P.sh_brick) return (size_t)P.sh_dim[0] * P.sh_dim[1] * P.sh_dim[2];
    return (size_t)((P.sh_dim[0] + 3) / 4) * ((P.sh_dim[1] + 3) / 4) *
           ((P.sh_dim[2] + 3) / 4) * 64;
}

// ---------------------------------------------------------------------------
// Second half of the in-step re-bucket (TTL_ORDER_INSTEP), one workgroup of
// TTL_BLOCK threads for TTL_INSTEP_CHUNK slots; stated once for k_order_scatter
// (ttl_order.hip) and for the order-scatter rider of the gather launch
// (ttl_state.hip).  k_tail<true> has counted the bricks and left per slot
// rec[j] = {bin << TTL_INSTEP_OFF_BITS | offset inside the bin, or -1; next row
// or -1} (so: orders of at most 2^18 slots, which is the default ceiling of the
// one-launch tail, and bins < 2^14).  Workgroup `wg` of `n_wg` scans the bin
// counts itself through LDS (nobody waits for anybody) and drops its slots'
// rows at cursor[bin] + offset: the dense order of the survivors in
// out[0 .. n_slots), -1 behind them.  The workgroups also share the clearing of
// the OTHER count buffer, which the next re-bucket counts into.
// s_bin = (bins + TTL_BLOCK / 64) words of LDS: counts -> cursors, wave totals.
// ---------------------------------------------------------------------------
constexpr int TTL_INSTEP_OFF_BITS = 18;
constexpr int TTL_INSTEP_ITEMS = 4;     // slots per thread: a quarter of the workgroups scan
constexpr int TTL_INSTEP_CHUNK = TTL_BLOCK * TTL_INSTEP_ITEMS;
inline size_t ttl_detail_order_scatter_lds(int bins) {
    return ((size_t)bins + TTL_BLOCK / 64) * sizeof(unsigned);
}
__device__ __forceinline__ void order_scatter_block(unsigned *s_bin, int wg, int n_wg,
                                                    const int2 *__restrict__ rec, int n_slots,
                                                    const unsigned *__restrict__ gcount,
                                                    unsigned *__restrict__ gcount_other,
                                                    int bins, int *__restrict__ out) {
    constexpr int BLOCK = TTL_BLOCK, ITEMS = TTL_INSTEP_ITEMS;
    unsigned *s_wave = s_bin + bins;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the slots' records first: their latency hides behind the scan
    const int base = wg * TTL_INSTEP_CHUNK + tid;
    int2 r[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = base + k * BLOCK;
        r[k] = j < n_slots ? rec[j] : int2{-1, -1};
    }
    for (int b = tid; b < bins; b += BLOCK) s_bin[b] = gcount[b];
    for (int b = wg * BLOCK + tid; b < bins; b += n_wg * BLOCK) gcount_other[b] = 0;
    __syncthreads();
    // exclusive scan: ceil(bins / BLOCK) consecutive bins per thread
    const int per = (bins + BLOCK - 1) / BLOCK;
    const int lo = tid * per;
    unsigned sum = 0;
    for (int k = 0; k < per; ++k)
        if (lo + k < bins) sum += s_bin[lo + k];
    unsigned incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned run = incl - sum, total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        if (w < wave) run += s_wave[w];
        total += s_wave[w];
    }
    for (int k = 0; k < per; ++k)
        if (lo + k < bins) {
            const unsigned c = s_bin[lo + k];
            s_bin[lo + k] = run;
            run += c;
        }
    __syncthreads();
    // positions [0, total) are written by the survivors (every bin's offsets
    // are 0 .. count - 1, each taken once), [total, n_slots) by the threads of
    // those slots: every position exactly once
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int j = base + k * BLOCK;
        if (j >= n_slots) continue;
        if ((unsigned)j >= total) out[j] = -1;
        if (r[k].x != -1) {      // (bin << 18 | offset never is all ones: bins < 16 380)
            const unsigned p = s_bin[(unsigned)r[k].x >> TTL_INSTEP_OFF_BITS] +
                               ((unsigned)r[k].x & ((1u << TTL_INSTEP_OFF_BITS) - 1u));
            if (p < (unsigned)n_slots) out[p] = r[k].y;   // (always, unless the counts were not this step's)
        }
    }
}

// ---------------------------------------------------------------------------
// Riders of the gather launch (TTL_TAIL_RIDERS).  Two parts of a k_tail step
// are needed by nothing before the next step: the order scatter of a re-bucket
// step and the row maps (step_map_row).  Both are short and latency-bound, so
// they run as extra workgroups BEHIND the gather's own (blockIdx.x >=
// n_vblocks), which are dispatched while the gather's grid drains: no launch of
// their own on the step's dependency chain, no second stream, no event, and
// nothing pending when the step's launches are done.
//   [n_vblocks, + n_scatter)  order_scatter_block(), TTL_INSTEP_CHUNK slots each;
//   [.., + n_row_blocks)      step_map_row() of TTL_BLOCK active rows each, from
//                             the scanned block bases k_tail's workgroup 0 left
//                             in row_base and the survivor count in P.counts[0].
// ---------------------------------------------------------------------------
struct TailRiders {
    int n_scatter;             // order-scatter workgroups, 0: none
    int n_row_blocks;          // row-map workgroups, 0: none
    // order scatter (see order_scatter_block)
    const int2 *rec;
    const unsigned *count;
    unsigned *count_other;
    int *order_out;
    int n_slots;
    int bins;
    // row maps
    const int *row_base;       // [n_row_blocks] survivors in front of each block of rows
    const int *idx;
    int *idx_next;
    int n_active;
    int order;
    int n_pts;
};
// the most dynamic LDS the riders may ask of the gather launch: with four
// workgroups per CU it leaves the gather's occupancy alone
constexpr size_t TTL_RIDER_MAX_LDS = 16384;

// ttl_state.hip: gathers the state rows of `n_rows` active rows (a step when
// idx != nullptr, the reset otherwise) on stream s; riders (or null): extra
// workgroups of a k_state_dd launch with one workgroup per block of slots --
// TTL_ERR_INVALID for any other launch
int ttl_detail_launch_state(const EnvParams &P, int state_kernel, const int *idx,
                            const int *row_dest, const int *proc, int n_rows, int L,
                            float *out, int64_t pitch, hipStream_t s,
                            const TailRiders *riders = nullptr);
// ttl_state.hip: whether ttl_detail_launch_state() takes the register-deduplicated
// gather (k_state_dd: reads the per-slot records of a processing order)
bool ttl_detail_state_dedupes(const EnvParams &P, int state_kernel);
// ttl_state.hip: the small-batch step tail (prefix + compaction + gather) in
// one launch; host_word = device-visible pinned {n_continue, n_stopped, seq}
// or null
bool ttl_detail_can_fuse_tail(const EnvParams &P, int n_active);
int ttl_detail_launch_fused_tail(const EnvParams &P, const int *idx, int *idx_next,
                                 int n_active, int order, int n_pts, float *out,
                                 int64_t pitch, int *host_word, int seq, hipStream_t s);
// ttl_state.hip: the same tail for a free-running step: n_active, the length
// and the live continue_idx buffer are read from P.counts + TTL_FR_SNAP, the
// next step's words are written to P.counts + TTL_FR_LIVE; rows in partition
// order; n_cap = rows the launch covers
int ttl_detail_launch_fused_tail_fr(const EnvParams &P, int *idx_a, int *idx_b, int n_cap,
                                    float *out, int64_t pitch, int *host_word,
                                    hipStream_t s);
// ---------------------------------------------------------------------------
// The tissue-map criterion inside the step (ttl_env_set_act; ttl_act.hip).
// ---------------------------------------------------------------------------
// ttl_act_desc as the kernels receive it
struct ActCrit {
    const float *include, *exclude;
    int dim[3];
    int mode;
    double shift, exponent;
    unsigned long long seed;
    long long ids_base;
};
// The criterion of a free-running episode, in workspace memory of the handle:
// written by ttl_env_freerun_begin, read by every free-running step -- device
// memory, not a kernel argument, so that a captured step stays valid when the
// next batch brings another seed or ids_base, or switches the criterion off
// (on == 0: the step's hook changes nothing)
struct ActRecord {
    ActCrit crit;
    int on;
};
// the refusals ttl_act_flags and ttl_env_set_act share (TTL_ERR_INVALID): a null
// descriptor or map, a dim < 1, an unknown mode, a negative ids_base, in CMC mode
// an exponent that is not finite and positive
int ttl_detail_act_check(const ttl_act_desc *desc, const char *who);
ActCrit ttl_detail_act_crit(const ttl_act_desc &desc);
// The hook of a host-stepped step, behind k_advance / k_advance_retrack on their
// grid: judges the newest point (point n_points - 1, in P.head) of the n_active
// rows, ORs the bits into the step's decisions by k_restop's rule and redoes the
// block ranks.  init_len: the handle's in a backward pass, else null
int ttl_detail_launch_act_step(const EnvParams &P, const ActCrit &crit, const int *init_len,
                               int n_active, int n_points, uint8_t *done_out, hipStream_t s);
// The same behind k_advance_fr, on its grid of n_cap rows: the criterion comes
// from *rec, the row count and the length from P.counts + TTL_FR_SNAP; a record
// that is off or a step the snapshot marks as skipped judges nothing
int ttl_detail_launch_act_step_fr(const EnvParams &P, const ActRecord *rec, int n_cap,
                                  uint8_t *done_out, hipStream_t s);
// one-thread launch: *rec = {*crit, on} (crit == null: off)
int ttl_detail_launch_act_record(ActRecord *rec, const ActCrit *crit, hipStream_t s);

// ttl_order.hip: rows 0..n-1 sorted by the 8^3-voxel brick of their newest
// point (P.last2 of streamline idx[row]) -> order_out[n]; ws = scratch of
// ttl_detail_order_workspace_bytes(n_max) bytes
size_t ttl_detail_order_workspace_bytes(size_t n);
int ttl_detail_refresh_order(const EnvParams &P, const int *idx, int n, char *ws,
                             size_t ws_bytes, int *order_out, hipStream_t s);
// ttl_order.hip: the in-step re-bucket (TTL_ORDER_INSTEP).  The brick raster of
// the refresh above -> nb[3]; returns its bin count, 0 when it exceeds what the
// scatter's scan holds in LDS (such handles never re-bucket in the step)
int ttl_detail_order_bins(const EnvParams &P, int nb[3]);
// bytes of ONE of the two bin-count buffers
size_t ttl_detail_order_instep_count_bytes();
// the stand-alone launch of order_scatter_block() (see there); clears count_other
int ttl_detail_order_scatter(const int2 *rec, int n_slots, const unsigned *count,
                             unsigned *count_other, int bins, int *order_out, hipStream_t s);
#endif
