// ttl_connectome.hip -- the structural connectome's device work (restated in
// include/ttl_hip.h at ttl_connectome_assign / ttl_connectome_accumulate);
// part of libttl_hip.so.  assign: one wavefront per streamline of the ragged
// layout of ttl_tract_coverage: the length in mm as a butterfly sum over the
// segments, then the node of each end -- its own voxel's label, or the nearest
// labelled voxel centre inside a ball of radius_mm (lanes over the box of
// voxels within reach, z fastest; a wave-wide minimum of (d2, linear index)).
// accumulate: one thread per row; the rows of a wavefront that share a cell of
// the (N + 1) x (N + 1) matrices are summed in the wave and one lane adds them
// with one integer atomic per matrix, so the sums do not depend on the order.
// accumulate_metric: the same for a per-row value (the mean of a scalar map along
// the streamline, ttl_tract_sample.hip) at a power-of-two scale.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;
typedef unsigned long long u64;

struct Lin {
    double m[9];
};

struct Reach {
    int r[3];
};

// butterfly: a + b == b + a, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// row r of lin applied to d: ((m0 x + m1 y) + m2 z)
__device__ __forceinline__ double lin_row(const Lin &A, int r, const double (&d)[3]) {
    return (A.m[3 * r] * d[0] + A.m[3 * r + 1] * d[1]) + A.m[3 * r + 2] * d[2];
}

__device__ __forceinline__ bool is_node(int label, int N) { return label >= 1 && label <= N; }

// The node of the end p (finite), the same value in every lane: ttl_hip.h.
__device__ int end_node(const double (&p)[3], const int *__restrict__ labels, const WalkDims &D,
                        int N, const Lin &A, double r2, const Reach &R, int lane) {
    double e[3];
    bool inside = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e[i] = floor(p[i]);
        inside = inside && e[i] >= 0.0 && e[i] < (double)D.d[i];
    }
    // 1. the end's own voxel
    if (inside) {
        const int own = labels[walk_index(D, (int)e[0], (int)e[1], (int)e[2])];
        if (is_node(own, N)) return own;
    }
    // 2. the box of voxels within reach, cut to the volume while still float64: an end
    // at 1e30 never becomes an integer
    int lo[3], cnt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = fmax(e[i] - (double)R.r[i], 0.0);
        const double b = fmin(e[i] + (double)R.r[i], (double)(D.d[i] - 1));
        if (!(a <= b)) return 0;
        lo[i] = (int)a;
        cnt[i] = (int)b - (int)a + 1;
    }
    const int total = cnt[0] * cnt[1] * cnt[2];     // <= (2 * MAX_REACH + 1)^3
    u64 best_d2 = ~0ull, best_idx = ~0ull;
    int best_label = 0;
    for (int t = lane; t < total; t += 64) {
        const int z = lo[2] + t % cnt[2], y = lo[1] + (t / cnt[2]) % cnt[1],
                  x = lo[0] + t / (cnt[2] * cnt[1]);
        const size_t idx = walk_index(D, x, y, z);
        const int label = labels[idx];
        if (!is_node(label, N)) continue;
        const double d[3] = {p[0] - ((double)x + 0.5), p[1] - ((double)y + 0.5),
                             p[2] - ((double)z + 0.5)};
        const double wx = lin_row(A, 0, d), wy = lin_row(A, 1, d), wz = lin_row(A, 2, d);
        const double d2 = (wx * wx + wy * wy) + wz * wz;
        if (!(d2 <= r2)) continue;
        // a lane meets its voxels in increasing linear index: only a smaller d2 replaces
        const u64 bits = (u64)__double_as_longlong(d2);
        if (bits < best_d2) {
            best_d2 = bits;
            best_idx = (u64)idx;
            best_label = label;
        }
    }
    // wave-wide minimum of (d2, index): non-negative doubles order as their bit patterns
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const u64 o_d2 = __shfl_xor(best_d2, off), o_idx = __shfl_xor(best_idx, off);
        const int o_label = __shfl_xor(best_label, off);
        if (o_d2 < best_d2 || (o_d2 == best_d2 && o_idx < best_idx)) {
            best_d2 = o_d2;
            best_idx = o_idx;
            best_label = o_label;
        }
    }
    return best_label;
}

__global__ __launch_bounds__(BLOCK) void k_connectome_assign(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const int *__restrict__ labels, WalkDims D, int N, Lin A, double r2, Reach R,
    int *__restrict__ node, double *__restrict__ length) {
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        const auto leave = [&](int n0, int n1, double len) {
            if (lane == 0) {
                node[2 * (size_t)row] = n0;
                node[2 * (size_t)row + 1] = n1;
                length[row] = len;
            }
        };
        if (L < 2) return leave(-1, -1, 0.0);
        // the length: lanes over the segments
        double len = 0.0;
        bool bad = false;
        for (long long j = lane; j < L; j += 64) {
            const float *q = p + 3 * j;
            const double c[3] = {q[0], q[1], q[2]};
            bad |= !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2]);
            if (j < L - 1) {
                const double e[3] = {(double)q[3] - c[0], (double)q[4] - c[1],
                                     (double)q[5] - c[2]};
                const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
                len += sqrt((vx * vx + vy * vy) + vz * vz);
            }
        }
        if (__ballot(bad)) return leave(-1, -1, 0.0);
        len = wave_sum(len);
        if (!(len < 1099511627776.0)) return leave(-1, -1, 0.0);      // 2^40 mm
        const float *q = p + 3 * (L - 1);
        const double c0[3] = {p[0], p[1], p[2]}, c1[3] = {q[0], q[1], q[2]};
        const int n0 = end_node(c0, labels, D, N, A, r2, R, lane);
        const int n1 = end_node(c1, labels, D, N, A, r2, R, lane);
        leave(n0, n1, len);
    });
}

constexpr int ACCUMULATE_GRID = 2048;       // workgroups: 8 per CU of 256

// One thread per row, whole wavefronts per pass (the loop bound is wave-uniform).  The
// lanes of a wave that share a cell elect their lowest lane, which adds their sum.
__global__ __launch_bounds__(BLOCK) void k_connectome_accumulate(
    const int *__restrict__ node, const double *__restrict__ length, int n, int N,
    u64 *__restrict__ count, u64 *__restrict__ length_q) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * BLOCK;
    const long long first = (long long)blockIdx.x * BLOCK + (threadIdx.x & ~63);
    for (long long base = first; base < n; base += stride) {
        const long long row = base + lane;
        int cell = -1;
        long long q = 0;
        if (row < n) {
            const int n0 = node[2 * row], n1 = node[2 * row + 1];
            // a node above N is not the assign kernel's: skipped, never out of bounds
            if (n0 >= 0 && n1 >= 0 && n0 <= N && n1 <= N) {
                const int a = n0 < n1 ? n0 : n1, b = n0 < n1 ? n1 : n0;
                cell = a * (N + 1) + b;
                if (length) q = llrint(length[row] * TTL_CONNECTOME_LENGTH_SCALE);
            }
        }
        u64 todo = __ballot(cell >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int c = __shfl(cell, leader);
            const bool mine = cell == c;
            const u64 group = __ballot(mine);
            const long long sum = length ? wave_sum(mine ? q : 0ll) : 0ll;
            if (lane == leader) {
                atomicAdd(&count[c], (u64)__popcll(group));
                if (length) atomicAdd(&length_q[c], (u64)sum);
            }
            todo &= ~group;
        }
    }
}

// accumulate for a per-row value: the election of k_connectome_accumulate, written beside it
// so that the kernel above stays as it was compiled.  q = llrint(mean * scale) of the rows
// that count; the rest (not scored, a non-finite mean, |mean * scale| >= 2^40) hold no cell.
__global__ __launch_bounds__(BLOCK) void k_connectome_accumulate_metric(
    const int *__restrict__ node, const double *__restrict__ mean, int n, int N, double scale,
    u64 *__restrict__ metric_q, u64 *__restrict__ metric_n) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * BLOCK;
    const long long first = (long long)blockIdx.x * BLOCK + (threadIdx.x & ~63);
    for (long long base = first; base < n; base += stride) {
        const long long row = base + lane;
        int cell = -1;
        long long q = 0;
        if (row < n) {
            const int n0 = node[2 * row], n1 = node[2 * row + 1];
            const double scaled = mean[row] * scale;
            // a NaN fails the comparison; an infinite mean gives an infinite product
            if (n0 >= 0 && n1 >= 0 && n0 <= N && n1 <= N && fabs(scaled) < 1099511627776.0) {
                const int a = n0 < n1 ? n0 : n1, b = n0 < n1 ? n1 : n0;
                cell = a * (N + 1) + b;
                q = llrint(scaled);
            }
        }
        u64 todo = __ballot(cell >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int c = __shfl(cell, leader);
            const bool mine = cell == c;
            const u64 group = __ballot(mine);
            const long long sum = wave_sum(mine ? q : 0ll);
            if (lane == leader) {
                atomicAdd(&metric_n[c], (u64)__popcll(group));
                atomicAdd(&metric_q[c], (u64)sum);
            }
            todo &= ~group;
        }
    }
}

bool bad_dims(const int32_t *dims) {
    return !dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1;
}
bool bad_nodes(int32_t n_nodes) { return n_nodes < 1 || n_nodes > TTL_CONNECTOME_MAX_NODES; }
}  // namespace

extern "C" {

int ttl_connectome_assign(const float *points, const int64_t *offsets, int32_t n,
                          const int32_t *labels, const int32_t *dims, int32_t n_nodes,
                          const double *lin, double radius_mm, const int32_t *reach,
                          int32_t *node, double *length, void *hip_stream) {
    if (!points || !offsets || !labels || !lin || !reach || !node || !length || n < 0 ||
        bad_nodes(n_nodes) || bad_dims(dims) || !(radius_mm >= 0.0) || !std::isfinite(radius_mm))
        return fail(TTL_ERR_INVALID, "ttl_connectome_assign: bad arguments");
    Reach R;
    for (int i = 0; i < 3; ++i) {
        if (reach[i] < 0 || reach[i] > TTL_CONNECTOME_MAX_REACH)
            return fail(TTL_ERR_INVALID, "ttl_connectome_assign: reach outside 0 .. %d",
                        TTL_CONNECTOME_MAX_REACH);
        R.r[i] = reach[i];
    }
    if (n == 0) return TTL_OK;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    const Lin A = ttl_detail_lin<Lin>(lin);
    hipLaunchKernelGGL(k_connectome_assign, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, labels, D,
                       n_nodes, A, radius_mm * radius_mm, R, node, length);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_connectome_accumulate(const int32_t *node, const double *length, int32_t n,
                              int32_t n_nodes, int64_t *count, int64_t *length_q,
                              void *hip_stream) {
    if (!node || !count || !length_q || n < 0 || bad_nodes(n_nodes))
        return fail(TTL_ERR_INVALID, "ttl_connectome_accumulate: bad arguments");
    if (n == 0) return TTL_OK;
    const long long want = ((long long)n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_connectome_accumulate,
                       dim3((unsigned)(want < ACCUMULATE_GRID ? want : ACCUMULATE_GRID)),
                       dim3(BLOCK), 0, (hipStream_t)hip_stream, node, length, n, n_nodes,
                       (u64 *)count, (u64 *)length_q);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_connectome_accumulate_metric(const int32_t *node, const double *mean, int32_t n,
                                     int32_t n_nodes, double scale, int64_t *metric_q,
                                     int64_t *metric_n, void *hip_stream) {
    if (!node || !mean || !metric_q || !metric_n || n < 0 || bad_nodes(n_nodes))
        return fail(TTL_ERR_INVALID, "ttl_connectome_accumulate_metric: bad arguments");
    if (ttl_detail_bad_scale(scale))
        return fail(TTL_ERR_INVALID,
                    "ttl_connectome_accumulate_metric: scale must be a power of two in "
                    "2^-60 .. 2^60");
    if (n == 0) return TTL_OK;
    const long long want = ((long long)n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_connectome_accumulate_metric,
                       dim3((unsigned)(want < ACCUMULATE_GRID ? want : ACCUMULATE_GRID)),
                       dim3(BLOCK), 0, (hipStream_t)hip_stream, node, mean, n, n_nodes, scale,
                       (u64 *)metric_q, (u64 *)metric_n);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
