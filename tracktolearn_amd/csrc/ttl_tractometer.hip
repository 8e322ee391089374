// ttl_tractometer.hip -- the Tractometer validator's device work
// (TrackToLearn/experiment/tractometer_validator.py: scilpy
// segment_tractogram_from_roi + compute_tractometry, restated in
// include/ttl_hip.h at ttl_tractometer_classify / ttl_tractometer_overlap);
// part of libttl_hip.so.  The per-bundle volumes are bit planes (bit b of a
// voxel's 64-bit word = bundle b), so one load tests a voxel against every
// bundle.  classify: one wavefront per streamline; the end test sends the bulk
// of a tractogram away after four words, the rest pays for the float64 sums,
// the limits (lane b tests bundle b), the voxel walk (walk_segment,
// ttl_internal.h: the walk of ttl_tract_coverage) and, where a surviving
// bundle sets an angle, the winding.  overlap: the valid streamlines are
// walked again and OR their bundle's bit into a bit volume, which a second
// kernel counts against the ground-truth planes with integer atomics.  invalid
// (ttl_tractometer_invalid): the rows left without a bundle, one thread each,
// test their two ends against the bit planes of the distinct ROIs and name the
// first invalid pair of ROIs they connect.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;
constexpr int LIMITS = TTL_TRACTOMETER_LIMITS;
typedef unsigned long long u64;

struct Planes {
    const u64 *head, *tail, *all, *any;
    u64 has_all, has_any;
};

struct Lin {
    double m[9];
};

__device__ __forceinline__ u64 bundle_mask(int B) { return B < 64 ? (1ull << B) - 1ull : ~0ull; }

// butterfly reductions: a + b == b + a, so after every stage both lanes of a
// pair hold the same bits, and at the end all 64 do
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ u64 wave_and(u64 v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v &= __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ u64 wave_or(u64 v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ u64 wave_uniform(u64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// the voxel floor(c) of an end point: false when the point is non-finite or outside
__device__ inline bool end_voxel(const float *__restrict__ p, const WalkDims &D, size_t *index) {
    int v[3];
    for (int i = 0; i < 3; ++i) {
        const double c = p[i];
        if (!isfinite(c)) return false;
        const double f = floor(c);
        if (f < 0.0 || f >= (double)D.d[i]) return false;
        v[i] = (int)f;
    }
    *index = walk_index(D, v[0], v[1], v[2]);
    return true;
}

// One Jacobi rotation of a symmetric 3x3 matrix in the (p, q) plane: a_pq -> 0.
// r is the third index; vp, vq are columns p and q of the eigenvector matrix.
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &apr,
                                              double &aqr, double (&vp)[3], double (&vq)[3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double pr = apr, qr = aqr;
    apr = c * pr - s * qr;
    aqr = s * pr + c * qr;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vp[k], b = vq[k];
        vp[k] = c * a - s * b;
        vq[k] = s * a + c * b;
    }
}

constexpr int JACOBI_SWEEPS = 8;   // 3x3, float64: converged after 4-5, the rest change nothing

// dipy's winding of the row p[0 .. L) in degrees (ttl_hip.h); mean = its centroid.  The
// same value in every lane.
__device__ double wave_winding(const float *__restrict__ p, long long L, const double (&mean)[3],
                               int lane) {
    double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    for (long long j = lane; j < L; j += 64) {
        const double x = (double)p[3 * j] - mean[0], y = (double)p[3 * j + 1] - mean[1],
                     z = (double)p[3 * j + 2] - mean[2];
        s00 += x * x;
        s01 += x * y;
        s02 += x * z;
        s11 += y * y;
        s12 += y * z;
        s22 += z * z;
    }
    s00 = wave_sum(s00);
    s01 = wave_sum(s01);
    s02 = wave_sum(s02);
    s11 = wave_sum(s11);
    s12 = wave_sum(s12);
    s22 = wave_sum(s22);
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate(s00, s11, s01, s02, s12, v0, v1);
        jacobi_rotate(s00, s22, s02, s01, s12, v0, v2);
        jacobi_rotate(s11, s22, s12, s01, s02, v1, v2);
    }
    // the plane of the two largest eigenvalues: drop the smallest (which of the two
    // vectors comes first does not change a dot product in the plane)
    double u1[3], u2[3];
    const bool drop0 = s00 <= s11 && s00 <= s22, drop1 = !drop0 && s11 <= s22;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u1[k] = drop0 ? v1[k] : v0[k];
        u2[k] = drop0 || drop1 ? v2[k] : v1[k];
    }
    double turn = 0.0;
    for (long long j = lane; j < L - 1; j += 64) {
        double q[2][3];
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) q[e][k] = (double)p[3 * (j + e) + k] - mean[k];
        const double ax = (q[0][0] * u1[0] + q[0][1] * u1[1]) + q[0][2] * u1[2];
        const double ay = (q[0][0] * u2[0] + q[0][1] * u2[1]) + q[0][2] * u2[2];
        const double bx = (q[1][0] * u1[0] + q[1][1] * u1[1]) + q[1][2] * u1[2];
        const double by = (q[1][0] * u2[0] + q[1][1] * u2[1]) + q[1][2] * u2[2];
        double v = (ax * bx + ay * by) / (sqrt(ax * ax + ay * ay) * sqrt(bx * bx + by * by));
        v = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);      // a NaN stays a NaN
        turn += acos(v);
    }
    return wave_sum(turn) * (180.0 / 3.14159265358979323846);
}

__global__ __launch_bounds__(BLOCK) void k_tractometer_classify(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n, WalkDims D,
    int B, Planes P, const double *__restrict__ limits, Lin A, int *__restrict__ bundle,
    u64 *__restrict__ connected) {
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        const auto leave = [&](int b, u64 conn) {
            if (lane == 0) {
                bundle[row] = b;
                connected[row] = conn;
            }
        };
        // 1. the ends: four words decide most rows
        u64 cand = 0;
        if (L >= 2) {
            size_t i0, i1;
            if (end_voxel(p, D, &i0) && end_voxel(p + 3 * (L - 1), D, &i1))
                cand = (P.head[i0] & P.tail[i1]) | (P.tail[i0] & P.head[i1]);
        }
        cand = wave_uniform(cand) & bundle_mask(B);
        if (cand == 0) return leave(-1, 0);

        // 2. float64 sums over the points and segments
        double len = 0.0, sv[3] = {0.0, 0.0, 0.0}, sa[3] = {0.0, 0.0, 0.0},
               sc[3] = {0.0, 0.0, 0.0};
        bool bad = false;
        for (long long j = lane; j < L; j += 64) {
            const float *q = p + 3 * j;
            const double c[3] = {q[0], q[1], q[2]};
            bad |= !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) sc[k] += c[k];
            if (j < L - 1) {
                const double e[3] = {(double)q[3] - c[0], (double)q[4] - c[1],
                                     (double)q[5] - c[2]};
                double v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    v[k] = (A.m[3 * k] * e[0] + A.m[3 * k + 1] * e[1]) + A.m[3 * k + 2] * e[2];
                    sv[k] += v[k];
                    sa[k] += fabs(v[k]);
                }
                len += sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            }
        }
        if (__ballot(bad)) return leave(-1, cand);
        len = wave_sum(len);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sv[k] = fabs(wave_sum(sv[k]));
            sa[k] = wave_sum(sa[k]);
            sc[k] = wave_sum(sc[k]);
        }

        // 3. lane b holds bundle b's limits to the scalars (inclusive bounds)
        bool ok = false;
        double angle = INFINITY;
        if ((cand >> lane) & 1ull) {
            const double *lim = limits + (size_t)LIMITS * lane;
            ok = lim[0] <= len && len <= lim[1];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ok = ok && lim[2 + 2 * k] <= sv[k] && sv[k] <= lim[3 + 2 * k];
                ok = ok && lim[8 + 2 * k] <= sa[k] && sa[k] <= lim[9 + 2 * k];
            }
            angle = lim[14];
        }
        u64 valid = __ballot(ok) & cand;
        if (valid == 0) return leave(-1, cand);

        // 4. all_mask / any_mask over the walk, when a surviving bundle has one
        const u64 need_all = valid & P.has_all, need_any = valid & P.has_any;
        if (need_all | need_any) {
            u64 acc_all = ~0ull, acc_any = 0;
            const auto visit = [&](int x, int y, int z) {
                const size_t i = walk_index(D, x, y, z);
                if (need_all) acc_all &= P.all[i];
                if (need_any) acc_any |= P.any[i];
            };
            if (lane == 0) walk_first_point(p, D, visit);
            for (long long j = lane; j < L - 1; j += 64)
                walk_segment(p + 3 * j, p + 3 * (j + 1), D, visit);
            valid &= (wave_and(acc_all) | ~P.has_all) & (wave_or(acc_any) | ~P.has_any);
            if (valid == 0) return leave(-1, cand);
        }

        // 5. winding < angle (strict; NaN fails), when a surviving bundle sets an angle
        const bool wants = ((valid >> lane) & 1ull) && angle < INFINITY;
        if (__ballot(wants)) {
            const double mean[3] = {sc[0] / (double)L, sc[1] / (double)L, sc[2] / (double)L};
            const double w = wave_winding(p, L, mean, lane);
            valid &= ~__ballot(wants && !(w < angle));
        }
        leave(valid ? __builtin_ctzll(valid) : -1, cand);
    });
}

// the rows with a bundle walk again: bit `bundle` into every voxel of V(s)
__global__ __launch_bounds__(BLOCK) void k_tractometer_mark(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const int *__restrict__ bundle, WalkDims D, int B, u64 *__restrict__ visited) {
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const int b = bundle[row];
        if (b < 0 || b >= B) return;
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        if (L < 1) return;
        const float *p = points + 3 * o0;
        const u64 bit = 1ull << b;
        const auto mark = [&](int x, int y, int z) {
            u64 *word = visited + walk_index(D, x, y, z);
            // bits are only ever set: a word that already shows the bit needs no atomic
            if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
                atomicOr(word, bit);
        };
        if (lane == 0) walk_first_point(p, D, mark);
        for (long long j = lane; j < L - 1; j += 64)
            walk_segment(p + 3 * j, p + 3 * (j + 1), D, mark);
    });
}

// counts[b] = {|M_b & G_b|, |M_b \ G_b|}: LDS counters per workgroup, then one integer
// atomic per non-zero counter
__global__ __launch_bounds__(BLOCK) void k_tractometer_count(
    const u64 *__restrict__ visited, const u64 *__restrict__ gt, size_t n_vox, int B,
    u64 *__restrict__ counts) {
    __shared__ unsigned s_count[128];
    const int tid = threadIdx.x;
    if (tid < 128) s_count[tid] = 0;
    __syncthreads();
    const u64 mask = bundle_mask(B);
    for (size_t v = (size_t)blockIdx.x * BLOCK + tid; v < n_vox; v += (size_t)gridDim.x * BLOCK) {
        u64 m = visited[v] & mask;
        if (m == 0) continue;
        const u64 g = gt[v];
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            atomicAdd(&s_count[2 * b + (int)(((g >> b) & 1ull) ^ 1ull)], 1u);
        }
    }
    __syncthreads();
    if (tid < 2 * B && s_count[tid]) atomicAdd(&counts[tid], (u64)s_count[tid]);
}

// ---- invalid connections (ttl_hip.h, ttl_tractometer_invalid): a set of ROIs is W words,
// bit r % 64 of word r / 64 = ROI r
template <int W>
struct RoiSet {
    u64 w[W];
};

// element `index` of an array of W-word sets, by one load
template <int W>
__device__ __forceinline__ RoiSet<W> load_set(const u64 *__restrict__ base, size_t index);
template <>
__device__ __forceinline__ RoiSet<1> load_set<1>(const u64 *__restrict__ base, size_t index) {
    return RoiSet<1>{{base[index]}};
}
template <>
__device__ __forceinline__ RoiSet<2> load_set<2>(const u64 *__restrict__ base, size_t index) {
    const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(base)[index];
    return RoiSet<2>{{v.x, v.y}};
}

// i * R + j of the first invalid pair (i < j, lexicographic) that the end sets A and B
// connect, or -1.  Such a pair has i in A | B, and its partners are J below.
template <int W>
__device__ __forceinline__ int first_invalid_pair(const RoiSet<W> &A, const RoiSet<W> &B,
                                                  const u64 *__restrict__ valid, int R) {
    u64 any_a = 0, any_b = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        any_a |= A.w[w];
        any_b |= B.w[w];
    }
    if (any_a == 0 || any_b == 0) return -1;       // an end in no ROI connects nothing
#pragma unroll
    for (int w = 0; w < W; ++w) {
        u64 m = A.w[w] | B.w[w];
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1;
            const u64 one = 1ull << bit;
            const bool in_a = (A.w[w] & one) != 0, in_b = (B.w[w] & one) != 0;
            const int i = 64 * w + bit;
            const RoiSet<W> V = load_set<W>(valid, (size_t)i);
#pragma unroll
            for (int v = w; v < W; ++v) {
                u64 J = ((in_a ? B.w[v] : 0ull) | (in_b ? A.w[v] : 0ull)) & ~V.w[v];
                if (v == w) J &= ~((one << 1) - 1ull);      // the bits above i (none above 63)
                if (J) return i * R + 64 * v + __builtin_ctzll(J);
            }
        }
    }
    return -1;
}

// one thread per streamline; top = the bits of the last word that name an ROI (bits at or
// above R in the caller's planes are not read as ROIs, so i and j stay below R)
template <int W>
__global__ __launch_bounds__(BLOCK) void k_tractometer_invalid(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const int *__restrict__ bundle, WalkDims D, int R, u64 top, const u64 *__restrict__ roi,
    const u64 *__restrict__ valid, int *__restrict__ pair) {
    const long long stride = (long long)gridDim.x * BLOCK;
    for (long long row = (long long)blockIdx.x * BLOCK + threadIdx.x; row < n; row += stride) {
        int found = -1;
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        if (bundle[row] < 0 && L >= 2) {
            const float *p = points + 3 * o0;
            size_t i0, i1;
            if (end_voxel(p, D, &i0) && end_voxel(p + 3 * (L - 1), D, &i1)) {
                RoiSet<W> A = load_set<W>(roi, i0), B = load_set<W>(roi, i1);
                A.w[W - 1] &= top;
                B.w[W - 1] &= top;
                found = first_invalid_pair<W>(A, B, valid, R);
            }
        }
        pair[row] = found;
    }
}
constexpr int INVALID_GRID = 2048;      // workgroups: 8 per CU of 256, every wave slot

bool bad_dims(const int32_t *dims) {
    return !dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1;
}
}  // namespace

extern "C" {

int ttl_tractometer_classify(const float *points, const int64_t *offsets, int32_t n,
                             const int32_t *dims, int32_t n_bundles, const uint64_t *head,
                             const uint64_t *tail, const uint64_t *all, const uint64_t *any,
                             uint64_t has_all, uint64_t has_any, const double *limits,
                             const double *lin, int32_t *bundle, uint64_t *connected,
                             void *hip_stream) {
    if (!points || !offsets || !head || !tail || !all || !any || !limits || !lin || !bundle ||
        !connected || n < 0 || n_bundles < 1 || n_bundles > 64 || bad_dims(dims))
        return fail(TTL_ERR_INVALID, "ttl_tractometer_classify: bad arguments");
    if (n == 0) return TTL_OK;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    const Planes P{(const u64 *)head, (const u64 *)tail, (const u64 *)all, (const u64 *)any,
                   has_all, has_any};
    const Lin A = ttl_detail_lin<Lin>(lin);
    hipLaunchKernelGGL(k_tractometer_classify, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK),
                       0, (hipStream_t)hip_stream, points, (const long long *)offsets, n, D,
                       n_bundles, P, limits, A, bundle, (u64 *)connected);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_tractometer_overlap(const float *points, const int64_t *offsets, int32_t n,
                            const int32_t *bundle, const int32_t *dims, int32_t n_bundles,
                            const uint64_t *gt, uint64_t *visited_bits, int64_t *counts,
                            void *hip_stream) {
    if (!points || !offsets || !bundle || !gt || !visited_bits || !counts || n < 0 ||
        n_bundles < 1 || n_bundles > 64 || bad_dims(dims))
        return fail(TTL_ERR_INVALID, "ttl_tractometer_overlap: bad arguments");
    hipStream_t s = (hipStream_t)hip_stream;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    const size_t n_vox = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * (size_t)n_bundles, s));
    if (n > 0)
        hipLaunchKernelGGL(k_tractometer_mark, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK),
                           0, s, points, (const long long *)offsets, n, bundle, D, n_bundles,
                           (u64 *)visited_bits);
    const size_t want = (n_vox + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_tractometer_count, dim3((unsigned)(want < 2048 ? want : 2048)),
                       dim3(BLOCK), 0, s, (const u64 *)visited_bits, (const u64 *)gt, n_vox,
                       n_bundles, (u64 *)counts);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_tractometer_invalid(const float *points, const int64_t *offsets, int32_t n,
                            const int32_t *bundle, const int32_t *dims, int32_t n_rois,
                            const uint64_t *roi, const uint64_t *valid, int32_t *pair,
                            void *hip_stream) {
    if (!points || !offsets || !bundle || !roi || !valid || !pair || n < 0 || n_rois < 2 ||
        n_rois > TTL_TRACTOMETER_MAX_ROIS || bad_dims(dims))
        return fail(TTL_ERR_INVALID, "ttl_tractometer_invalid: bad arguments");
    const int W = (n_rois + 63) / 64;
    if (W == 2 && (((uintptr_t)roi | (uintptr_t)valid) & 15))
        return fail(TTL_ERR_INVALID, "ttl_tractometer_invalid: two-word sets need 16-byte "
                                     "aligned roi and valid");
    if (n == 0) return TTL_OK;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    const u64 top = n_rois % 64 ? (1ull << (n_rois % 64)) - 1ull : ~0ull;
    const long long want = ((long long)n + BLOCK - 1) / BLOCK;
    const dim3 grid((unsigned)(want < INVALID_GRID ? want : INVALID_GRID));
    if (W == 1)
        hipLaunchKernelGGL(k_tractometer_invalid<1>, grid, dim3(BLOCK), 0,
                           (hipStream_t)hip_stream, points, (const long long *)offsets, n,
                           bundle, D, n_rois, top, (const u64 *)roi, (const u64 *)valid, pair);
    else
        hipLaunchKernelGGL(k_tractometer_invalid<2>, grid, dim3(BLOCK), 0,
                           (hipStream_t)hip_stream, points, (const long long *)offsets, n,
                           bundle, D, n_rois, top, (const u64 *)roi, (const u64 *)valid, pair);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
