// ttl_coverage.hip -- the binarised tract-count map of the oracle validator
// (TrackToLearn/experiment/oracle_validator.py:48-53: scilpy
// compute_tract_counts_map over the accepted streamlines, > 0 -> 1); part of
// libttl_hip.so.  One wavefront per streamline, one lane per segment: the
// segment's voxel walk (include/ttl_hip.h, ttl_tract_coverage) marks the
// voxels it enters with plain byte stores of 1.  Every writer stores the same
// value, so no atomics are needed.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;

struct Dims {
    int d[3];
};

__device__ inline void mark(unsigned char *__restrict__ visited, const Dims &D, long long x,
                            long long y, long long z) {
    if (x < 0 || y < 0 || z < 0 || x >= D.d[0] || y >= D.d[1] || z >= D.d[2]) return;
    visited[((size_t)x * (size_t)D.d[1] + (size_t)y) * (size_t)D.d[2] + (size_t)z] = 1;
}

// crossing order: increasing t, the lower axis first on ties
__device__ inline bool before(double t0, int ax0, double t1, int ax1) {
    return t0 < t1 || (t0 == t1 && ax0 < ax1);
}

// floor of a finite coordinate, clamped to [-1, dim]: every test below (inside at the
// start, first / last in-volume plane, leaving the volume) sees the same answer as with
// the unclamped index, and the value fits an int
__device__ inline long long clamped_floor(double v, int dim) {
    return (long long)fmin(fmax(floor(v), -1.0), (double)dim);
}

// The walk of segment a -> b (ttl_hip.h): the voxel entered at every integer-plane
// crossing, crossings in increasing t = (plane - a_i) / d_i (float64, straight from the
// formula), the lower axis first on ties.  Only the crossings during which all three
// indices stay inside the volume are visited: on each axis the planes whose crossing
// leaves that index inside form one run; the in-volume crossings are the part of the
// merged order after the last axis enters (E) and up to the first axis leaving (X).  The
// runs start at E by binary search (t is monotone along a run), so the work is the
// voxels marked plus O(log dim).
__device__ void walk_segment(const float *__restrict__ pa, const float *__restrict__ pb,
                             const Dims &D, unsigned char *__restrict__ visited) {
    double a[3], b[3], d[3];
    long long idx[3], cur[3], left[3];
    int step[3];
    double et = -INFINITY, xt = INFINITY;      // entry E / exit X: (t, axis)
    int eax = -1, xax = 3;
    for (int i = 0; i < 3; ++i) {
        const double ai = pa[i], bi = pb[i];
        if (!isfinite(ai) || !isfinite(bi)) return;
        a[i] = ai;
        b[i] = bi;
        d[i] = bi - ai;
    }
    for (int i = 0; i < 3; ++i) {
        const int dim = D.d[i];
        const long long va = clamped_floor(a[i], dim), vb = clamped_floor(b[i], dim);
        const bool inside = va >= 0 && va < dim;
        idx[i] = va;
        left[i] = 0;
        if (va == vb) {
            if (!inside) return;               // this index never enters the volume
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
            if (left[i] == 0) return;
            const double t = ((double)first - a[i]) / d[i];
            if (before(et, eax, t, i)) {
                et = t;
                eax = i;
            }
        }
        if (exit_plane != -2) {
            const double t = ((double)exit_plane - a[i]) / d[i];
            if (before(t, i, xt, xax)) {
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
                if (before(t, i, et, eax)) lo = mid + 1;
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
            if (left[i] && (m < 0 || before(tn[i], i, tn[m], m))) m = i;
        if (m < 0 || before(xt, xax, tn[m], m)) break;
        idx[m] = step[m] > 0 ? cur[m] : cur[m] - 1;
        mark(visited, D, idx[0], idx[1], idx[2]);
        cur[m] += step[m];
        if (--left[m]) tn[m] = ((double)cur[m] - a[m]) / d[m];
    }
}

__global__ __launch_bounds__(BLOCK) void k_tract_coverage(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const float *__restrict__ scores, float threshold, Dims D,
    unsigned char *__restrict__ visited) {
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        if (scores && !(scores[row] > threshold)) return;
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        if (L < 1) return;
        const float *p = points + 3 * o0;
        if (lane == 0) {
            const double x = p[0], y = p[1], z = p[2];
            if (isfinite(x) && isfinite(y) && isfinite(z))
                mark(visited, D, clamped_floor(x, D.d[0]), clamped_floor(y, D.d[1]),
                     clamped_floor(z, D.d[2]));
        }
        for (long long j = lane; j < L - 1; j += 64)
            walk_segment(p + 3 * j, p + 3 * (j + 1), D, visited);
    });
}
}  // namespace

extern "C" {

int ttl_tract_coverage(const float *points, const int64_t *offsets, int32_t n,
                       const float *scores, float threshold, const int32_t *dims,
                       uint8_t *visited, void *hip_stream) {
    if (!points || !offsets || !visited || !dims || n < 0 || dims[0] < 1 || dims[1] < 1 ||
        dims[2] < 1)
        return fail(TTL_ERR_INVALID, "ttl_tract_coverage: bad arguments");
    if (n == 0) return TTL_OK;
    const Dims D{{dims[0], dims[1], dims[2]}};
    hipLaunchKernelGGL(k_tract_coverage, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, scores,
                       threshold, D, visited);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
