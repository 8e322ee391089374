// ttl_coverage.hip -- the binarised tract-count map of the oracle validator
// (TrackToLearn/experiment/oracle_validator.py:48-53: scilpy
// compute_tract_counts_map over the accepted streamlines, > 0 -> 1); part of
// libttl_hip.so.  One wavefront per streamline, one lane per segment: the
// segment's voxel walk (include/ttl_hip.h, ttl_tract_coverage; walk_segment
// in ttl_internal.h) marks the voxels it enters with plain byte stores of 1.
// Every writer stores the same value, so no atomics are needed.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;

__global__ __launch_bounds__(BLOCK) void k_tract_coverage(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const float *__restrict__ scores, float threshold, WalkDims D,
    unsigned char *__restrict__ visited) {
    const int lane = threadIdx.x & 63;
    const auto mark = [&](int x, int y, int z) { visited[walk_index(D, x, y, z)] = 1; };
    wave_rows(n, [&](int row) {
        if (scores && !(scores[row] > threshold)) return;
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        if (L < 1) return;
        const float *p = points + 3 * o0;
        if (lane == 0) walk_first_point(p, D, mark);
        for (long long j = lane; j < L - 1; j += 64)
            walk_segment(p + 3 * j, p + 3 * (j + 1), D, mark);
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
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    hipLaunchKernelGGL(k_tract_coverage, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, scores,
                       threshold, D, visited);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
