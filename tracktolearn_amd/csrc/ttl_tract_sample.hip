// ttl_tract_sample.hip -- the arc-length weighted mean of a scalar volume along
// every streamline (restated in include/ttl_hip.h at ttl_tract_sample_mean);
// part of libttl_hip.so.  One wavefront per streamline of the ragged layout of
// ttl_tract_coverage, lanes over the points, 64 a round: a lane measures the
// segment that leaves its point (ttl_connectome_assign's expression), takes the
// one that arrives from the lane below by a shuffle (lane 0: the last lane's of
// the round before, carried in a register), samples the volume trilinearly at its
// point and adds weight and weight * sample to two lane sums; a butterfly sum
// ends the row.  No atomics, no LDS, plain stores by lane 0.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;

// Lin, wave_sum, lin_row, segment_mm and sample_at: ttl_internal.h
using namespace ttl_shared;

__global__ __launch_bounds__(BLOCK) void k_tract_sample_mean(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const float *__restrict__ volume, WalkDims D, Lin A, double *__restrict__ mean,
    double *__restrict__ weight) {
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        double sum_w = 0.0, sum_ws = 0.0;
        double carry = 0.0;                     // the segment that arrives at lane 0's point
        for (long long base = 0; base < L; base += 64) {        // wave-uniform bound
            const long long j = base + lane;
            double after = 0.0, value = 0.0;    // |v_j|, s_j
            bool sampled = false;
            if (j < L) {
                const float *q = p + 3 * j;
                const double c[3] = {q[0], q[1], q[2]};
                if (j < L - 1) {
                    const double c1[3] = {q[3], q[4], q[5]};
                    after = segment_mm(A, c, c1);
                }
                sampled = sample_at(c, volume, D, value);
            }
            double before = __shfl_up(after, 1);                // |v_{j-1}|
            if (lane == 0) before = carry;
            carry = __shfl(after, 63);
            if (sampled) {
                const double w = (before + after) * 0.5;
                sum_w += w;
                sum_ws += w * value;
            }
        }
        sum_w = wave_sum(sum_w);
        sum_ws = wave_sum(sum_ws);
        if (lane == 0) {
            const bool scored = L >= 2 && sum_w > 0.0;
            mean[row] = scored ? sum_ws / sum_w : quiet_nan();
            weight[row] = scored ? sum_w : 0.0;
        }
    });
}
}  // namespace

extern "C" {

int ttl_tract_sample_mean(const float *points, const int64_t *offsets, int32_t n,
                          const float *volume, const int32_t *dims, const double *lin,
                          double *mean, double *weight, void *hip_stream) {
    if (!points || !offsets || !volume || !dims || !lin || !mean || !weight || n < 0 ||
        dims[0] < 1 || dims[1] < 1 || dims[2] < 1)
        return fail(TTL_ERR_INVALID, "ttl_tract_sample_mean: bad arguments");
    if (n == 0) return TTL_OK;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    const Lin A = ttl_detail_lin<Lin>(lin);
    hipLaunchKernelGGL(k_tract_sample_mean, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, volume, D,
                       A, mean, weight);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
