// ttl_resample.hip -- arc-length resampling of streamlines for the
// TractOracle-Net scoring path (TrackToLearn/oracles/oracle.py:52,70:
// dipy set_number_of_points(streamlines, 128)); part of libttl_hip.so.
// One wavefront per streamline and ONE statement of the algorithm,
// resample_row() (ttl_internal.h, shared with ttl_bundle_profile.hip): float64 segment lengths -> blocked wave scan of the
// cumulative arc length -> each lane places its target points by binary search
// and interpolates linearly inside the segment, the last point kept exactly.
// It is parameterised by how the cumulative arc length is kept: CumStored
// (every value in LDS: rows the LDS holds) or CumReplayed (the 64 lane prefixes
// in LDS, values recomputed on demand: any length, the same bits).  The three
// kernels are shells around it:
//   k_resample                padded batch -> nb points              (CumStored)
//   k_oracle_segments         history rows, optional 3x3 map -> nb - 1
//                             difference vectors                     (CumStored)
//   k_oracle_segments_packed  ragged input of any length -> the same (CumReplayed)
// The file also holds the library's dynamic-LDS reservation
// (ttl_detail_reserve_lds) and the oracle's sparse bonus.
#include <vector>

#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;

// resample_row() and its cumulative arc lengths: ttl_internal.h
using ttl_shared::CumReplayed;
using ttl_shared::CumStored;
using ttl_shared::resample_row;
using ttl_shared::wave_lds;
using ttl_shared::wave_lds_bytes;

// ... per wave: k_resample cum [max_len] doubles; k_oracle_segments cum [n_pts] doubles,
// pts [3 n_pts] floats, res [3 nb] floats; k_oracle_segments_packed pre [64] doubles,
// res [3 nb] floats
__host__ __device__ inline size_t resample_lds(int max_len) { return (size_t)max_len * 8; }
__host__ __device__ inline size_t segments_lds(int n_pts, int nb) {
    return (size_t)n_pts * 8 + (size_t)n_pts * 12 + (size_t)nb * 12;
}
__host__ __device__ inline size_t packed_lds(int nb) { return (size_t)64 * 8 + (size_t)nb * 12; }

// The network's input of a row: the float32 differences of its nb resampled points `res`
// (LDS), which the next row may overwrite on return
__device__ __forceinline__ void difference_row(const float *res, int nb, float *__restrict__ o,
                                               int lane) {
    for (int e = lane; e < 3 * (nb - 1); e += 64) o[e] = res[e + 3] - res[e];
    wave_sync();
}

__global__ __launch_bounds__(BLOCK) void k_resample(
    const float *__restrict__ points, long long row_pitch, const int *__restrict__ lengths32,
    const long long *__restrict__ lengths64, int n, int max_len, int nb,
    float *__restrict__ out) {
    double *cum = reinterpret_cast<double *>(wave_lds(resample_lds(max_len)));
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        int L = lengths32 ? lengths32[row] : (int)lengths64[row];
        L = min(max(L, 1), max_len);
        resample_row(CumStored{cum}, points + (size_t)row * (size_t)row_pitch, L - 1, nb,
                     out + (size_t)row * (size_t)nb * 3, lane);
    });
}

// History rows -> the network's input in one pass: what the env's oracle path
// does with torch ops (gather the rows' first n_pts points, optional 3x3 map
// into the oracle's voxel space, resample to nb points, difference).  The mapped
// points are rounded to float32 and the resampled points to float32 before
// differencing, as the separate steps do.
struct Lin { float m[9]; };          // row-major: out = p @ m

__global__ __launch_bounds__(BLOCK) void k_oracle_segments(
    const float *__restrict__ hist, long long row_pitch, const int *__restrict__ ids,
    int id_stride, int n, int n_pts, int use_lin, Lin lin, int nb, float *__restrict__ dirs) {
    char *base = wave_lds(segments_lds(n_pts, nb));
    double *cum = reinterpret_cast<double *>(base);
    float *pts = reinterpret_cast<float *>(base + (size_t)n_pts * 8);
    float *res = pts + 3 * (size_t)n_pts;
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const long long g = ids ? ids[(size_t)row * id_stride] : row;
        const float *p = hist + g * row_pitch;
        for (int j = lane; j < n_pts; j += 64) {
            float x = p[3 * j], y = p[3 * j + 1], z = p[3 * j + 2];
            if (use_lin) {
                const float a = x, b = y, c = z;
                x = fmaf(c, lin.m[6], fmaf(b, lin.m[3], a * lin.m[0]));
                y = fmaf(c, lin.m[7], fmaf(b, lin.m[4], a * lin.m[1]));
                z = fmaf(c, lin.m[8], fmaf(b, lin.m[5], a * lin.m[2]));
            }
            pts[3 * j] = x;
            pts[3 * j + 1] = y;
            pts[3 * j + 2] = z;
        }
        wave_sync();
        resample_row(CumStored{cum}, pts, n_pts - 1, nb, res, lane);
        difference_row(res, nb, dirs + (size_t)row * (size_t)(nb - 1) * 3, lane);
    });
}

// Ragged streamlines (points + int64 offsets) -> the network's input, for any length
__global__ __launch_bounds__(BLOCK) void k_oracle_segments_packed(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n, int nb,
    float *__restrict__ dirs) {
    char *base = wave_lds(packed_lds(nb));
    double *pre = reinterpret_cast<double *>(base);
    float *res = reinterpret_cast<float *>(base + 64 * 8);
    const int lane = threadIdx.x & 63;
    wave_rows(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        float *o = dirs + (size_t)row * (size_t)(nb - 1) * 3;
        if (L < 1) {                            // nothing to resample: zero vectors
            for (int e = lane; e < 3 * (nb - 1); e += 64) o[e] = 0.0f;
            return;
        }
        resample_row(CumReplayed{pre}, points + 3 * o0, L - 1, nb, res, lane);
        difference_row(res, nb, o, lane);
    });
}

// OracleReward's sparse bonus (oracle_reward.py:84-93): term = 0 everywhere,
// bonus at the stopped rows whose score is > 0.5 (rows past n_scored were never
// scored: 0); reward += term.
__global__ __launch_bounds__(BLOCK) void k_oracle_bonus(
    const float *__restrict__ scores, int n_scored, const int *__restrict__ stop_list,
    int n_stopped, double bonus, double *__restrict__ term, double *__restrict__ reward) {
    const int q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n_stopped) return;
    const int row = stop_list[2 * (size_t)q];
    const double t = (q < n_scored && scores[q] > 0.5f) ? bonus : 0.0;
    term[row] = t;
    reward[row] += t;
}
}  // namespace

int ttl_detail_reserve_lds(const void *kernel, size_t dynamic, LdsRoom *room) {
    struct Seen {
        const void *kernel;
        int dev;
        size_t limit, fixed, allowed;
    };
    static thread_local std::vector<Seen> seen;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    Seen *k = nullptr;
    for (Seen &s : seen)
        if (s.kernel == kernel && s.dev == dev) k = &s;
    if (!k) {
        int limit = 0;
        HIP_TRY(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        hipFuncAttributes fa;
        HIP_TRY(hipFuncGetAttributes(&fa, kernel));
        seen.push_back(Seen{kernel, dev, (size_t)(limit > 0 ? limit : 0), fa.sharedSizeBytes, 0});
        k = &seen.back();
    }
    *room = LdsRoom{k->fixed, k->limit, k->fixed + dynamic <= k->limit};
    if (room->fits && dynamic > k->allowed) {
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dynamic));
        k->allowed = dynamic;
    }
    return TTL_OK;
}

extern "C" {

int ttl_resample_streamlines(const float *points, int64_t row_pitch, const int32_t *lengths32,
                             const int64_t *lengths64, int32_t n, int32_t max_len,
                             int32_t nb_points, float *out, void *hip_stream) {
    if (!points || !out || (!lengths32 && !lengths64) || n < 1 || max_len < 1 ||
        nb_points < 2 || row_pitch < 3LL * max_len)
        return fail(TTL_ERR_INVALID, "ttl_resample_streamlines: bad arguments");
    const size_t lds = wave_lds_bytes(resample_lds(max_len));
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_resample, lds, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_resample_streamlines: %d points per row exceed the LDS",
                    max_len);
    hipLaunchKernelGGL(k_resample, dim3(ttl_detail_wave_grid(n, 4096)), dim3(BLOCK), lds,
                       (hipStream_t)hip_stream, points, (long long)row_pitch, lengths32,
                       (const long long *)lengths64, n, max_len, nb_points, out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_oracle_segments(const float *history, int64_t row_pitch, const int32_t *ids,
                        int32_t id_stride, int32_t n, int32_t n_points, const float *lin,
                        int32_t nb_points, float *dirs_out, void *hip_stream) {
    if (!history || !dirs_out || n < 1 || n_points < 1 || nb_points < 2 ||
        row_pitch < 3LL * n_points || (ids && id_stride < 1))
        return fail(TTL_ERR_INVALID, "ttl_oracle_segments: bad arguments");
    const size_t lds = wave_lds_bytes(segments_lds(n_points, nb_points));
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_oracle_segments, lds, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_oracle_segments: %d points per row exceed the LDS",
                    n_points);
    Lin L{};
    if (lin)
        for (int k = 0; k < 9; ++k) L.m[k] = lin[k];
    hipLaunchKernelGGL(k_oracle_segments, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), lds,
                       (hipStream_t)hip_stream, history, (long long)row_pitch, ids, id_stride, n,
                       n_points, lin ? 1 : 0, L, nb_points, dirs_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_oracle_segments_packed(const float *points, const int64_t *offsets, int32_t n,
                               int32_t nb_points, float *dirs_out, void *hip_stream) {
    if (!points || !offsets || !dirs_out || n < 1 || nb_points < 2)
        return fail(TTL_ERR_INVALID, "ttl_oracle_segments_packed: bad arguments");
    const size_t lds = wave_lds_bytes(packed_lds(nb_points));
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_oracle_segments_packed, lds, &room))
        return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_oracle_segments_packed: %d output points exceed the LDS",
                    nb_points);
    hipLaunchKernelGGL(k_oracle_segments_packed, dim3(ttl_detail_wave_grid(n, 8192)),
                       dim3(BLOCK), lds, (hipStream_t)hip_stream, points,
                       (const long long *)offsets, n, nb_points, dirs_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_oracle_bonus(const float *scores, int32_t n_scored, const int32_t *stop_list,
                     int32_t n_stopped, double bonus, int32_t n_active, double *term,
                     double *reward, void *hip_stream) {
    if (!term || !reward || n_stopped < 0 || n_scored < 0 ||
        (n_stopped > 0 && (!scores || !stop_list)) ||
        n_scored > n_stopped || n_stopped > n_active)
        return fail(TTL_ERR_INVALID, "ttl_oracle_bonus: bad arguments");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(term, 0, (size_t)n_active * sizeof(double), s));
    if (n_stopped > 0) {
        hipLaunchKernelGGL(k_oracle_bonus, dim3((n_stopped + BLOCK - 1) / BLOCK), dim3(BLOCK), 0,
                           s, scores, n_scored, stop_list, n_stopped, bonus, term, reward);
        HIP_TRY(hipGetLastError());
    }
    return TTL_OK;
}

}  // extern "C"
