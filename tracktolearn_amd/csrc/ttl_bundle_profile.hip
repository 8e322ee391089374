// ttl_bundle_profile.hip -- bundle profiles (include/ttl_hip.h, ttl_bundle_orient and
// ttl_bundle_profile); part of libttl_hip.so.  Two passes over the ragged rows
// of a segmented tractogram: orient every streamline of a bundle against the bundle's
// model and sum the oriented stations (the centroid), then sample a scalar volume at the
// oriented stations and sum value and square per station (the profile).  One wavefront per
// streamline: the row is resampled into the wave's LDS by the library's one resampler
// (resample_row over CumReplayed, ttl_internal.h: 64 prefixes, so LDS does not grow with
// the row), lane k owns station k, k + 64, ...  Every sum is an integer, so it does not
// depend on the order in which rows arrive.  That is what the register runs rest on: a wave
// takes a contiguous range of rows and keeps its lanes' sums in registers while the bundle
// stays the same; the device-scope atomics are issued when the bundle changes and after
// the wave's last row.  TTL_BUNDLE_PROFILE_NO_RUNS (a build-time switch for the
// benchmark's variant, never set in the library) flushes after every row instead.
#include "ttl_internal.h"

namespace {
using namespace ttl_shared;
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int SLOTS = TTL_PROFILE_MAX_POINTS / 64;   // stations per lane, at most
constexpr int GRID_CAP = 1024;                       // workgroups: 16 waves per CU on 256 CUs
constexpr double GATE = 1099511627776.0;             // 2^40
typedef unsigned long long u64;

// per wave: pre [64] doubles, res [3 nb] floats
__host__ __device__ inline size_t profile_lds(int nb) { return (size_t)64 * 8 + (size_t)nb * 12; }

// body(row) for this wave's rows: the n rows are cut into contiguous ranges, one per wave
// of the grid, so that rows sorted by bundle give a wave long runs of one bundle
template <class F>
__device__ __forceinline__ void wave_row_range(int n, F body) {
    const long long waves = (long long)WAVES * gridDim.x;
    const long long per = ((long long)n + waves - 1) / waves;
    const long long wave = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const long long lo = wave * per, hi = lo + per < n ? lo + per : n;
    for (long long row = lo; row < hi; ++row) body((int)row);
}

__global__ __launch_bounds__(BLOCK) void k_bundle_orient(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const int *__restrict__ bundle, int B, int K, const float *__restrict__ model, Lin A,
    double scale, int *__restrict__ flip, double *__restrict__ mdf, u64 *__restrict__ sum_q,
    u64 *__restrict__ sum_n) {
    char *base = wave_lds(profile_lds(K));
    double *pre = reinterpret_cast<double *>(base);
    float *res = reinterpret_cast<float *>(base + 64 * 8);
    const int lane = threadIdx.x & 63;
    u64 acc[SLOTS][3] = {};
    u64 rows = 0;
    int run = -1;                               // the bundle the registers hold, -1: nothing
    auto flush = [&]() {
        if (run < 0) return;
        u64 *q = sum_q + (size_t)run * (size_t)K * 3;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int k = lane + 64 * i;
            if (k < K) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (acc[i][c]) atomicAdd(q + 3 * k + c, acc[i][c]);
                    acc[i][c] = 0;
                }
            }
        }
        if (lane == 0) atomicAdd(sum_n + run, rows);
        rows = 0;
        run = -1;
    };
    wave_row_range(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        const int b = bundle[row];
        bool part = b >= 0 && b < B && L >= 2 && row_is_finite(p, L, lane);
        if (part) {
            resample_row(CumReplayed{pre}, p, L - 1, K, res, lane);
            bool bad = false;
            for (int e = lane; e < 3 * K; e += 64) bad |= !(fabs((double)res[e] * scale) < GATE);
            part = !__ballot(bad);
        }
        if (!part) {                            // wave-uniform
            if (lane == 0) {
                flip[row] = 0;
                mdf[row] = quiet_nan();
            }
            wave_sync();                        // res is rewritten by the next row
            return;
        }
        const float *m = model + (size_t)b * (size_t)K * 3;
        double d = 0.0, f = 0.0;
        for (int k = lane; k < K; k += 64) {
            const double mx = m[3 * k], my = m[3 * k + 1], mz = m[3 * k + 2];
            d += distance_mm(A, res + 3 * k, mx, my, mz);
            f += distance_mm(A, res + 3 * (K - 1 - k), mx, my, mz);
        }
        const Mdf w = mdf_of(wave_sum(d), wave_sum(f), K);
        const bool flipped = w.flipped;
        if (lane == 0) {
            flip[row] = flipped ? 1 : 0;
            mdf[row] = w.delta;
        }
        if (b != run) {
            flush();
            run = b;
        }
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int k = lane + 64 * i;
            if (k < K) {
                const float *o = res + 3 * (flipped ? K - 1 - k : k);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[i][c] += (u64)llrint((double)o[c] * scale);
            }
        }
        rows += 1;
#ifdef TTL_BUNDLE_PROFILE_NO_RUNS
        flush();
#endif
        wave_sync();                            // res is rewritten by the next row
    });
    flush();
}

__global__ __launch_bounds__(BLOCK) void k_bundle_profile(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const int *__restrict__ bundle, const int *__restrict__ flip, int B, int K,
    const float *__restrict__ volume, WalkDims D, double scale, double scale_sq,
    u64 *__restrict__ sum_q, u64 *__restrict__ sum_qq, u64 *__restrict__ count,
    double *__restrict__ values) {
    char *base = wave_lds(profile_lds(K));
    double *pre = reinterpret_cast<double *>(base);
    float *res = reinterpret_cast<float *>(base + 64 * 8);
    const int lane = threadIdx.x & 63;
    u64 acc_q[SLOTS] = {}, acc_qq[SLOTS] = {}, acc_n[SLOTS] = {};
    int run = -1;
    auto flush = [&]() {
        if (run < 0) return;
        const size_t at = (size_t)run * (size_t)K;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int k = lane + 64 * i;
            if (k < K && acc_n[i]) {
                atomicAdd(sum_q + at + k, acc_q[i]);
                atomicAdd(sum_qq + at + k, acc_qq[i]);
                atomicAdd(count + at + k, acc_n[i]);
            }
            acc_q[i] = acc_qq[i] = acc_n[i] = 0;
        }
        run = -1;
    };
    wave_row_range(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        const int b = bundle[row];
        double *out = values ? values + (size_t)row * (size_t)K : nullptr;
        if (!(b >= 0 && b < B && L >= 2 && row_is_finite(p, L, lane))) {    // wave-uniform
            if (out)
                for (int k = lane; k < K; k += 64) out[k] = quiet_nan();
            return;
        }
        resample_row(CumReplayed{pre}, p, L - 1, K, res, lane);
        const bool flipped = flip[row] != 0;
        if (b != run) {
            flush();
            run = b;
        }
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int k = lane + 64 * i;
            if (k < K) {
                const float *o = res + 3 * (flipped ? K - 1 - k : k);
                const double c[3] = {o[0], o[1], o[2]};
                double v = 0.0;
                const bool sampled = sample_at(c, volume, D, v);
                if (out) out[k] = sampled ? v : quiet_nan();
                const double q = v * scale, qq = (v * v) * scale_sq;
                if (sampled && fabs(q) < GATE && fabs(qq) < GATE) {
                    acc_q[i] += (u64)llrint(q);
                    acc_qq[i] += (u64)llrint(qq);
                    acc_n[i] += 1;
                }
            }
        }
#ifdef TTL_BUNDLE_PROFILE_NO_RUNS
        flush();
#endif
        wave_sync();                            // res is rewritten by the next row
    });
    flush();
}

bool bad_shape(int32_t n, int32_t n_bundles, int32_t nb_points) {
    return n < 0 || n_bundles < 1 || n_bundles > TTL_PROFILE_MAX_BUNDLES || nb_points < 2 ||
           nb_points > TTL_PROFILE_MAX_POINTS;
}
}  // namespace

extern "C" {

int ttl_bundle_orient(const float *points, const int64_t *offsets, int32_t n,
                      const int32_t *bundle, int32_t n_bundles, int32_t nb_points,
                      const float *model, const double *lin, double scale, int32_t *flip,
                      double *mdf, int64_t *sum_q, int64_t *sum_n, void *hip_stream) {
    if (!points || !offsets || !bundle || !model || !lin || !flip || !mdf || !sum_q || !sum_n ||
        bad_shape(n, n_bundles, nb_points))
        return fail(TTL_ERR_INVALID, "ttl_bundle_orient: bad arguments");
    if (ttl_detail_bad_scale(scale))
        return fail(TTL_ERR_INVALID,
                    "ttl_bundle_orient: scale must be a power of two in 2^-60 .. 2^60");
    if (n == 0) return TTL_OK;
    const size_t lds = wave_lds_bytes(profile_lds(nb_points));
    if (int rc = ttl_detail_reserve_stations((const void *)k_bundle_orient, lds,
                                             "ttl_bundle_orient", nb_points))
        return rc;
    const Lin A = ttl_detail_lin<Lin>(lin);
    hipLaunchKernelGGL(k_bundle_orient, dim3(ttl_detail_wave_grid(n, GRID_CAP)), dim3(BLOCK), lds,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, bundle,
                       n_bundles, nb_points, model, A, scale, flip, mdf, (u64 *)sum_q,
                       (u64 *)sum_n);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_bundle_profile(const float *points, const int64_t *offsets, int32_t n,
                       const int32_t *bundle, const int32_t *flip, int32_t n_bundles,
                       int32_t nb_points, const float *volume, const int32_t *dims, double scale,
                       double scale_sq, int64_t *sum_q, int64_t *sum_qq, int64_t *count,
                       double *values, void *hip_stream) {
    if (!points || !offsets || !bundle || !flip || !volume || !dims || !sum_q || !sum_qq ||
        !count || bad_shape(n, n_bundles, nb_points) || dims[0] < 1 || dims[1] < 1 || dims[2] < 1)
        return fail(TTL_ERR_INVALID, "ttl_bundle_profile: bad arguments");
    if (ttl_detail_bad_scale(scale) || ttl_detail_bad_scale(scale_sq))
        return fail(TTL_ERR_INVALID,
                    "ttl_bundle_profile: scale and scale_sq must be powers of two in "
                    "2^-60 .. 2^60");
    if (n == 0) return TTL_OK;
    const size_t lds = wave_lds_bytes(profile_lds(nb_points));
    if (int rc = ttl_detail_reserve_stations((const void *)k_bundle_profile, lds,
                                             "ttl_bundle_profile", nb_points))
        return rc;
    const WalkDims D{{dims[0], dims[1], dims[2]}};
    hipLaunchKernelGGL(k_bundle_profile, dim3(ttl_detail_wave_grid(n, GRID_CAP)), dim3(BLOCK), lds,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, bundle,
                       flip, n_bundles, nb_points, volume, D, scale, scale_sq, (u64 *)sum_q,
                       (u64 *)sum_qq, (u64 *)count, values);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
