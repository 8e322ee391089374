// ttl_bundle_recognize.hip -- bundle recognition (include/ttl_hip.h, ttl_bundle_recognize;
// DESIGN 3.19); part of libttl_hip.so.  For every streamline the nearest of M model lines
// by the minimum-average-direct-flip distance, the direction, and the nearest model of
// another label: n * M * K * 2 float64 distances, the assignment step of RecoBundles /
// QuickBundles.  A workgroup takes ROWS = 4 * ROWS_PER_WAVE consecutive rows; every wave
// resamples its own rows into its LDS by the library's one resampler (resample_row over
// CumReplayed, ttl_internal.h) and then all waves walk the models together: TILE_MODELS
// models by at most TILE_STATIONS stations are staged in LDS station-major ([k][c][model],
// padded so that the coalesced global read stores without a bank conflict), a lane owns one
// model of the tile, reads the row's station as a broadcast and its own model's station
// from consecutive banks, and every model station read feeds 2 * ROWS_PER_WAVE distances
// (r_k and r_{K-1-k} of each row).  The two K-term sums of a (row, model) pair stay in the
// lane's registers across the station chunks: k = 0, 1, .. K - 1 in that order.
#include "ttl_internal.h"

namespace {
using namespace ttl_shared;
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
#ifndef TTL_RECOGNIZE_ROWS_PER_WAVE
#define TTL_RECOGNIZE_ROWS_PER_WAVE 2           // a build-time switch for the benchmark only
#endif
constexpr int ROWS_PER_WAVE = TTL_RECOGNIZE_ROWS_PER_WAVE;
constexpr int ROWS = WAVES * ROWS_PER_WAVE;     // rows of a workgroup
constexpr int TILE_MODELS = 64;                 // one model per lane
constexpr int TILE_STATIONS = 32;               // stations of a tile, at most
constexpr int TILE_PITCH = TILE_MODELS + 1;     // words per (k, c) line of the tile

// per wave: pre [64] doubles, res [ROWS_PER_WAVE][3 nb] floats; behind the waves' parts the
// tile [min(nb, TILE_STATIONS)][3][TILE_PITCH] floats
__host__ __device__ inline size_t recognize_wave_lds(int nb) {
    return (size_t)64 * 8 + (size_t)ROWS_PER_WAVE * (size_t)nb * 12;
}
__host__ __device__ inline size_t recognize_tile_lds(int nb) {
    return (size_t)(nb < TILE_STATIONS ? nb : TILE_STATIONS) * 3 * TILE_PITCH * sizeof(float);
}

__device__ __forceinline__ double quiet_nan() {
    return __longlong_as_double(0x7ff8000000000000ll);
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

// d(a, m) = |lin (a - m)|, ttl_bundle_orient's expression
__device__ __forceinline__ double distance_mm(const Lin &A, const float *a, double mx, double my,
                                              double mz) {
    const double e[3] = {(double)a[0] - mx, (double)a[1] - my, (double)a[2] - mz};
    const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
    return sqrt((vx * vx + vy * vy) + vz * vz);
}

// The nearest model seen so far and the nearest of another label than its own.  second is
// a distance only: NaN while there is none.
struct Nearest {
    double delta, second;
    int m, label, flip;                         // m < 0: nothing yet
};

__device__ __forceinline__ double lower_of(double a, double b) {   // a NaN is "none"
    if (a != a) return b;
    if (b != b) return a;
    return b < a ? b : a;
}

// (delta, m) of a model behind every model this state has seen (a lane meets its models in
// increasing m, so a tie keeps the earlier one); delta is not a NaN
__device__ __forceinline__ void nearest_add(Nearest &s, double delta, int m, int label, int flip) {
    if (s.m < 0 || delta < s.delta) {
        // the model displaced was the nearest of all: of every label but the new one, too
        if (s.m >= 0 && label != s.label) s.second = s.delta;
        s.delta = delta;
        s.m = m;
        s.label = label;
        s.flip = flip;
    } else if (label != s.label) {
        s.second = lower_of(s.second, delta);
    }
}

// The state of the union of two disjoint model sets: the lexicographic minimum of (delta,
// m); the nearest of another label is, from either side, its first entry when that has
// another label and its second otherwise.  Symmetric in its arguments.
__device__ __forceinline__ Nearest nearest_merge(const Nearest &a, const Nearest &b) {
    const bool b_wins = b.m >= 0 && (a.m < 0 || b.delta < a.delta ||
                                     (b.delta == a.delta && b.m < a.m));
    Nearest w, l;                               // field by field: the states stay in registers
    w.delta = b_wins ? b.delta : a.delta, l.delta = b_wins ? a.delta : b.delta;
    w.second = b_wins ? b.second : a.second, l.second = b_wins ? a.second : b.second;
    w.m = b_wins ? b.m : a.m, l.m = b_wins ? a.m : b.m;
    w.label = b_wins ? b.label : a.label, l.label = b_wins ? a.label : b.label;
    w.flip = b_wins ? b.flip : a.flip;
    w.second = lower_of(w.second, l.m >= 0 && l.label != w.label ? l.delta : l.second);
    return w;
}

__device__ __forceinline__ Nearest nearest_of_wave(Nearest s) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        Nearest o;
        o.delta = __shfl_xor(s.delta, off);
        o.second = __shfl_xor(s.second, off);
        o.m = __shfl_xor(s.m, off);
        o.label = __shfl_xor(s.label, off);
        o.flip = __shfl_xor(s.flip, off);
        s = nearest_merge(s, o);
    }
    return s;
}

__global__ __launch_bounds__(BLOCK) void k_bundle_recognize(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n,
    const float *__restrict__ models, const int *__restrict__ label, int M, int K, Lin A,
    int *__restrict__ best, int *__restrict__ flip, double *__restrict__ mdf,
    double *__restrict__ runner_up) {
    const size_t per_wave = recognize_wave_lds(K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char *base = wave_lds(per_wave);
    double *pre = reinterpret_cast<double *>(base);
    float *res = reinterpret_cast<float *>(base + 64 * 8);
    float *tile = reinterpret_cast<float *>(base + (size_t)(WAVES - wave) *
                                                       ((per_wave + 15) & ~(size_t)15));
    const long long row0 = (long long)blockIdx.x * ROWS + (long long)wave * ROWS_PER_WAVE;

    bool part[ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        part[r] = false;
        if (row0 + r < n) {                     // wave-uniform
            const long long o0 = offsets[row0 + r], L = offsets[row0 + r + 1] - o0;
            const float *p = points + 3 * o0;
            part[r] = L >= 2 && row_is_finite(p, L, lane);
            if (part[r]) resample_row(CumReplayed{pre}, p, L - 1, K, res + (size_t)r * 3 * K, lane);
        }
    }
    // a row that takes no part is computed on whatever its LDS holds and never written

    Nearest near[ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) near[r] = Nearest{0.0, quiet_nan(), -1, 0, 0};

    for (int m0 = 0; m0 < M; m0 += TILE_MODELS) {
        const int in_tile = min(TILE_MODELS, M - m0);
        double d[ROWS_PER_WAVE], f[ROWS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) d[r] = f[r] = 0.0;
        for (int k0 = 0; k0 < K; k0 += TILE_STATIONS) {
            const int kc = min(TILE_STATIONS, K - k0), line = 3 * kc;
            __syncthreads();                    // the tile before this one has been read
            // model ml's stations k0 .. k0 + kc are `line` consecutive floats: consecutive
            // threads read consecutive floats and store TILE_PITCH words apart
            for (int e = threadIdx.x; e < in_tile * line; e += BLOCK) {
                const int ml = e / line, j = e - ml * line;
                tile[j * TILE_PITCH + ml] = models[((size_t)(m0 + ml) * K + k0) * 3 + j];
            }
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
                const float *t = tile + 3 * kk * TILE_PITCH + lane;
                const double mx = t[0], my = t[TILE_PITCH], mz = t[2 * TILE_PITCH];
                const int k = k0 + kk;
#pragma unroll
                for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                    const float *row = res + (size_t)r * 3 * K;
                    d[r] = d[r] + distance_mm(A, row + 3 * k, mx, my, mz);
                    f[r] = f[r] + distance_mm(A, row + 3 * (K - 1 - k), mx, my, mz);
                }
            }
        }
        const int m = m0 + lane;
        if (m < M) {                            // the lanes behind the last model read stale words
            const int lab = label ? label[m] : m;
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                const double D = d[r] / (double)K, F = f[r] / (double)K;
                const bool flipped = F < D;     // strict: a tie or a NaN keeps the row
                const double delta = flipped ? F : D;
                if (delta == delta) nearest_add(near[r], delta, m, lab, flipped ? 1 : 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        if (row0 + r >= n) continue;
        const Nearest s = nearest_of_wave(near[r]);
        if (lane == 0) {
            const bool found = part[r] && s.m >= 0;
            best[row0 + r] = found ? s.m : -1;
            flip[row0 + r] = found ? s.flip : 0;
            mdf[row0 + r] = found ? s.delta : quiet_nan();
            if (runner_up) runner_up[row0 + r] = found ? s.second : quiet_nan();
        }
    }
}
}  // namespace

extern "C" {

int ttl_bundle_recognize(const float *points, const int64_t *offsets, int32_t n,
                         const float *models, const int32_t *label, int32_t n_models,
                         int32_t nb_points, const double *lin, int32_t *best, int32_t *flip,
                         double *mdf, double *runner_up, void *hip_stream) {
    if (!points || !offsets || !models || !lin || !best || !flip || !mdf || n < 0 ||
        n_models < 1 || n_models > TTL_RECOGNIZE_MAX_MODELS || nb_points < 2 ||
        nb_points > TTL_PROFILE_MAX_POINTS)
        return fail(TTL_ERR_INVALID, "ttl_bundle_recognize: bad arguments");
    if (n == 0) return TTL_OK;
    const size_t lds = wave_lds_bytes(recognize_wave_lds(nb_points)) + recognize_tile_lds(nb_points);
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_bundle_recognize, lds, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_bundle_recognize: %d stations exceed the LDS",
                    nb_points);
    Lin A;
    for (int i = 0; i < 9; ++i) A.m[i] = lin[i];
    const unsigned grid = (unsigned)(((long long)n + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(k_bundle_recognize, dim3(grid), dim3(BLOCK), lds, (hipStream_t)hip_stream,
                       points, (const long long *)offsets, n, models, label, n_models, nb_points,
                       A, best, flip, mdf, runner_up);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
