// ttl_bundle_recognize.hip -- bundle recognition (include/ttl_hip.h, ttl_bundle_recognize;
// DESIGN 3.19); part of libttl_hip.so.  For every streamline the nearest of M model lines
// by the minimum-average-direct-flip distance, the direction, and the nearest model of
// another label: n * M * K * 2 float64 distances, the assignment step of RecoBundles /
// QuickBundles.  A workgroup takes ROWS = 4 * ROWS_PER_WAVE consecutive rows; every wave
// resamples its own rows into its LDS by the library's one resampler (resample_row over
// CumReplayed, ttl_internal.h) and then all waves walk the models together by the
// library's one tile walk (mdf_tile_walk, ttl_internal.h).  What this file
// adds: the staging of a float tile of at most TILE_STATIONS stations (the coalesced
// global read stores without a bank conflict in the padded tile) and the fold of a lane's
// distances into the nearest model and the nearest of another label.
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
constexpr int TILE_STATIONS = 32;               // stations of a tile, at most

// per wave: pre [64] doubles, res [ROWS_PER_WAVE][3 nb] floats; behind the waves' parts the
// tile [min(nb, TILE_STATIONS)][3][MDF_TILE_PITCH] floats
__host__ __device__ inline size_t recognize_wave_lds(int nb) {
    return (size_t)64 * 8 + (size_t)ROWS_PER_WAVE * (size_t)nb * 12;
}
__host__ __device__ inline size_t recognize_tile_lds(int nb) {
    return (size_t)(nb < TILE_STATIONS ? nb : TILE_STATIONS) * 3 * MDF_TILE_PITCH * sizeof(float);
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
    float *tile = reinterpret_cast<float *>(shared_lds(per_wave));
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

    mdf_tile_walk<ROWS_PER_WAVE>(
        A, res, K, M, tile, TILE_STATIONS, [](int) {},
        [&](int m0, int in_tile, int k0, int kc) {
            // model ml's stations k0 .. k0 + kc are `line` consecutive floats: consecutive
            // threads read consecutive floats and store MDF_TILE_PITCH words apart
            const int line = 3 * kc;
            for (int e = threadIdx.x; e < in_tile * line; e += BLOCK) {
                const int ml = e / line, j = e - ml * line;
                tile[j * MDF_TILE_PITCH + ml] = models[((size_t)(m0 + ml) * K + k0) * 3 + j];
            }
        },
        [&](int m0, const double(&d)[ROWS_PER_WAVE], const double(&f)[ROWS_PER_WAVE]) {
            const int m = m0 + lane;
            if (m >= M) return;                 // the lanes behind the last model read stale words
            const int lab = label ? label[m] : m;
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                const Mdf w = mdf_of(d[r], f[r], K);
                if (w.delta == w.delta) nearest_add(near[r], w.delta, m, lab, w.flipped ? 1 : 0);
            }
        });
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
    if (int rc = ttl_detail_reserve_stations((const void *)k_bundle_recognize, lds,
                                             "ttl_bundle_recognize", nb_points))
        return rc;
    const Lin A = ttl_detail_lin<Lin>(lin);
    const unsigned grid = (unsigned)(((long long)n + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(k_bundle_recognize, dim3(grid), dim3(BLOCK), lds, (hipStream_t)hip_stream,
                       points, (const long long *)offsets, n, models, label, n_models, nb_points,
                       A, best, flip, mdf, runner_up);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
