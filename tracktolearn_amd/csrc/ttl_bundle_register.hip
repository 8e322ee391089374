// ttl_bundle_register.hip -- the cost of streamline-based linear registration (include/
// ttl_hip.h, ttl_bundle_register_cost); part of libttl_hip.so.  For each of T
// candidate transforms the bundle-minimum distance between A fixed and B moving lines of K
// stations: A * B * K * 2 float64 distances per transform, reduced to the minimum of every
// row and of every column of the MDF table.  The inner loop is ttl_bundle_recognize.hip's:
// a workgroup takes ROWS = 4 * ROWS_PER_WAVE fixed lines of one transform, every wave keeps
// its own lines' stations in its LDS, and all waves walk the moving set together through a
// station-major LDS tile ([k][c][line]) in which a lane owns one moving line.  What is new:
// the tile holds float64 stations, transformed while they are staged (once per workgroup
// instead of once per distance); a lane folds its distances into a running minimum per
// fixed line (row_min, a plain store after a butterfly) and into the minimum over its
// workgroup's fixed lines (col_min: the 4 waves meet in LDS and one 64-bit atomic unsigned
// minimum on the bit pattern leaves per moving line and workgroup -- distances are +0 or
// larger, so their order as doubles is their order as unsigned integers).
#include "ttl_internal.h"

namespace {
using namespace ttl_shared;
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int ROWS_PER_WAVE = 2;
constexpr int ROWS = WAVES * ROWS_PER_WAVE;     // fixed lines of a workgroup
constexpr int TILE_LINES = 64;                  // one moving line per lane
constexpr int TILE_PITCH = TILE_LINES + 1;      // doubles per (k, c) line of the tile
constexpr unsigned long long NONE = ~0ull;      // above the bits of every distance

// stations of a tile: 32 as ttl_bundle_recognize while the workgroup stays within 64 KiB
// (K <= 128), 16 beyond
__host__ __device__ inline int register_tile_stations(int nb) {
    return nb <= 128 ? (nb < 32 ? nb : 32) : 16;
}
// per wave: fixed [ROWS_PER_WAVE][3 nb] floats
__host__ __device__ inline size_t register_wave_lds(int nb) {
    return (size_t)ROWS_PER_WAVE * (size_t)nb * 12;
}
// behind the waves' parts: the tile [stations][3][TILE_PITCH] doubles, the waves' column
// minima [WAVES][64] and the tile's "this line takes no part" words [64]
__host__ __device__ inline size_t register_tile_lds(int nb) {
    return (size_t)register_tile_stations(nb) * 3 * TILE_PITCH * sizeof(double);
}
__host__ __device__ inline size_t register_shared_lds(int nb) {
    return register_tile_lds(nb) + (size_t)WAVES * 64 * 8 + (size_t)TILE_LINES * 4;
}

__device__ __forceinline__ double quiet_nan() {
    return __longlong_as_double(0x7ff8000000000000ll);
}

// d(a, m) = |lin (a - m)|, ttl_bundle_orient's expression
__device__ __forceinline__ double distance_mm(const Lin &A, const float *a, double mx, double my,
                                              double mz) {
    const double e[3] = {(double)a[0] - mx, (double)a[1] - my, (double)a[2] - mz};
    const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
    return sqrt((vx * vx + vy * vy) + vz * vz);
}

__device__ __forceinline__ unsigned long long lower_bits(unsigned long long a,
                                                         unsigned long long b) {
    return b < a ? b : a;
}

__device__ __forceinline__ unsigned long long lowest_of_wave(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v = lower_bits(v, __shfl_xor(v, off));
    return v;
}

// grid: x over blocks of ROWS fixed lines, y over the transforms
__global__ __launch_bounds__(BLOCK) void k_bundle_register(
    const float *__restrict__ fixed, int A_lines, const float *__restrict__ moving, int B_lines,
    int K, int tile_k, const double *__restrict__ xf, Lin A, double *__restrict__ row_min,
    unsigned long long *__restrict__ col_bits) {
    const size_t per_wave = register_wave_lds(K);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char *base = wave_lds(per_wave);
    float *res = reinterpret_cast<float *>(base);
    char *shared = base + (size_t)(WAVES - wave) * ((per_wave + 15) & ~(size_t)15);
    double *tile = reinterpret_cast<double *>(shared);
    unsigned long long *colbuf =
        reinterpret_cast<unsigned long long *>(shared + register_tile_lds(K));
    int *bad = reinterpret_cast<int *>(colbuf + WAVES * 64);
    const int t = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * ROWS + (long long)wave * ROWS_PER_WAVE;

    double x[12];                               // the transform: the same in every lane
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = xf[(size_t)t * 12 + i];

    bool part[ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        part[r] = false;
        if (row0 + r < A_lines) {               // wave-uniform
            const float *p = fixed + (size_t)(row0 + r) * K * 3;
            float *q = res + (size_t)r * 3 * K;
            bool nonfinite = false;
            for (int e = lane; e < 3 * K; e += 64) {
                const float v = p[e];
                nonfinite |= !isfinite(v);
                q[e] = v;
            }
            part[r] = !__ballot(nonfinite);
        }
    }
    // a fixed line that takes no part is computed on whatever its LDS holds and never folded

    unsigned long long rbits[ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) rbits[r] = NONE;

    for (int m0 = 0; m0 < B_lines; m0 += TILE_LINES) {
        const int in_tile = min(TILE_LINES, B_lines - m0);
        // the fold of the tile before this one is behind its barrier
        if (threadIdx.x < TILE_LINES) bad[threadIdx.x] = 0;
        double d[ROWS_PER_WAVE], f[ROWS_PER_WAVE];
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) d[r] = f[r] = 0.0;
        for (int k0 = 0; k0 < K; k0 += tile_k) {
            const int kc = min(tile_k, K - k0);
            __syncthreads();                    // the tile before this one has been read
            // a thread takes a station: 3 consecutive floats in, 3 doubles out, 3 TILE_PITCH
            // doubles between the stations of consecutive threads
            for (int e = threadIdx.x; e < in_tile * kc; e += BLOCK) {
                const int ml = e / kc, s = e - ml * kc;
                const float *src = moving + ((size_t)(m0 + ml) * K + k0 + s) * 3;
                const double p0 = src[0], p1 = src[1], p2 = src[2];
                double *dst = tile + (size_t)3 * s * TILE_PITCH + ml;
                bool nonfinite = false;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double v = ((x[4 * c] * p0 + x[4 * c + 1] * p1) + x[4 * c + 2] * p2) +
                                     x[4 * c + 3];
                    nonfinite |= !isfinite(v);
                    dst[c * TILE_PITCH] = v;
                }
                if (nonfinite) bad[ml] = 1;     // every writer stores the same word
            }
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
                const double *m = tile + 3 * kk * TILE_PITCH + lane;
                const double mx = m[0], my = m[TILE_PITCH], mz = m[2 * TILE_PITCH];
                const int k = k0 + kk;
#pragma unroll
                for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                    const float *row = res + (size_t)r * 3 * K;
                    d[r] = d[r] + distance_mm(A, row + 3 * k, mx, my, mz);
                    f[r] = f[r] + distance_mm(A, row + 3 * (K - 1 - k), mx, my, mz);
                }
            }
        }
        const int j = m0 + lane;
        unsigned long long cbits = NONE;
        if (j < B_lines && !bad[lane]) {        // the lanes behind the last line read stale words
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                const double D = d[r] / (double)K, F = f[r] / (double)K;
                const double delta = F < D ? F : D;     // strict: a tie keeps D
                if (part[r] && delta == delta) {
                    const unsigned long long b = (unsigned long long)__double_as_longlong(delta);
                    rbits[r] = lower_bits(rbits[r], b);
                    cbits = lower_bits(cbits, b);
                }
            }
        }
        colbuf[wave * 64 + lane] = cbits;
        __syncthreads();
        if (wave == 0) {
            unsigned long long c = colbuf[lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) c = lower_bits(c, colbuf[w * 64 + lane]);
            if (j < B_lines && c != NONE) atomicMin(col_bits + (size_t)t * B_lines + j, c);
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        if (row0 + r >= A_lines) continue;
        const unsigned long long b = lowest_of_wave(rbits[r]);
        if (lane == 0)
            row_min[(size_t)t * A_lines + row0 + r] =
                b == NONE ? quiet_nan() : __longlong_as_double((long long)b);
    }
}

// The mean of the entries that are not NaN: lane partial sums (lane l adds entries l, l +
// 64, ... in that order), the butterfly, the division by the count; NaN without one.
struct LaneMean {
    double sum = 0.0;
    int count = 0;
    __device__ __forceinline__ void add(double e) {
        if (e == e) {
            sum = sum + e;
            ++count;
        }
    }
    __device__ __forceinline__ double of_wave() const {
        const double total = wave_sum(sum);
        int n = count;
#pragma unroll
        for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off);
        return n ? total / (double)n : quiet_nan();
    }
};

// One wave per transform: a column nothing lowered becomes the quiet NaN, then the cost.
__global__ __launch_bounds__(64) void k_bundle_register_close(
    const double *__restrict__ row_min, int A_lines, unsigned long long *__restrict__ col_bits,
    int B_lines, double *__restrict__ cost) {
    const int t = blockIdx.x, lane = threadIdx.x;
    LaneMean rows, cols;
    for (int i = lane; i < A_lines; i += 64) rows.add(row_min[(size_t)t * A_lines + i]);
    unsigned long long *col = col_bits + (size_t)t * B_lines;
    for (int j = lane; j < B_lines; j += 64) {
        unsigned long long b = col[j];
        if (b == NONE) col[j] = b = 0x7ff8000000000000ull;
        cols.add(__longlong_as_double((long long)b));
    }
    const double s = rows.of_wave() + cols.of_wave();
    if (lane == 0) cost[t] = 0.25 * (s * s);
}
}  // namespace

extern "C" {

int ttl_bundle_register_cost(const float *fixed, int32_t n_fixed, const float *moving,
                             int32_t n_moving, int32_t nb_points, const double *xf, int32_t n_xf,
                             const double *lin, double *row_min, double *col_min, double *cost,
                             void *hip_stream) {
    if (!fixed || !moving || !xf || !lin || !row_min || !col_min || !cost || n_fixed < 1 ||
        n_fixed > TTL_REGISTER_MAX_LINES || n_moving < 1 || n_moving > TTL_REGISTER_MAX_LINES ||
        n_xf < 1 || n_xf > TTL_REGISTER_MAX_TRANSFORMS || nb_points < 2 ||
        nb_points > TTL_PROFILE_MAX_POINTS)
        return fail(TTL_ERR_INVALID, "ttl_bundle_register_cost: bad arguments");
    const size_t lds = wave_lds_bytes(register_wave_lds(nb_points)) + register_shared_lds(nb_points);
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_bundle_register, lds, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_bundle_register_cost: %d stations exceed the LDS",
                    nb_points);
    Lin A;
    for (int i = 0; i < 9; ++i) A.m[i] = lin[i];
    hipStream_t stream = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(col_min, 0xff, (size_t)n_xf * (size_t)n_moving * sizeof(double), stream));
    const dim3 grid((unsigned)((n_fixed + ROWS - 1) / ROWS), (unsigned)n_xf);
    hipLaunchKernelGGL(k_bundle_register, grid, dim3(BLOCK), lds, stream, fixed, n_fixed, moving,
                       n_moving, nb_points, register_tile_stations(nb_points), xf, A, row_min,
                       (unsigned long long *)col_min);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bundle_register_close, dim3((unsigned)n_xf), dim3(64), 0, stream,
                       (const double *)row_min, n_fixed, (unsigned long long *)col_min, n_moving,
                       cost);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
