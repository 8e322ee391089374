// ttl_act.hip -- anatomically constrained stopping (ACT threshold / CMC) on
// tissue maps for gfx950; part of libttl_hip.so, C ABI and the definition in
// include/ttl_hip.h (ttl_act_flags), DESIGN 3.14.
#include "ttl_internal.h"

#include <cmath>

namespace {
constexpr int BLOCK = TTL_BLOCK;

struct ActArgs {
    const float *include, *exclude;
    int dim[3];
    int mode;
    double shift, exponent;
    unsigned long long seed;
    long long ids_base;
    const float *history;
    long long pitch;
    const int *ids;        // or null: row r judges history row r
    const int *init_len;   // or null: every row is judged
    int n, n_points;
    uint8_t *flags;
    double *values;        // [n][2] or null
};

// one axis of the trilinear stencil: the two clamped indices and the weight
struct Axis {
    int lo, hi;
    double f;
};
__device__ __forceinline__ Axis axis_of(double x, int dim) {
    const double fl = floor(x);
    const int i = (int)fl;                 // inside: -1 <= i <= dim - 1
    Axis a;
    a.lo = min(max(i, 0), dim - 1);
    a.hi = min(max(i + 1, 0), dim - 1);
    a.f = x - fl;
    return a;
}

// a*(1-f) + b*f, each multiply and the add rounded once (-ffp-contract=off)
__device__ __forceinline__ double lerp(double a, double b, double f) {
    return a * (1.0 - f) + b * f;
}

// the eight corners of one map, reduced along z, then y, then x
__device__ __forceinline__ double trilinear(const float *__restrict__ v, size_t sx, size_t sy,
                                            const Axis &X, const Axis &Y, const Axis &Z) {
    const float *a0 = v + X.lo * sx + Y.lo * sy, *a1 = v + X.lo * sx + Y.hi * sy;
    const float *b0 = v + X.hi * sx + Y.lo * sy, *b1 = v + X.hi * sx + Y.hi * sy;
    // eight independent loads issued before the first use
    const float v000 = a0[Z.lo], v001 = a0[Z.hi], v010 = a1[Z.lo], v011 = a1[Z.hi];
    const float v100 = b0[Z.lo], v101 = b0[Z.hi], v110 = b1[Z.lo], v111 = b1[Z.hi];
    const double c00 = lerp((double)v000, (double)v001, Z.f);
    const double c01 = lerp((double)v010, (double)v011, Z.f);
    const double c10 = lerp((double)v100, (double)v101, Z.f);
    const double c11 = lerp((double)v110, (double)v111, Z.f);
    const double c0 = lerp(c00, c01, Y.f), c1 = lerp(c10, c11, Y.f);
    return lerp(c0, c1, X.f);
}

// ---------------------------------------------------------------------------
// k_act: one lane per row.  The row's newest point (12 bytes at the end of a
// history row picked by ids[]) and its sixteen map values are scattered loads:
// nothing is shared between lanes, so no LDS and no cross-lane work; the
// loads of both maps are issued before either reduction so that one round of
// memory latency covers them.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_act(const ActArgs A) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= A.n) return;
    const int g = A.ids ? A.ids[r] : r;
    const float *p = A.history + (size_t)g * (size_t)A.pitch + 3 * (size_t)(A.n_points - 1);
    const double x = (double)p[0] + A.shift, y = (double)p[1] + A.shift,
                 z = (double)p[2] + A.shift;
    const bool judged = !A.init_len || A.n_points > A.init_len[g];
    // (NaN compares false: outside)
    const bool inside = x >= -0.5 && x < (double)A.dim[0] - 0.5 && y >= -0.5 &&
                        y < (double)A.dim[1] - 0.5 && z >= -0.5 && z < (double)A.dim[2] - 0.5;
    double inc = 0.0, exc = 0.0;
    if (inside) {
        const Axis X = axis_of(x, A.dim[0]), Y = axis_of(y, A.dim[1]), Z = axis_of(z, A.dim[2]);
        const size_t sy = (size_t)A.dim[2], sx = sy * (size_t)A.dim[1];
        inc = trilinear(A.include, sx, sy, X, Y, Z);
        exc = trilinear(A.exclude, sx, sy, X, Y, Z);
    }
    if (A.values) {
        A.values[2 * (size_t)r] = inc;
        A.values[2 * (size_t)r + 1] = exc;
    }
    uint8_t flag = 0;
    if (judged && inside) {
        if (A.mode == TTL_ACT_THRESHOLD) {
            if (inc > 0.5) flag = TTL_FLAG_TARGET;
            else if (exc > 0.5) flag = TTL_FLAG_EXCLUDE;
        } else {
            const double s = inc + exc;
            if (s > 0.0) {
                double num = 1.0 - s;
                if (num < 0.0) num = 0.0;
                const double den = num + s, rho = num / den;
                // (exponent 1: the power is rho itself, no call)
                const double pw = A.exponent == 1.0 ? rho : pow(rho, A.exponent);
                const unsigned long long id = (unsigned long long)(A.ids_base + g);
                uint32_t c0 = (uint32_t)id, c1 = (uint32_t)(id >> 32),
                         c2 = (uint32_t)A.n_points, c3 = TTL_ACT_STREAM;
                philox4x32_10(c0, c1, c2, c3, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
                const double u1 = (double)(c0 >> 8) * 5.9604644775390625e-08;   // 2^-24, exact
                const double u2 = (double)(c1 >> 8) * 5.9604644775390625e-08;
                if (u1 >= pw) flag = u2 < inc / s ? TTL_FLAG_TARGET : TTL_FLAG_EXCLUDE;
            }
        }
    }
    A.flags[r] = flag;
}
}  // namespace

extern "C" {

int ttl_act_flags(const ttl_act_desc *desc, const float *history, int64_t row_pitch,
                  const int32_t *ids, const int32_t *init_len, int32_t n, int32_t n_points,
                  uint8_t *flags_out, double *values_out, void *hip_stream) {
    if (!desc || !history || !flags_out || !desc->include || !desc->exclude)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: null pointer");
    for (int c = 0; c < 3; ++c)
        if (desc->dim[c] < 1)
            return fail(TTL_ERR_INVALID, "ttl_act_flags: dim[%d]=%d", c, desc->dim[c]);
    if (desc->mode != TTL_ACT_THRESHOLD && desc->mode != TTL_ACT_CMC)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: unknown mode %d", desc->mode);
    if (n < 0 || n_points < 1)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: n=%d, n_points=%d", n, n_points);
    if (row_pitch < 3 * (int64_t)n_points)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: row_pitch=%lld below 3 * n_points=%d",
                    (long long)row_pitch, n_points);
    if (desc->ids_base < 0) return fail(TTL_ERR_INVALID, "ttl_act_flags: negative ids_base");
    if (desc->mode == TTL_ACT_CMC && !(std::isfinite(desc->exponent) && desc->exponent > 0.0))
        return fail(TTL_ERR_INVALID, "ttl_act_flags: exponent=%g", desc->exponent);
    if (n == 0) return TTL_OK;
    ActArgs A;
    A.include = desc->include, A.exclude = desc->exclude;
    for (int c = 0; c < 3; ++c) A.dim[c] = desc->dim[c];
    A.mode = desc->mode;
    A.shift = desc->coord_shift, A.exponent = desc->exponent;
    A.seed = desc->seed, A.ids_base = desc->ids_base;
    A.history = history, A.pitch = row_pitch;
    A.ids = ids, A.init_len = init_len;
    A.n = n, A.n_points = n_points;
    A.flags = flags_out, A.values = values_out;
    hipLaunchKernelGGL(k_act, dim3((unsigned)(((long long)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, A);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
