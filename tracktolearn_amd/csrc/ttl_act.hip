// ttl_act.hip -- anatomically constrained stopping (ACT threshold / CMC) on
// tissue maps for gfx950; part of libttl_hip.so, C ABI and the definition in
// include/ttl_hip.h (ttl_act_flags; ttl_env_set_act for the criterion inside
// the step, whose kernels ttl_hip.hip launches), DESIGN 3.14.
#include "ttl_internal.h"

#include <cmath>

namespace {
constexpr int BLOCK = TTL_BLOCK;

struct ActArgs {
    ActCrit crit;
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

// The criterion, stated once (include/ttl_hip.h at ttl_act_flags) for k_act and
// the step's hook: the stopping bits of streamline g whose newest point, the
// n_points-th, is (px, py, pz); inc / exc receive the sampled include / exclude
// values (0 outside the grid).  A row that is not `judged` is sampled but gets
// no bit.  The loads of both maps are issued before either reduction so that
// one round of memory latency covers them.
__device__ __forceinline__ int act_bits(const ActCrit &C, float px, float py, float pz, int g,
                                        int n_points, bool judged, double &inc, double &exc) {
    const double x = (double)px + C.shift, y = (double)py + C.shift, z = (double)pz + C.shift;
    // (NaN compares false: outside)
    const bool inside = x >= -0.5 && x < (double)C.dim[0] - 0.5 && y >= -0.5 &&
                        y < (double)C.dim[1] - 0.5 && z >= -0.5 && z < (double)C.dim[2] - 0.5;
    inc = 0.0, exc = 0.0;
    if (inside) {
        const Axis X = axis_of(x, C.dim[0]), Y = axis_of(y, C.dim[1]), Z = axis_of(z, C.dim[2]);
        const size_t sy = (size_t)C.dim[2], sx = sy * (size_t)C.dim[1];
        inc = trilinear(C.include, sx, sy, X, Y, Z);
        exc = trilinear(C.exclude, sx, sy, X, Y, Z);
    }
    int flag = 0;
    if (judged && inside) {
        if (C.mode == TTL_ACT_THRESHOLD) {
            if (inc > 0.5) flag = TTL_FLAG_TARGET;
            else if (exc > 0.5) flag = TTL_FLAG_EXCLUDE;
        } else {
            const double s = inc + exc;
            if (s > 0.0) {
                double num = 1.0 - s;
                if (num < 0.0) num = 0.0;
                const double den = num + s, rho = num / den;
                // (exponent 1: the power is rho itself, no call)
                const double pw = C.exponent == 1.0 ? rho : pow(rho, C.exponent);
                const unsigned long long id = (unsigned long long)(C.ids_base + g);
                uint32_t c0 = (uint32_t)id, c1 = (uint32_t)(id >> 32),
                         c2 = (uint32_t)n_points, c3 = TTL_ACT_STREAM;
                philox4x32_10(c0, c1, c2, c3, (uint32_t)C.seed, (uint32_t)(C.seed >> 32));
                const double u1 = (double)(c0 >> 8) * 5.9604644775390625e-08;   // 2^-24, exact
                const double u2 = (double)(c1 >> 8) * 5.9604644775390625e-08;
                if (u1 >= pw) flag = u2 < inc / s ? TTL_FLAG_TARGET : TTL_FLAG_EXCLUDE;
            }
        }
    }
    return flag;
}

// ---------------------------------------------------------------------------
// k_act: one lane per row.  The row's newest point (12 bytes at the end of a
// history row picked by ids[]) and its sixteen map values are scattered loads:
// nothing is shared between lanes, so no LDS and no cross-lane work.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_act(const ActArgs A) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= A.n) return;
    const int g = A.ids ? A.ids[r] : r;
    const float *p = A.history + (size_t)g * (size_t)A.pitch + 3 * (size_t)(A.n_points - 1);
    const bool judged = !A.init_len || A.n_points > A.init_len[g];
    double inc, exc;
    const int flag = act_bits(A.crit, p[0], p[1], p[2], g, A.n_points, judged, inc, exc);
    if (A.values) {
        A.values[2 * (size_t)r] = inc;
        A.values[2 * (size_t)r + 1] = exc;
    }
    A.flags[r] = (uint8_t)flag;
}

// ---------------------------------------------------------------------------
// The criterion inside the step (ttl_env_set_act): one lane per active row, on
// the grid of the k_advance* launch in front of it, whose per-row records it
// reads -- P.head[i] holds the newest point and the streamline id of active row
// i (one coalesced 16-byte load instead of idx[i] and then a scattered history
// row), P.stop[i] the decision so far.  The bits go into flags / dones / stop /
// done_out by k_restop's rule (a row another criterion stopped keeps its bits)
// and the block's survivor ranks are redone, as k_restop redoes them.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void act_step_row(const EnvParams &P, const ActCrit &C,
                                             const int *__restrict__ init_len, int n_active,
                                             int n_points, uint8_t *__restrict__ done_out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool active = i < n_active;
    bool stop = false;
    if (active) {
        const float4 hd = *reinterpret_cast<const float4 *>(P.head + 4 * (size_t)i);
        const int g = __float_as_int(hd.w);
        stop = P.stop[i] != 0;
        const bool judged = !init_len || n_points > init_len[g];
        double inc, exc;
        const int bits = act_bits(C, hd.x, hd.y, hd.z, g, n_points, judged, inc, exc);
        if (bits) {
            P.flags[g] = (stop ? P.flags[g] : 0) | bits;
            P.dones[g] = 1;
            P.stop[i] = 1;
            done_out[i] = 1;
            stop = true;
        }
    }
    block_survivor_ranks(P, i, active, active && !stop);
}

// host-stepped: everything is a kernel argument
__global__ __launch_bounds__(BLOCK) void k_act_step(EnvParams P, const ActCrit C,
                                                    const int *__restrict__ init_len,
                                                    int n_active, int n_points,
                                                    uint8_t *__restrict__ done_out) {
    act_step_row(P, C, init_len, n_active, n_points, done_out);
}

// free-running: the criterion from the handle's record, row count and length
// from the words k_advance_fr snapshot (uniform over the grid: whole workgroups
// leave before the barrier of the ranks, which then stay as k_advance_fr left them)
__global__ __launch_bounds__(BLOCK) void k_act_step_fr(EnvParams P,
                                                       const ActRecord *__restrict__ rec,
                                                       uint8_t *__restrict__ done_out) {
    if (!rec->on) return;
    const int *snap = P.counts + TTL_FR_SNAP;
    if (snap[4]) return;           // a skipped step judges nothing
    const ActCrit C = rec->crit;
    act_step_row(P, C, nullptr, snap[0], snap[1] + 1, done_out);
}

__global__ void k_act_record(ActRecord *rec, const ActCrit C, int on) {
    rec->crit = C;
    rec->on = on;
}
}  // namespace

int ttl_detail_act_check(const ttl_act_desc *desc, const char *who) {
    if (!desc || !desc->include || !desc->exclude)
        return fail(TTL_ERR_INVALID, "%s: null pointer", who);
    for (int c = 0; c < 3; ++c)
        if (desc->dim[c] < 1)
            return fail(TTL_ERR_INVALID, "%s: dim[%d]=%d", who, c, desc->dim[c]);
    if (desc->mode != TTL_ACT_THRESHOLD && desc->mode != TTL_ACT_CMC)
        return fail(TTL_ERR_INVALID, "%s: unknown mode %d", who, desc->mode);
    if (desc->ids_base < 0) return fail(TTL_ERR_INVALID, "%s: negative ids_base", who);
    if (desc->mode == TTL_ACT_CMC && !(std::isfinite(desc->exponent) && desc->exponent > 0.0))
        return fail(TTL_ERR_INVALID, "%s: exponent=%g", who, desc->exponent);
    return TTL_OK;
}

ActCrit ttl_detail_act_crit(const ttl_act_desc &desc) {
    ActCrit C;
    C.include = desc.include, C.exclude = desc.exclude;
    for (int c = 0; c < 3; ++c) C.dim[c] = desc.dim[c];
    C.mode = desc.mode;
    C.shift = desc.coord_shift, C.exponent = desc.exponent;
    C.seed = desc.seed, C.ids_base = desc.ids_base;
    return C;
}

int ttl_detail_launch_act_step(const EnvParams &P, const ActCrit &crit, const int *init_len,
                               int n_active, int n_points, uint8_t *done_out, hipStream_t s) {
    hipLaunchKernelGGL(k_act_step, dim3((unsigned)((n_active + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       s, P, crit, init_len, n_active, n_points, done_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_detail_launch_act_step_fr(const EnvParams &P, const ActRecord *rec, int n_cap,
                                  uint8_t *done_out, hipStream_t s) {
    hipLaunchKernelGGL(k_act_step_fr, dim3((unsigned)((n_cap + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       s, P, rec, done_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_detail_launch_act_record(ActRecord *rec, const ActCrit *crit, hipStream_t s) {
    hipLaunchKernelGGL(k_act_record, dim3(1), dim3(1), 0, s, rec, crit ? *crit : ActCrit{},
                       crit ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

extern "C" {

int ttl_act_flags(const ttl_act_desc *desc, const float *history, int64_t row_pitch,
                  const int32_t *ids, const int32_t *init_len, int32_t n, int32_t n_points,
                  uint8_t *flags_out, double *values_out, void *hip_stream) {
    if (!history || !flags_out) return fail(TTL_ERR_INVALID, "ttl_act_flags: null pointer");
    if (const int rc = ttl_detail_act_check(desc, "ttl_act_flags")) return rc;
    if (n < 0 || n_points < 1)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: n=%d, n_points=%d", n, n_points);
    if (row_pitch < 3 * (int64_t)n_points)
        return fail(TTL_ERR_INVALID, "ttl_act_flags: row_pitch=%lld below 3 * n_points=%d",
                    (long long)row_pitch, n_points);
    if (n == 0) return TTL_OK;
    ActArgs A;
    A.crit = ttl_detail_act_crit(*desc);
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
