// ttl_odf_policy.hip -- classical fODF tracking as a policy (deterministic and
// probabilistic direction getters) for gfx950; part of libttl_hip.so, C ABI and
// the definition in include/ttl_hip.h (ttl_odf_actions), DESIGN 3.13.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int VB = 4;     // vertices whose sums run side by side (independent chains)
constexpr int CCH = 16;   // coefficients per staging round of a register kernel

struct OdfArgs {
    const float *state;
    long long pitch;
    int C, dir_offset;
    const float *B;        // [C][V]
    const float *dirs;     // [V][3]
    int V;
    int vch;               // vertices per LDS chunk of B and dirs, a multiple of VB
    float cos_theta, rel;
    int mode;
    unsigned long long seed;
    long long ids_base;
    const int *idx;        // continue_idx (explicit launch) or idx_a (free-running)
    const int *idx_b;      // free-running: the other continue_idx buffer
    const int *live;       // free-running: {n_active, length, cur, .} device words, else null
    int n;                 // rows (free-running: rows the launch covers)
    unsigned step;
    float *actions;
    int *vertex;           // or null
};

// floats of a wave's coefficient tile: CCH (+ 1: odd stride) columns at a time for
// the register kernels, whole rows of 64 rotated by the row number for the generic one
__host__ __device__ constexpr int tile_floats(int CT) { return CT ? 64 * (CCH + 1) : 64 * 64; }
// LDS bytes of a launch: the waves' tiles, then a chunk of B and of dirs
inline size_t odf_lds_bytes(int CT, int C, int vch) {
    return ((size_t)WAVES * tile_floats(CT) + (size_t)vch * (C + 3)) * sizeof(float);
}

// ---------------------------------------------------------------------------
// k_odf<CT>: one lane per row; a workgroup takes groups of 4 x 64 rows, one
// block of 64 per wave.  CT > 0: C == CT (the full even SH orders), the row's
// coefficients sit in CT registers; they come in coalesced, CCH columns at a
// time (lane = element of the block's [64][CCH] tile), through the wave's own LDS
// tile, whose odd row stride makes the read-back with lane = row conflict-free.
// CT == 0: any C up to TTL_ODF_MAX_COEF, the whole block in a tile of rotated
// rows, each term reading its coefficient from there.
// B[c][v] and d_v do not depend on the lane.  A chunk of `vch` vertices of both
// is staged in LDS by the whole workgroup as Bl[v / 4][c][v % 4] and Dl[v][3]
// (zeros behind V): the four B values of a vertex block and a coefficient are one
// 16-byte broadcast read at a constant offset from the block's base.  Where all of
// V fits one chunk it is staged once per launch, otherwise per group, pass and
// chunk.  (Read as wave-uniform global loads instead, B does not stay in the 16 KB
// scalar cache and the loads' latency is exposed: 0.78 ms against 0.2x ms for
// 262 144 rows at C = 45, V = 321)
// No cross-lane arithmetic: every sum is serial, c ascending, then v ascending.
// Passes over the vertices: 0 = gmax and the deterministic running argmax; the
// probabilistic mode adds 1 = the cdf's total and 2 = the pick, recomputing sf
// (the same operations, hence the same bits) instead of keeping V values per
// lane: 64 x V floats per wave would be 82 KB of LDS at V = 321.
// Every __syncthreads() below is reached by all threads: the loops around them
// run on n, V, vch and the mode alone.
// ---------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(BLOCK, 2) void k_odf(const OdfArgs A, const float *__restrict__ state,
                                               const float *__restrict__ Bm,
                                               const float *__restrict__ dirs,
                                               float *__restrict__ actions,
                                               int *__restrict__ vertex) {
    constexpr bool GEN = CT == 0;
    extern __shared__ __align__(16) float odf_lds[];
    int n = A.n;
    unsigned step = A.step;
    const int *idx = A.idx;
    if (A.live) {
        n = min(A.live[0], n);
        step = (unsigned)(A.live[1] - 1);
        idx = A.live[2] ? A.idx_b : A.idx;
    }
    const int C = GEN ? A.C : CT;
    const int V = A.V, vch = A.vch;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *mine = odf_lds + wave * tile_floats(CT);
    float *Bl = odf_lds + WAVES * tile_floats(CT);     // [vch / 4][C][4]
    float *Dl = Bl + (size_t)vch * C;                  // [vch][3]
    const bool one_chunk = vch >= V;
    // chunk [vc, vc + vch) of B and dirs -> LDS, zeros behind V
    auto stage_chunk = [&](int vc) {
        // a thread takes a vertex and walks down its column: the loads of a round are
        // coalesced across the threads and independent along c
        for (int j = threadIdx.x; j < vch; j += BLOCK) {
            const bool in = vc + j < V;
            const float *src = Bm + (in ? vc + j : 0);
            float *dst = Bl + (size_t)(j >> 2) * C * 4 + (j & 3);
#pragma unroll 8
            for (int c = 0; c < C; ++c) dst[4 * c] = in ? src[(size_t)c * V] : 0.0f;
        }
        for (int e = threadIdx.x; e < 3 * vch; e += BLOCK)
            Dl[e] = (3 * vc + e < 3 * V) ? dirs[3 * vc + e] : 0.0f;
    };
    if (one_chunk) {
        stage_chunk(0);
        __syncthreads();
    }
    const int n_groups = (n + BLOCK - 1) / BLOCK;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int r0 = (grp * WAVES + wave) << 6;      // may lie behind n: a wave of dead rows
        float sh[GEN ? 1 : CT];
        if constexpr (GEN) {
            for (int e = lane; e < 64 * C; e += 64) {
                const int r = e / C, c = e - r * C;
                mine[r * 64 + ((c + r) & 63)] =
                    (r0 + r < n) ? state[(size_t)(r0 + r) * (size_t)A.pitch + c] : 0.0f;
            }
            wave_sync();
        } else {
#pragma unroll
            for (int c0 = 0; c0 < CT; c0 += CCH) {
                constexpr int W = CCH;
                const int w = CT - c0 < W ? CT - c0 : W;
                for (int e = lane; e < 64 * w; e += 64) {
                    const int r = e / w, c = e - r * w;
                    mine[r * (CCH + 1) + c] =
                        (r0 + r < n) ? state[(size_t)(r0 + r) * (size_t)A.pitch + c0 + c] : 0.0f;
                }
                wave_sync();
#pragma unroll
                for (int c = 0; c < W; ++c)
                    if (c0 + c < CT) sh[c0 + c] = mine[lane * (CCH + 1) + c];
                wave_sync();                           // the next round overwrites the tile
            }
        }
        const int row = r0 + lane;
        const bool live_row = row < n;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        int g = 0;
        if (live_row) {
            const float *prow = state + (size_t)row * (size_t)A.pitch + A.dir_offset;
            px = prow[0], py = prow[1], pz = prow[2];
            g = idx[row];
        }
        const bool has_p = (px != 0.0f) || (py != 0.0f) || (pz != 0.0f);
        const float cone_min = A.cos_theta * sqrtf((px * px + py * py) + pz * pz);
        float gmax = -INFINITY, best_sf = 0.0f, thr = 0.0f, cdf = 0.0f, pick_at = 0.0f;
        int best = -1, pick = -1;
        const int passes = A.mode == TTL_ODF_PROB ? 3 : 1;
        for (int pass = 0; pass < passes; ++pass) {
            for (int vc = 0; vc < V; vc += vch) {
                if (!one_chunk) {
                    __syncthreads();                   // everybody is done with the last chunk
                    stage_chunk(vc);
                    __syncthreads();
                }
                const int width = min(vch, V - vc);
                for (int j0 = 0; j0 < width; j0 += VB) {
                    const float *bb = Bl + (size_t)(j0 >> 2) * C * 4;
                    float acc[VB];
#pragma unroll
                    for (int k = 0; k < VB; ++k) acc[k] = 0.0f;
                    if constexpr (GEN) {
                        for (int c = 0; c < C; ++c) {
                            const float s = mine[lane * 64 + ((c + lane) & 63)];
                            const float4 b = *reinterpret_cast<const float4 *>(bb + 4 * c);
                            acc[0] = acc[0] + s * b.x;
                            acc[1] = acc[1] + s * b.y;
                            acc[2] = acc[2] + s * b.z;
                            acc[3] = acc[3] + s * b.w;
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < CT; ++c) {
                            const float4 b = *reinterpret_cast<const float4 *>(bb + 4 * c);
                            acc[0] = acc[0] + sh[c] * b.x;
                            acc[1] = acc[1] + sh[c] * b.y;
                            acc[2] = acc[2] + sh[c] * b.z;
                            acc[3] = acc[3] + sh[c] * b.w;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < VB; ++k) {
                        const int v = vc + j0 + k;
                        if (v >= V) break;             // the zeros behind V
                        const float sf = acc[k];
                        const float *d = Dl + 3 * (j0 + k);
                        const float dot = (px * d[0] + py * d[1]) + pz * d[2];
                        const bool cand = (!has_p || fabsf(dot) >= cone_min) && sf > 0.0f;
                        if (pass == 0) {
                            if (sf > gmax) gmax = sf;
                            if (cand && (best < 0 || sf > best_sf)) {
                                best = v;
                                best_sf = sf;
                            }
                        } else if (cand && sf >= thr) {
                            cdf = cdf + sf;
                            if (pass == 2 && pick < 0 && cdf > pick_at) pick = v;
                        }
                    }
                }
            }
            if (pass == 0) {
                thr = A.rel * gmax;
                if (best >= 0 && !(best_sf >= thr)) best = -1;
            } else if (pass == 1) {
                uint32_t c0 = 0, c1 = 0, c2 = step, c3 = TTL_ODF_STREAM;
                if (live_row) {
                    const unsigned long long id = (unsigned long long)(A.ids_base + g);
                    c0 = (uint32_t)id;
                    c1 = (uint32_t)(id >> 32);
                }
                philox4x32_10(c0, c1, c2, c3, (uint32_t)A.seed, (uint32_t)(A.seed >> 32));
                const float u = (float)(c0 >> 8) * 5.9604644775390625e-08f;   // 2^-24, exact
                pick_at = u * cdf;
                cdf = 0.0f;
            }
        }
        if (GEN) wave_sync();                          // the next group overwrites the tile
        if (!live_row) continue;
        const int chosen = A.mode == TTL_ODF_PROB ? pick : best;
        float ax, ay, az;
        if (chosen >= 0) {
            ax = dirs[3 * chosen + 0], ay = dirs[3 * chosen + 1], az = dirs[3 * chosen + 2];
            if ((px * ax + py * ay) + pz * az < 0.0f) ax = -ax, ay = -ay, az = -az;
        } else if (has_p) {
            ax = px, ay = py, az = pz;
        } else {
            ax = dirs[0], ay = dirs[1], az = dirs[2];
        }
        float *o = actions + (size_t)row * 3;
        o[0] = ax, o[1] = ay, o[2] = az;
        if (vertex) vertex[row] = chosen;
    }
}

// LDS a launch aims to stay within where V allows: two workgroups of a register
// kernel, one of the generic kernel per CU
constexpr size_t ODF_LDS_AIM = 80 * 1024, ODF_LDS_AIM_GENERIC = 128 * 1024;

template <int CT>
int launch_one(OdfArgs A, hipStream_t s, const char *what) {
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_odf<CT>, 0, &room)) return rc;
    const size_t aim = CT ? ODF_LDS_AIM : ODF_LDS_AIM_GENERIC;
    const size_t have = (room.limit > room.fixed ? room.limit - room.fixed : 0);
    const size_t tiles = odf_lds_bytes(CT, A.C, 0), budget = have < aim ? have : aim;
    const long long fit = budget > tiles
        ? (long long)((budget - tiles) / ((A.C + 3) * sizeof(float))) / VB * VB : 0;
    if (fit < VB)
        return fail(TTL_ERR_UNSUPPORTED, "%s: %zu bytes of LDS per workgroup are too few", what, have);
    const long long all = ((long long)A.V + VB - 1) / VB * VB;
    A.vch = (int)(all < fit ? all : fit);
    const size_t lds = odf_lds_bytes(CT, A.C, A.vch);
    if (int rc = ttl_detail_reserve_lds((const void *)k_odf<CT>, lds, &room)) return rc;
    if (!room.fits) return fail(TTL_ERR_UNSUPPORTED, "%s: LDS", what);
    const long long wgs = ((long long)A.n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(k_odf<CT>,
                       dim3((unsigned)(wgs < TTL_ODF_GRID_CAP ? wgs : TTL_ODF_GRID_CAP)),
                       dim3(BLOCK), lds, s, A, A.state, A.B, A.dirs, A.actions, A.vertex);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

// the full even orders 2, 4, 6, 8 have kernels of exactly their width
int launch(const OdfArgs &A, hipStream_t s, const char *what) {
    switch (A.C) {
        case 6: return launch_one<6>(A, s, what);
        case 15: return launch_one<15>(A, s, what);
        case 28: return launch_one<28>(A, s, what);
        case 45: return launch_one<45>(A, s, what);
        default: return launch_one<0>(A, s, what);
    }
}

// the argument checks both entry points share; `what` names the caller
int check_args(const char *what, const float *state, int64_t state_pitch, int32_t n_coef,
               int32_t dir_offset, const float *sf_matrix, const float *dirs,
               int32_t n_vertices, int32_t mode, int64_t ids_base, const float *actions_out) {
    if (!state || !sf_matrix || !dirs || !actions_out)
        return fail(TTL_ERR_INVALID, "%s: null pointer", what);
    if (n_coef < 1 || n_coef > TTL_ODF_MAX_COEF)
        return fail(TTL_ERR_INVALID, "%s: n_coef=%d outside 1..%d", what, n_coef,
                    TTL_ODF_MAX_COEF);
    if (n_vertices < 1) return fail(TTL_ERR_INVALID, "%s: n_vertices=%d", what, n_vertices);
    if (mode != TTL_ODF_DET && mode != TTL_ODF_PROB)
        return fail(TTL_ERR_INVALID, "%s: unknown mode %d", what, mode);
    if (dir_offset < 0 || state_pitch < n_coef || state_pitch < (int64_t)dir_offset + 3)
        return fail(TTL_ERR_INVALID, "%s: state_pitch=%lld too small for n_coef=%d, dir_offset=%d",
                    what, (long long)state_pitch, n_coef, dir_offset);
    if (ids_base < 0) return fail(TTL_ERR_INVALID, "%s: negative ids_base", what);
    return TTL_OK;
}
}  // namespace

extern "C" {

int ttl_odf_actions(const float *state, int64_t state_pitch, int32_t n_coef,
                    int32_t dir_offset, const float *sf_matrix, const float *dirs,
                    int32_t n_vertices, float cos_theta, float rel_threshold, int32_t mode,
                    uint64_t seed, int64_t ids_base, const int32_t *continue_idx, int32_t n,
                    uint32_t step, float *actions_out, int32_t *vertex_out, void *hip_stream) {
    if (int rc = check_args("ttl_odf_actions", state, state_pitch, n_coef, dir_offset, sf_matrix,
                            dirs, n_vertices, mode, ids_base, actions_out))
        return rc;
    if (!continue_idx) return fail(TTL_ERR_INVALID, "ttl_odf_actions: null pointer");
    if (n < 0) return fail(TTL_ERR_INVALID, "ttl_odf_actions: n=%d", n);
    if (n == 0) return TTL_OK;
    const OdfArgs A{state, (long long)state_pitch, n_coef, dir_offset, sf_matrix, dirs,
                    n_vertices, 0, cos_theta, rel_threshold, mode, seed, ids_base, continue_idx,
                    nullptr, nullptr, n, step, actions_out, vertex_out};
    return launch(A, (hipStream_t)hip_stream, "ttl_odf_actions");
}

int ttl_env_freerun_odf_actions(ttl_env *env, const float *state, int64_t state_pitch,
                                int32_t n_coef, int32_t dir_offset, const float *sf_matrix,
                                const float *dirs, int32_t n_vertices, float cos_theta,
                                float rel_threshold, int32_t mode, uint64_t seed,
                                int64_t ids_base, int32_t n_rows, float *actions_out,
                                int32_t *vertex_out, void *hip_stream) {
    if (!env) return fail(TTL_ERR_INVALID, "ttl_env_freerun_odf_actions: null pointer");
    if (int rc = check_args("ttl_env_freerun_odf_actions", state, state_pitch, n_coef, dir_offset,
                            sf_matrix, dirs, n_vertices, mode, ids_base, actions_out))
        return rc;
    if (n_rows < 1) return fail(TTL_ERR_INVALID, "ttl_env_freerun_odf_actions: n_rows=%d", n_rows);
    FreerunView fr;
    ttl_detail_freerun_view(env, &fr);
    if (!fr.cap || n_rows > fr.cap)
        return fail(TTL_ERR_STATE, "ttl_env_freerun_odf_actions: not free-running for %d rows",
                    n_rows);
    // a launch only: the call may run under stream capture
    const OdfArgs A{state, (long long)state_pitch, n_coef, dir_offset, sf_matrix, dirs,
                    n_vertices, 0, cos_theta, rel_threshold, mode, seed, ids_base, fr.idx_a,
                    fr.idx_b, fr.live, n_rows, 0u, actions_out, vertex_out};
    return launch(A, (hipStream_t)hip_stream, "ttl_env_freerun_odf_actions");
}

}  // extern "C"
