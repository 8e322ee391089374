// ttl_tract_density.hip -- track density maps (include/ttl_hip.h, ttl_tract_density;
// DESIGN 3.17); part of libttl_hip.so.  Per voxel: how many streamlines pass through it,
// how many mm of streamline lie in it (total and per RAS axis), how many streamlines end in
// it.  One wavefront per streamline, lanes over the segments: the voxel walk of
// ttl_tract_coverage (walk_segment_pieces, ttl_internal.h) cuts a segment into the pieces
// between consecutive crossings, and every piece goes straight to global integer atomics.
// The count needs the SET of a row's voxels: the visited voxels are inserted into an
// open-addressing table in this wave's LDS, and a sweep adds 1 per occupied slot and clears
// it.  A row whose set does not fit goes to a list in the workspace; a second launch of the
// same call takes one workgroup per such row and repeats the walk with a table in global
// memory.  Every probe loop is bounded by its table's size and insertion stops once the
// count of new keys has passed the capacity, so a full table ends a row, never holds a lane.
#include "ttl_internal.h"

namespace {
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
constexpr int DEFAULT_WAVE_SLOTS = 2048;
constexpr int MAX_SPILL_SLOTS = 1 << 26;
constexpr int SPILL_GRID = 256;             // workgroups of the spill launch, at most
constexpr int SPILL_TABLE_WORDS = 1 << 22;  // ... and the words of all their tables, when > 1
constexpr size_t WS_HEADER = 64;            // bytes: {rows listed, workgroups done}
typedef unsigned long long u64;

struct Lin {
    double m[9];
};

struct Maps {
    int *count;
    u64 *length_q, *dec_q;
    int *ends;
};

// ttl_connectome.hip's butterfly: a + b == b + a, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// row r of lin applied to d: ((m0 x + m1 y) + m2 z)
__device__ __forceinline__ double lin_row(const Lin &A, int r, const double (&d)[3]) {
    return (A.m[3 * r] * d[0] + A.m[3 * r + 1] * d[1]) + A.m[3 * r + 2] * d[2];
}

// the voxel of a finite point when it lies inside the volume
__device__ __forceinline__ bool voxel_of(const float *__restrict__ p, const WalkDims &D,
                                         size_t *index) {
    const long long x = walk_clamped_floor((double)p[0], D.d[0]),
                    y = walk_clamped_floor((double)p[1], D.d[1]),
                    z = walk_clamped_floor((double)p[2], D.d[2]);
    if (x < 0 || y < 0 || z < 0 || x >= D.d[0] || y >= D.d[1] || z >= D.d[2]) return false;
    *index = walk_index(D, (int)x, (int)y, (int)z);
    return true;
}

// The set of a row's voxels: open addressing over mask + 1 words (LDS of one wave, or
// global memory of one workgroup), key = voxel index + 1, 0 = free; *fresh counts the new
// keys.  At most mask + 1 probes; nothing is inserted once *fresh has passed cap.  A key that
// finds the table full is counted too: it is a new one, and the table holds more than cap.
__device__ __forceinline__ void set_insert(unsigned *tab, unsigned mask, unsigned key, int *fresh,
                                           int cap) {
    if (__hip_atomic_load(fresh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > cap) return;
    unsigned h = key * 0x9E3779B1u;
    h = (h ^ (h >> 15)) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned old = atomicCAS(tab + h, 0u, key);
        if (old == key) return;
        if (old == 0u) break;
        h = (h + 1u) & mask;
    }
    atomicAdd(fresh, 1);
}

// The length rule of ttl_connectome_assign, the same value in every lane: the row adds
// nothing when a point is non-finite or sum_j |v_j| is not < 2^40 mm.
__device__ __forceinline__ bool row_is_added(const float *__restrict__ p, long long L,
                                             const Lin &A, int lane) {
    double len = 0.0;
    bool bad = false;
    for (long long j = lane; j < L; j += 64) {
        const float *q = p + 3 * j;
        const double c[3] = {q[0], q[1], q[2]};
        bad |= !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2]);
        if (j < L - 1) {
            const double e[3] = {(double)q[3] - c[0], (double)q[4] - c[1], (double)q[5] - c[2]};
            const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
            len += sqrt((vx * vx + vy * vy) + vz * vz);
        }
    }
    if (__ballot(bad)) return false;
    return wave_sum(len) < 1099511627776.0;      // 2^40 mm
}

// list: the rows whose set left the wave's table, for k_density_spill (null: status 2)
__global__ __launch_bounds__(BLOCK) void k_tract_density(
    const float *__restrict__ points, const long long *__restrict__ offsets, int n, WalkDims D,
    Lin A, Maps M, int wave_slots, int *__restrict__ status, unsigned *__restrict__ ws_header,
    int *__restrict__ list) {
    extern __shared__ unsigned s_density[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *tab = s_density + (size_t)wave * wave_slots;
    int *fresh = reinterpret_cast<int *>(s_density + (size_t)WAVES * wave_slots) + wave;
    const unsigned mask = (unsigned)wave_slots - 1u;
    const int cap = wave_slots / 2;
    if (M.count) {
        for (int s = lane; s < wave_slots; s += 64) tab[s] = 0u;
        if (lane == 0) *fresh = 0;
        wave_sync();
    }
    const bool pieces = M.length_q || M.dec_q;
    wave_rows(n, [&](int row) {
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        if (L < 2 || !row_is_added(p, L, A, lane)) {
            if (lane == 0) status[row] = -1;
            return;
        }
        if (lane == 0) {
            size_t v;
            if (voxel_of(p, D, &v)) {
                if (M.ends) atomicAdd(M.ends + v, 1);
                if (M.count) set_insert(tab, mask, (unsigned)v + 1u, fresh, cap);
            }
            if (M.ends && voxel_of(p + 3 * (L - 1), D, &v)) atomicAdd(M.ends + v, 1);
        }
        for (long long j = lane; j < L - 1; j += 64) {
            const float *pa = p + 3 * j, *pb = pa + 3;
            double len = 0.0, av[3] = {0.0, 0.0, 0.0};
            if (pieces) {
                const double e[3] = {(double)pb[0] - (double)pa[0], (double)pb[1] - (double)pa[1],
                                     (double)pb[2] - (double)pa[2]};
                const double vx = lin_row(A, 0, e), vy = lin_row(A, 1, e), vz = lin_row(A, 2, e);
                len = sqrt((vx * vx + vy * vy) + vz * vz);
                av[0] = fabs(vx);
                av[1] = fabs(vy);
                av[2] = fabs(vz);
            }
            // the open piece: its voxel and where it starts; floor(a)'s starts at 0
            size_t vox = 0;
            double t_lo = 0.0;
            bool open = voxel_of(pa, D, &vox);
            const auto close = [&](double t_hi) {
                if (!open || !pieces) return;
                const double w = t_hi - t_lo;
                if (M.length_q)
                    atomicAdd(M.length_q + vox, (u64)llrint((w * len) * TTL_CONNECTOME_LENGTH_SCALE));
                if (M.dec_q) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        atomicAdd(M.dec_q + 3 * vox + k,
                                  (u64)llrint((w * av[k]) * TTL_CONNECTOME_LENGTH_SCALE));
                }
            };
            unsigned last_key = 0u;        // a lane's own latest key needs no second probe
            const double t_end = walk_segment_pieces(pa, pb, D, [&](int x, int y, int z, double t) {
                close(t);
                vox = walk_index(D, x, y, z);
                t_lo = t;
                open = true;
                const unsigned key = (unsigned)vox + 1u;
                if (M.count && key != last_key) {
                    set_insert(tab, mask, key, fresh, cap);
                    last_key = key;
                }
            });
            close(t_end);
        }
        if (!M.count) {
            if (lane == 0) status[row] = 0;
            return;
        }
        // the sweep: one add per voxel of the set when the row fitted, none otherwise; the
        // table is empty for the wave's next row either way
        wave_sync();
        const bool fitted = *fresh <= cap;
        for (int s = lane; s < wave_slots; s += 64) {
            const unsigned key = tab[s];
            if (key == 0u) continue;
            if (fitted) atomicAdd(M.count + (key - 1u), 1);
            tab[s] = 0u;
        }
        if (lane == 0) {
            *fresh = 0;
            if (fitted) {
                status[row] = 0;
            } else if (list) {
                list[atomicAdd(ws_header, 1u)] = row;    // at most once per row: < n entries
            } else {
                status[row] = 2;
            }
        }
        wave_sync();
    });
}

// One workgroup per listed row, the list taken by stride: the walk once more with only the
// set, in this workgroup's table of spill_slots words of the workspace.  Leaves the list,
// its counter and the tables zeroed.
__global__ __launch_bounds__(BLOCK) void k_tract_density_spill(
    const float *__restrict__ points, const long long *__restrict__ offsets, WalkDims D,
    int *__restrict__ count, int spill_slots, int *__restrict__ status,
    unsigned *__restrict__ ws_header, int *__restrict__ list, unsigned *__restrict__ tables) {
    __shared__ int s_fresh;
    unsigned *tab = tables + (size_t)blockIdx.x * spill_slots;
    const unsigned mask = (unsigned)spill_slots - 1u;
    const int cap = spill_slots / 2;
    const int total = (int)__hip_atomic_load(ws_header, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0) s_fresh = 0;
    __syncthreads();
    for (int e = blockIdx.x; e < total; e += gridDim.x) {
        const int row = list[e];
        const long long o0 = offsets[row], L = offsets[row + 1] - o0;
        const float *p = points + 3 * o0;
        if (threadIdx.x == 0) {
            size_t v;
            if (voxel_of(p, D, &v)) set_insert(tab, mask, (unsigned)v + 1u, &s_fresh, cap);
        }
        for (long long j = threadIdx.x; j < L - 1; j += BLOCK) {
            unsigned last_key = 0u;
            walk_segment(p + 3 * j, p + 3 * (j + 1), D, [&](int x, int y, int z) {
                const unsigned key = (unsigned)walk_index(D, x, y, z) + 1u;
                if (key != last_key) {
                    set_insert(tab, mask, key, &s_fresh, cap);
                    last_key = key;
                }
            });
        }
        __syncthreads();
        const bool fitted = s_fresh <= cap;
        // the table was written by atomics at the device's L2: read it there
        for (int s = threadIdx.x; s < spill_slots; s += BLOCK) {
            const unsigned key =
                __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (key == 0u) continue;
            if (fitted) atomicAdd(count + (key - 1u), 1);
            __hip_atomic_store(tab + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            status[row] = fitted ? 1 : 2;
            list[e] = 0;
            s_fresh = 0;
        }
        __syncthreads();
    }
    // the last workgroup to finish zeroes the header: every one has read the count by now
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned done = atomicAdd(ws_header + 1, 1u);
        if (done == gridDim.x - 1u) {
            __hip_atomic_store(ws_header, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ws_header + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

bool power_of_two(long long v) { return v > 0 && (v & (v - 1)) == 0; }

unsigned spill_grid(int spill_slots) {
    const int fit = SPILL_TABLE_WORDS / spill_slots;
    return (unsigned)(fit < 1 ? 1 : fit > SPILL_GRID ? SPILL_GRID : fit);
}

size_t list_bytes(int n_max) { return ((size_t)n_max * sizeof(int) + 63) & ~(size_t)63; }
}  // namespace

extern "C" {

size_t ttl_tract_density_workspace_bytes(int32_t spill_slots, int32_t n_max) {
    if (!power_of_two(spill_slots) || spill_slots < 64 || spill_slots > MAX_SPILL_SLOTS ||
        n_max < 1)
        return 0;
    return WS_HEADER + list_bytes(n_max) +
           (size_t)spill_grid(spill_slots) * (size_t)spill_slots * sizeof(unsigned);
}

int ttl_tract_density(const ttl_density_desc *desc, const float *points, const int64_t *offsets,
                      int32_t n, int32_t *status, void *hip_stream) {
    if (!desc || !points || !offsets || !status || n < 0)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: bad arguments");
    if (desc->dims[0] < 1 || desc->dims[1] < 1 || desc->dims[2] < 1 ||
        (long long)desc->dims[0] * desc->dims[1] >= 2147483647LL ||
        (long long)desc->dims[0] * desc->dims[1] * desc->dims[2] >= 2147483647LL)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: dims must be >= 1 with X * Y * Z < 2^31 - 1");
    if (!desc->count && !desc->length_q && !desc->dec_q && !desc->ends)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: no map to add to");
    const int wave_slots = desc->wave_slots ? desc->wave_slots : DEFAULT_WAVE_SLOTS;
    if (!power_of_two(wave_slots) || wave_slots < 64 || wave_slots > TTL_DENSITY_MAX_WAVE_SLOTS)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: wave_slots must be a power of two in 64 .. %d",
                    TTL_DENSITY_MAX_WAVE_SLOTS);
    if (desc->spill_slots &&
        (!power_of_two(desc->spill_slots) || desc->spill_slots < 64 ||
         desc->spill_slots > MAX_SPILL_SLOTS))
        return fail(TTL_ERR_INVALID, "ttl_tract_density: spill_slots must be 0 or a power of two in 64 .. %d",
                    MAX_SPILL_SLOTS);
    if (desc->workspace && !desc->spill_slots)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: a workspace needs spill_slots");
    if (n == 0) return TTL_OK;
    const bool spill = desc->workspace && desc->count;
    if (desc->workspace &&
        desc->workspace_bytes < ttl_tract_density_workspace_bytes(desc->spill_slots, n))
        return fail(TTL_ERR_INVALID, "ttl_tract_density: the workspace holds %zu bytes, %d rows at "
                    "spill_slots = %d need %zu", desc->workspace_bytes, n, desc->spill_slots,
                    ttl_tract_density_workspace_bytes(desc->spill_slots, n));
    const size_t lds = ((size_t)WAVES * wave_slots + WAVES) * sizeof(unsigned);
    LdsRoom room;
    if (int rc = ttl_detail_reserve_lds((const void *)k_tract_density, lds, &room)) return rc;
    if (!room.fits)
        return fail(TTL_ERR_INVALID, "ttl_tract_density: wave_slots = %d exceeds the LDS of a workgroup",
                    wave_slots);
    const WalkDims D{{desc->dims[0], desc->dims[1], desc->dims[2]}};
    const Lin A = ttl_detail_lin<Lin>(desc->lin);
    const Maps M{desc->count, (u64 *)desc->length_q, (u64 *)desc->dec_q, desc->ends};
    char *ws = (char *)desc->workspace;
    unsigned *header = spill ? (unsigned *)ws : nullptr;
    int *list = spill ? (int *)(ws + WS_HEADER) : nullptr;
    hipLaunchKernelGGL(k_tract_density, dim3(ttl_detail_wave_grid(n, 8192)), dim3(BLOCK), lds,
                       (hipStream_t)hip_stream, points, (const long long *)offsets, n, D, A, M,
                       wave_slots, status, header, list);
    HIP_TRY(hipGetLastError());
    if (spill) {
        unsigned *tables = (unsigned *)(ws + WS_HEADER + list_bytes(n));
        hipLaunchKernelGGL(k_tract_density_spill, dim3(spill_grid(desc->spill_slots)), dim3(BLOCK),
                           0, (hipStream_t)hip_stream, points, (const long long *)offsets, D,
                           desc->count, desc->spill_slots, status, header, list, tables);
        HIP_TRY(hipGetLastError());
    }
    return TTL_OK;
}

}  // extern "C"
