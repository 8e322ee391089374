// ttl_tract.hip -- the tracker's output stage on the device: the
// arc-length filter of TrackToLearn/tracking/tracker.py:120-121, the greedy
// linearisation of tractogram.compress_streamline and the ragged pack of what
// survives; part of libttl_hip.so.  Kernels over the env's history buffer,
// one wavefront per streamline each, with an exclusive prefix sum (the
// caller's) between select and emit:
//   k_tract_select     kept length, float64 arc, accept, survivor bitmask + count
//   k_tract_emit       survivors -> packed points, compacted counts and rows
//   k_tract_emit_file  survivors -> the .trk / .tck records of the batch
// (the two emits are one walk of a row's survivors, walk_accepted_row)
// and the pack without a filter, of env.get_streamlines():
//   k_pack_streamlines the first keep[i] points of every row
// All float64 arithmetic is plain IEEE (no fused multiply-add), in the order
// include/ttl_hip.h states.
#include "ttl_internal.h"

#pragma clang fp contract(off)

namespace {
constexpr int BLOCK = TTL_BLOCK;
constexpr int WAVES = BLOCK / 64;
// points of one row a wave stages in the LDS (float32, 12 B each: 4.5 KB per
// wave); longer rows read the history from global memory instead
constexpr int STAGE_PTS = 384;

struct D3 {
    double x, y, z;
};

__device__ __forceinline__ D3 point(const float *__restrict__ p, int j) {
    return D3{(double)p[3 * j], (double)p[3 * j + 1], (double)p[3 * j + 2]};
}

// bits [64 w, 64 w + 64) of the mask whose first `keep` bits are set
__device__ __forceinline__ unsigned long long prefix_word(int w, int keep) {
    const int left = keep - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

// The greedy compression of the first `keep` (> 2) points of p (LDS or global);
// survivor words go to mrow[0 .. nwords), the survivor count is returned.  Every
// variable that steers the loops is the same in all 64 lanes.
__device__ int compress_row(const float *__restrict__ p, int keep, double tol, double max_seg,
                            unsigned long long *__restrict__ mrow, int nwords, int lane) {
    int wcur = 0, count = 1, prev = 0;
    unsigned long long word = 1ull;                  // point 0
    auto keep_point = [&](int k) {
        const int w = k >> 6;
        while (wcur < w) {
            if (lane == 0) mrow[wcur] = word;
            word = 0ull;
            ++wcur;
        }
        word |= 1ull << (k & 63);
        ++count;
    };
    for (int nxt = 2; nxt < keep; ++nxt) {
        const D3 a = point(p, prev), b = point(p, nxt);
        const double abx = b.x - a.x, aby = b.y - a.y, abz = b.z - a.z;
        const double L = sqrt(abx * abx + aby * aby + abz * abz);
        bool ok = L <= max_seg;
        if (ok) {
            const double LL = L * L;
            for (int j0 = prev + 1; j0 < nxt; j0 += 64) {
                const int j = j0 + lane;
                bool bad = false;
                if (j < nxt) {
                    const D3 c = point(p, j);
                    double dx = c.x - a.x, dy = c.y - a.y, dz = c.z - a.z;
                    if (L > 0.0) {
                        double t = (dx * abx + dy * aby + dz * abz) / LL;
                        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
                        dx = dx - t * abx;
                        dy = dy - t * aby;
                        dz = dz - t * abz;
                    }
                    bad = !(sqrt(dx * dx + dy * dy + dz * dz) <= tol);
                }
                if (__ballot(bad) != 0ull) {
                    ok = false;
                    break;
                }
            }
        }
        if (!ok) {
            keep_point(nxt - 1);
            prev = nxt - 1;
        }
    }
    keep_point(keep - 1);
    while (wcur < nwords) {
        if (lane == 0) mrow[wcur] = word;
        word = 0ull;
        ++wcur;
    }
    return count;
}

template <bool STAGED>
__global__ __launch_bounds__(BLOCK) void k_tract_select(
    const float *__restrict__ hist, long long row_pitch, const int *__restrict__ lengths,
    const int *__restrict__ flags, int n, double min_arc, double max_arc, double tol,
    double max_seg, int *__restrict__ counts, int *__restrict__ accepted,
    unsigned long long *__restrict__ mask, int nwords) {
    __shared__ float stage[STAGED ? WAVES * STAGE_PTS * 3 : 1];
    const int i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int T = (int)(row_pitch / 3);
    int keep = lengths[i] - ((flags[i] & (TTL_FLAG_CURVATURE | TTL_FLAG_MASK)) != 0 ? 1 : 0);
    keep = keep < 0 ? 0 : (keep > T ? T : keep);
    const float *p = hist + (size_t)i * (size_t)row_pitch;
    if (STAGED) {
        float *s = stage + (threadIdx.x >> 6) * (STAGE_PTS * 3);
        for (int f = lane; f < 3 * keep; f += 64) s[f] = p[f];
        wave_sync();
        p = s;
    }
    // arc length: float32 differences widened to float64; lane l sums segments l, l + 64,
    // ... in that order, then a fixed butterfly adds the 64 partial sums (every lane ends
    // with the same bits: each level adds the same two values in both lanes of a pair)
    double arc = 0.0;
    for (int j = lane; j < keep - 1; j += 64) {
        const double dx = (double)(p[3 * j + 3] - p[3 * j]);
        const double dy = (double)(p[3 * j + 4] - p[3 * j + 1]);
        const double dz = (double)(p[3 * j + 5] - p[3 * j + 2]);
        arc += sqrt(dx * dx + dy * dy + dz * dz);
    }
    for (int m = 32; m >= 1; m >>= 1) arc += __shfl_xor(arc, m, 64);
    arc = __shfl(arc, 0, 64);
    const bool ok = min_arc <= arc && arc <= max_arc;
    unsigned long long *mrow = mask + (size_t)i * (size_t)nwords;
    int count;
    if (ok && tol > 0.0 && keep > 2) {
        count = compress_row(p, keep, tol, max_seg, mrow, nwords, lane);
    } else {
        count = ok ? keep : 0;
        for (int w = lane; w < nwords; w += 64) mrow[w] = prefix_word(w, count);
    }
    if (lane == 0) {
        counts[i] = count;
        accepted[i] = ok ? 1 : 0;
    }
}

// The walk of an accepted row's survivors, stated once for the two emit kernels: the wave's
// row (a row that is not accepted is left at once), its place in the output -- accepted
// row k, with b points in the rows before it --, then per 64-point word of the mask that
// has a survivor: c of them, starting at `from` in the row.  The kernel says what happens to
// a word and where the barriers stand:
//   open(i, lane, count, k, b)               once, before the first word
//   word(prefix, from, s, c, lane, compact)  `prefix`: the word's set bits are its lowest
//       ones, the c points at `from` are the survivors; any other word the kernel has compacted
//       into s, the wave's 192 words of `pack`, by calling compact(): the survivors do it
//       themselves (survivor r of the word writes words 3 r .. 3 r + 2), without a barrier
//   close(i, lane)                           once, behind the last word
template <class W, class Open, class Word, class Close>
__device__ __forceinline__ void walk_accepted_row(
    const W *__restrict__ hist, long long row_pitch, int n, const int *__restrict__ counts,
    const int *__restrict__ accepted, const long long *__restrict__ count_ends,
    const long long *__restrict__ accept_ends, const unsigned long long *__restrict__ mask,
    int nwords, W *pack, Open open, Word each_word, Close close) {
    const int i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n || !accepted[i]) return;
    const int lane = threadIdx.x & 63;
    const int count = counts[i];
    open(i, lane, count, accept_ends[i] - 1, count_ends[i] - count);
    const W *src = hist + (size_t)i * (size_t)row_pitch;
    const unsigned long long *mrow = mask + (size_t)i * (size_t)nwords;
    W *s = pack + (threadIdx.x >> 6) * 192;
    for (int w = 0; w < nwords; ++w) {
        const unsigned long long word = mrow[w];
        if (word == 0ull) continue;
        const int c = __popcll(word);
        const W *from = src + (size_t)w * 192;
        each_word((word & (word + 1ull)) == 0ull, from, s, c, lane, [&] {
            if ((word >> lane) & 1ull) {
                const int r = __popcll(word & ((1ull << lane) - 1ull));
                s[3 * r] = from[3 * lane];
                s[3 * r + 1] = from[3 * lane + 1];
                s[3 * r + 2] = from[3 * lane + 2];
            }
        });
    }
    close(i, lane);
}

// Survivors of the accepted rows, streamline-major: a prefix word is a straight copy from
// the row to the packed output, a compacted one is stored from the LDS, so that the stores
// run along the packed output either way.
__global__ __launch_bounds__(BLOCK) void k_tract_emit(
    const float *__restrict__ hist, long long row_pitch, int n, const int *__restrict__ counts,
    const int *__restrict__ accepted, const long long *__restrict__ count_ends,
    const long long *__restrict__ accept_ends, const unsigned long long *__restrict__ mask,
    int nwords, float *__restrict__ points_out, long long *__restrict__ counts_out,
    int *__restrict__ rows_out) {
    __shared__ float pack[WAVES * 192];
    float *dst;
    walk_accepted_row(
        hist, row_pitch, n, counts, accepted, count_ends, accept_ends, mask, nwords, pack,
        [&](int i, int lane, int count, long long k, long long b) {
            if (lane == 0) {
                counts_out[k] = count;
                rows_out[k] = i;
            }
            dst = points_out + 3 * (size_t)b;
        },
        [&](bool prefix, const float *from, const float *s, int c, int lane, auto compact) {
            if (prefix) {
                for (int f = lane; f < 3 * c; f += 64) dst[f] = from[f];
            } else {
                compact();
                wave_sync();
                for (int f = lane; f < 3 * c; f += 64) dst[f] = s[f];
                wave_sync();
            }
            dst += 3 * c;
        },
        [](int, int) {});
}

// Where record k of a file body starts when the records before it hold b points, in 4-byte
// words (include/ttl_hip.h); at (accepted rows, points) of a batch: the size of its body.
__host__ __device__ inline long long record_start(int format, int n_props, long long k,
                                                  long long b) {
    return format == TTL_TRACT_FILE_TRK ? k * (1 + n_props) + 3 * b : 3 * (b + k);
}

// One point through the descriptor's steps (include/ttl_hip.h); d is uniform over the grid.
__device__ __forceinline__ void file_point(const ttl_tract_file_desc &d, float x, float y,
                                           float z, unsigned int out[3]) {
    double v[3];
    if (d.has_pre) {
        const float t[3] = {x + 0.5f, y + 0.5f, z + 0.5f};
        for (int c = 0; c < 3; ++c) v[c] = (double)(float)((double)t[c] * d.pre_scale);
    } else {
        v[0] = (double)x, v[1] = (double)y, v[2] = (double)z;
    }
    for (int m = 0; m < d.n_maps; ++m) {
        const double *a = d.maps[m];
        double o[3];
        for (int i = 0; i < 3; ++i)
            o[i] = ((v[0] * a[4 * i] + v[1] * a[4 * i + 1]) + v[2] * a[4 * i + 2]) + a[4 * i + 3];
        v[0] = o[0], v[1] = o[1], v[2] = o[2];
    }
    if (d.has_post)
        for (int c = 0; c < 3; ++c) v[c] = (v[c] + 0.5) * d.post_scale[c];
    for (int c = 0; c < 3; ++c) out[c] = __float_as_uint((float)v[c]);
}

// k_tract_emit writing file records (TTL_HAS_TRACT_FILE): every word of the mask is staged
// in the LDS (a prefix word with loads along the row, any other by its survivors), lane r
// converts survivor r in place, and the stores run along the body one dword per lane.  The
// count word in front of a .trk record, the seed or NaN words behind a record close it.
__global__ __launch_bounds__(BLOCK) void k_tract_emit_file(
    const float *__restrict__ hist, long long row_pitch, int n, const int *__restrict__ counts,
    const int *__restrict__ accepted, const long long *__restrict__ count_ends,
    const long long *__restrict__ accept_ends, const unsigned long long *__restrict__ mask,
    int nwords, const double *__restrict__ seeds, const ttl_tract_file_desc d,
    unsigned int *__restrict__ words_out) {
    __shared__ unsigned int pack[WAVES * 192];
    const bool trk = d.format == TTL_TRACT_FILE_TRK;
    const int P = trk ? d.n_props : 0;
    unsigned int *dst;
    walk_accepted_row(
        (const unsigned int *)hist, row_pitch, n, counts, accepted, count_ends, accept_ends, mask,
        nwords, pack,
        [&](int, int lane, int count, long long k, long long b) {
            dst = words_out + record_start(d.format, P, k, b);
            if (trk) {
                if (lane == 0) dst[0] = (unsigned int)count;
                ++dst;
            }
        },
        [&](bool prefix, const unsigned int *from, unsigned int *s, int c, int lane,
            auto compact) {
            if (prefix)
                for (int f = lane; f < 3 * c; f += 64) s[f] = from[f];
            else
                compact();
            wave_sync();
            if (lane < c) {          // a lane reads and writes its own three words only
                unsigned int q[3];
                file_point(d, __uint_as_float(s[3 * lane]), __uint_as_float(s[3 * lane + 1]),
                           __uint_as_float(s[3 * lane + 2]), q);
                s[3 * lane] = q[0];
                s[3 * lane + 1] = q[1];
                s[3 * lane + 2] = q[2];
            }
            wave_sync();
            for (int f = lane; f < 3 * c; f += 64) dst[f] = s[f];
            wave_sync();
            dst += 3 * c;
        },
        [&](int i, int lane) {
            if (lane < 3) {
                if (!trk)
                    dst[lane] = 0x7fc00000u;
                else if (P == 3)
                    dst[lane] = __float_as_uint((float)(seeds[3 * (size_t)i + lane] - 0.5));
            }
        });
}

// ragged pack of the tracked streamlines (tracking_env.py:263-284: the first
// keep[i] points of streamline i, one after the other): one wave per streamline
__global__ __launch_bounds__(BLOCK) void k_pack_streamlines(
    const float *__restrict__ hist, long long row_pitch, const long long *__restrict__ keep,
    const long long *__restrict__ offsets, int n, float *__restrict__ out) {
    const int i = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int floats = (int)keep[i] * 3;
    const float *src = hist + (size_t)i * (size_t)row_pitch;
    float *dst = out + (size_t)offsets[i] * 3;
    for (int f = lane; f < floats; f += 64) dst[f] = src[f];
}

// the argument check the three ttl_tract_* launches share
int check_rows(const char *who, int32_t n, int64_t row_pitch) {
    if (n < 0 || row_pitch < 3 || row_pitch / 3 > INT32_MAX / 4)
        return fail(TTL_ERR_INVALID, "%s: n=%d, row_pitch=%lld", who, n, (long long)row_pitch);
    return TTL_OK;
}

// the grid of every kernel here: one wave per row
dim3 wave_per_row(int n) { return dim3((n + WAVES - 1) / WAVES); }
}  // namespace

extern "C" {

int32_t ttl_tract_mask_words(int64_t row_pitch) {
    return row_pitch < 3 ? 0 : (int32_t)((row_pitch / 3 + 63) / 64);
}

int32_t ttl_tract_stage_points(void) { return STAGE_PTS; }

int ttl_tract_select(const float *history, int64_t row_pitch, const int32_t *lengths,
                     const int32_t *flags, int32_t n, double min_arc, double max_arc,
                     double tol_error, double max_segment_length, int32_t *counts,
                     int32_t *accepted, uint64_t *mask, void *hip_stream) {
    if (const int rc = check_rows("ttl_tract_select", n, row_pitch)) return rc;
    if (n == 0) return TTL_OK;
    if (!history || !lengths || !flags || !counts || !accepted || !mask)
        return fail(TTL_ERR_INVALID, "ttl_tract_select: null argument");
    if (!(tol_error >= 0.0) || max_segment_length != max_segment_length ||
        min_arc != min_arc || max_arc != max_arc)
        return fail(TTL_ERR_INVALID, "ttl_tract_select: tol_error must be >= 0 and no bound NaN");
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, wave_per_row(n), dim3(BLOCK), 0, (hipStream_t)hip_stream, history,
                           (long long)row_pitch, lengths, flags, n, min_arc, max_arc, tol_error,
                           max_segment_length, counts, accepted, (unsigned long long *)mask,
                           ttl_tract_mask_words(row_pitch));
    };
    if (row_pitch / 3 <= STAGE_PTS) launch(k_tract_select<true>);
    else launch(k_tract_select<false>);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_tract_emit(const float *history, int64_t row_pitch, int32_t n, const int32_t *counts,
                   const int32_t *accepted, const int64_t *count_ends,
                   const int64_t *accept_ends, const uint64_t *mask, float *points_out,
                   int64_t *counts_out, int32_t *rows_out, void *hip_stream) {
    if (const int rc = check_rows("ttl_tract_emit", n, row_pitch)) return rc;
    if (n == 0) return TTL_OK;
    // points_out may be null when no point survives; the kernel then stores none
    if (!history || !counts || !accepted || !count_ends || !accept_ends || !mask ||
        !counts_out || !rows_out)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit: null argument");
    hipLaunchKernelGGL(k_tract_emit, wave_per_row(n), dim3(BLOCK), 0, (hipStream_t)hip_stream, history, (long long)row_pitch, n, counts, accepted,
                       (const long long *)count_ends, (const long long *)accept_ends,
                       (const unsigned long long *)mask,
                       ttl_tract_mask_words(row_pitch), points_out, (long long *)counts_out,
                       rows_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int64_t ttl_tract_file_words(int32_t format, int32_t n_props, int64_t k, int64_t M) {
    if ((n_props != 0 && n_props != 3) || k < 0 || M < 0 ||
        (format != TTL_TRACT_FILE_TRK && format != TTL_TRACT_FILE_TCK))
        return -1;
    return record_start(format, n_props, k, M);
}

int ttl_tract_emit_file(const float *history, int64_t row_pitch, int32_t n, const int32_t *counts,
                        const int32_t *accepted, const int64_t *count_ends,
                        const int64_t *accept_ends, const uint64_t *mask, const double *seeds,
                        const ttl_tract_file_desc *desc, uint32_t *words_out, void *hip_stream) {
    if (const int rc = check_rows("ttl_tract_emit_file", n, row_pitch)) return rc;
    if (!desc) return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: null descriptor");
    if (desc->format != TTL_TRACT_FILE_TRK && desc->format != TTL_TRACT_FILE_TCK)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: unknown format %d", desc->format);
    if (desc->n_props != 0 && desc->n_props != 3)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: n_props=%d (0 or 3)", desc->n_props);
    if (desc->n_props == 3 && !seeds)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: n_props=3 without seeds");
    if (desc->n_maps < 0 || desc->n_maps > 2)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: n_maps=%d (at most 2)", desc->n_maps);
    if (n == 0) return TTL_OK;
    // words_out may be null when no row is accepted; the kernel then stores nothing
    if (!history || !counts || !accepted || !count_ends || !accept_ends || !mask)
        return fail(TTL_ERR_INVALID, "ttl_tract_emit_file: null argument");
    hipLaunchKernelGGL(k_tract_emit_file, wave_per_row(n), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, history, (long long)row_pitch, n, counts, accepted,
                       (const long long *)count_ends, (const long long *)accept_ends,
                       (const unsigned long long *)mask, ttl_tract_mask_words(row_pitch), seeds,
                       *desc, words_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

int ttl_pack_streamlines(const float *history, int64_t row_pitch, const int64_t *keep,
                         const int64_t *offsets, int32_t n, float *points_out,
                         void *hip_stream) {
    if (!history || !keep || !offsets || !points_out || n < 1 || row_pitch < 3)
        return fail(TTL_ERR_INVALID, "ttl_pack_streamlines: bad arguments");
    hipLaunchKernelGGL(k_pack_streamlines, wave_per_row(n), dim3(BLOCK), 0,
                       (hipStream_t)hip_stream, history, (long long)row_pitch,
                       (const long long *)keep, (const long long *)offsets, n, points_out);
    HIP_TRY(hipGetLastError());
    return TTL_OK;
}

}  // extern "C"
