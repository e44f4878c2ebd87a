// chunks.hip -- cut the speech out of (or drop it from) a resident batch, for every clip at once: the batched collect_chunks / drop_chunks
// of Silero/modeling_modified/utils_vad.py:588-631 / 634-682 (include/vadx.h, "Chunks").
//   vadx_chunks_plan   segment table + counts + clip lengths -> the PLAN record: per clip the resolved source intervals of its pieces and
//                      the prefix of their lengths, over the batch the prefix of the clips' (aligned) output lengths, the total, a status word;
//   vadx_chunks_copy   src + plan -> the packed output: clip after clip, each starting on a multiple of `align` elements, gaps zero.
// The copy is HBM-bound and does no arithmetic on a sample: 16-byte loads, a register-pair byte shift, 16-byte stores.
#include "common.h"

namespace vadx {
namespace chunks {

// ---- the plan record (byte offsets; every section 8-byte aligned, the record a multiple of 16 bytes) --------------------------------
//   0   int64 total          = clip_dst[B]: a fixed offset, so that a host reads 8 bytes and knows what to allocate
//   8   int32 status         VADX_CHUNKS_ST_* bits; 12: int32 reserved (0)
//   16  int64 clip_dst  [B+1]
//   ..  int64 piece_dst [B][cap+2]
//   ..  int64 piece_src [B][cap+1][2]
//   ..  int32 n_pieces  [B]
struct Layout {
    size_t clip_dst, piece_dst, piece_src, n_pieces, bytes;
};

__host__ __device__ inline Layout layout(long long B, long long cap) {
    Layout l;
    l.clip_dst = 16;
    l.piece_dst = l.clip_dst + 8 * (size_t)(B + 1);
    l.piece_src = l.piece_dst + 8 * (size_t)B * (size_t)(cap + 2);
    l.n_pieces = l.piece_src + 16 * (size_t)B * (size_t)(cap + 1);
    l.bytes = (l.n_pieces + 4 * (size_t)B + 15) & ~(size_t)15;
    return l;
}

struct Plan {
    long long *total;
    int *status;
    long long *clip_dst, *piece_dst, *piece_src;
    int *n_pieces;
};

__host__ __device__ inline Plan plan_of(void *rec, long long B, long long cap) {
    char *p = static_cast<char *>(rec);
    const Layout l = layout(B, cap);
    return Plan{reinterpret_cast<long long *>(p), reinterpret_cast<int *>(p + 8), reinterpret_cast<long long *>(p + l.clip_dst),
                reinterpret_cast<long long *>(p + l.piece_dst), reinterpret_cast<long long *>(p + l.piece_src),
                reinterpret_cast<int *>(p + l.n_pieces)};
}

// THE interval rule, once for both modes: Python's slice bound.  An index i < 0 counts from the end, then it is clamped to [0, len].
__device__ __forceinline__ long long slice_bound(long long i, long long len) {
    if (i < 0) i += len;                  // i < 0 <= len: the sum cannot overflow
    return i < 0 ? 0 : (i > len ? len : i);
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ long long wave_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// One WAVE per clip, lanes are pieces, 64 at a time with a carried prefix (the segmenter's shape: one wave owns one clip's table).
// collect: piece k = [start_k, end_k) for k < n.   drop: piece k = [end_{k-1}, start_k) with end_{-1} = 0, and the last piece [end_{n-1}, len).
// Every entry of the clip's rows is written: piece_dst[k] for k > n_pieces repeats the clip's output length (so entry cap+1 always holds
// it, and the row is monotone over its whole width), piece_src beyond n_pieces is (0, 0).  A BAD clip (count outside [0, cap] or a
// negative length) gets n_pieces = -1 and all-zero rows; its table rows are never read.
__global__ __launch_bounds__(256) void plan_clips_kernel(const long long *__restrict__ segs, const int *__restrict__ counts,
                                                         const long long *__restrict__ clip_len, int B, int cap, int mode, Plan P) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int n = counts[b];
    const long long len = clip_len[b];
    const bool bad = n < 0 || n > cap || len < 0;
    const int np = bad ? 0 : (mode == VADX_CHUNKS_DROP ? n + 1 : n);
    const long long *row = segs + b * (long long)cap * 2;
    long long *pd = P.piece_dst + b * (long long)(cap + 2), *ps = P.piece_src + b * (long long)(cap + 1) * 2;
    long long carry = 0;
    for (int k0 = 0; k0 < cap + 2; k0 += 64) {
        const int k = k0 + lane;
        long long lo = 0, hi = 0;
        if (k < np) {
            if (mode == VADX_CHUNKS_DROP) {
                lo = k == 0 ? 0 : slice_bound(row[2 * (k - 1) + 1], len);
                hi = k == n ? len : slice_bound(row[2 * k], len);
            } else {
                lo = slice_bound(row[2 * k], len);
                hi = slice_bound(row[2 * k + 1], len);
            }
            if (hi < lo) hi = lo;             // lo >= hi: empty
        }
        const long long incl = wave_scan(hi - lo, lane);
        if (k < cap + 2) pd[k] = carry + incl - (hi - lo);
        if (k < cap + 1) {
            ps[2 * k] = lo;
            ps[2 * k + 1] = hi;
        }
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) P.n_pieces[b] = bad ? -1 : np;
}

// The cross-clip prefix: ONE workgroup of 1024 walks the clips 1024 at a time with a carried 64-bit prefix (B = 2^20 is 1024 rounds).
// clip_dst[b + 1] = clip_dst[b] + round_up(length of clip b, align): every clip starts on a multiple of align, and so does the total.
__global__ __launch_bounds__(1024) void plan_prefix_kernel(int B, int cap, long long align, Plan P) {
    __shared__ long long wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    int bad = 0;
    for (long long base = 0; base < B; base += 1024) {
        const long long b = base + tid;
        long long v = 0;
        if (b < B) {
            v = (P.piece_dst[b * (cap + 2) + cap + 1] + align - 1) & ~(align - 1);
            bad |= P.n_pieces[b] < 0;
        }
        const long long incl = wave_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long s = wsum[w];
            if (w < wave) before += s;
            all += s;
        }
        if (b < B) P.clip_dst[b] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        P.clip_dst[B] = carry;
        *P.total = carry;
        P.status[0] = bad ? VADX_CHUNKS_ST_BAD_CLIP : 0;
        P.status[1] = 0;
    }
}

// ---- the copy -----------------------------------------------------------------------------------------------------------------------
constexpr int COPY_THREADS = 256, COPY_ROWS = 4, TILE_BYTES = COPY_THREADS * COPY_ROWS * 16;       // 16 KB of destination per workgroup

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// largest i in [lo, hi] with a[i] <= x (a is non-decreasing and a[lo] <= x)
__device__ __forceinline__ long long last_le(const long long *__restrict__ a, long long lo, long long hi, long long x) {
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Where destination element d comes from: `gap` (an alignment gap, written as zero) or source element `src`, and `end` = the first
// destination element after d that this answer does not cover (the end of the piece, or of the gap).  [b_lo, b_hi] brackets d's clip.
// `end` > d whatever the record holds, so that a walk that follows it always advances.
struct Loc {
    long long src, end;
    bool gap;
};

__device__ __forceinline__ Loc locate(const Plan &P, const long long *__restrict__ clip_src, int cap, long long b_lo, long long b_hi, long long d) {
    const long long b = last_le(P.clip_dst, b_lo, b_hi, d);
    const long long at = P.clip_dst[b], local = d - at;
    const long long *pd = P.piece_dst + b * (long long)(cap + 2);
    int np = P.n_pieces[b];
    np = np < 0 ? 0 : (np > cap + 1 ? cap + 1 : np);
    Loc l;
    if (np == 0 || local >= pd[np]) {
        l = Loc{0, P.clip_dst[b + 1], true};
    } else {
        const long long k = last_le(pd, 0, np - 1, local);      // among pieces that start here, the last: the one that is not empty
        l = Loc{clip_src[b] + P.piece_src[(b * (long long)(cap + 1) + k) * 2] + (local - pd[k]), at + pd[k + 1], false};
    }
    if (l.end <= d) l.end = d + 1;
    return l;
}

// Work is laid out over DESTINATION tiles of 16 KB: a thread owns COPY_ROWS 16-byte vectors, 4 KB apart (a wave's stores are one 1 KB run).
// A vector that lies inside one piece, whose source vectors lie inside src, is moved as 16 bytes: an aligned load when the source has the
// destination's residue, otherwise the two aligned vectors around it and a byte shift of the register pair.  Every other vector (a seam,
// a gap's edge, the end of the output, a source within a vector of src's end) goes element by element.
template <typename T>
__global__ __launch_bounds__(COPY_THREADS) void copy_kernel(const T *__restrict__ src, long long src_elems, const long long *__restrict__ clip_src,
                                                            Plan P, int B, int cap, T *__restrict__ dst, long long dst_elems) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr long long TILE = TILE_BYTES / (long long)sizeof(T);
    const long long total = *P.total;
    if (total < 0 || total > dst_elems) {                       // nothing at all is written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(P.status, VADX_CHUNKS_ST_OVERFLOW);
        return;
    }
    const long long t0 = (long long)blockIdx.x * TILE;
    if (t0 >= total) return;
    const long long t1 = t0 + TILE < total ? t0 + TILE : total;
    // the tile's clips, found once per workgroup (uniform addresses): a thread then searches [b_lo, b_hi] only
    const long long b_lo = last_le(P.clip_dst, 0, B - 1, t0), b_hi = last_le(P.clip_dst, b_lo, B - 1, t1 - 1);
    Loc loc{0, t0, true};                                       // covers nothing yet
    long long loc_d = t0;                                       // the destination element loc.src belongs to
    bool outside = false;
    for (int r = 0; r < COPY_ROWS; ++r) {
        const long long d0 = t0 + ((long long)r * COPY_THREADS + threadIdx.x) * VEC;
        if (d0 >= t1) break;
        if (d0 >= loc.end) {
            loc = locate(P, clip_src, cap, b_lo, b_hi, d0);
            loc_d = d0;
        }
        u32x4 *out = reinterpret_cast<u32x4 *>(dst + d0);
        if (d0 + VEC <= loc.end && d0 + VEC <= t1) {
            if (loc.gap) {
                *out = u32x4{0, 0, 0, 0};
                continue;
            }
            const long long s0 = loc.src + (d0 - loc_d), sa = s0 & ~(long long)(VEC - 1);
            const int sh = (int)(s0 - sa) * (int)sizeof(T);     // bytes, 0 .. 14
            if (sa >= 0 && sa + (sh ? 2 * VEC : VEC) <= src_elems) {
                const u32x4 *in = reinterpret_cast<const u32x4 *>(src + sa);
                const u32x4 a = in[0];
                if (sh == 0) {
                    *out = a;
                    continue;
                }
                const u32x4 c = in[1];
                const unsigned int w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
                const int q = sh >> 2, bits = (sh & 3) * 8;
                unsigned int o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned int lo = q == 0 ? w[j] : q == 1 ? w[j + 1] : q == 2 ? w[j + 2] : w[j + 3];
                    const unsigned int hi = q == 0 ? w[j + 1] : q == 1 ? w[j + 2] : q == 2 ? w[j + 3] : w[j + 4];
                    o[j] = (unsigned int)((((unsigned long long)hi << 32) | lo) >> bits);
                }
                *out = u32x4{o[0], o[1], o[2], o[3]};
                continue;
            }
        }
        // element by element, piece by piece
        long long d = d0;
        const long long dend = d0 + VEC < t1 ? d0 + VEC : t1;
        while (d < dend) {
            if (d >= loc.end) {
                loc = locate(P, clip_src, cap, b_lo, b_hi, d);
                loc_d = d;
            }
            const long long stop = loc.end < dend ? loc.end : dend;
            for (; d < stop; ++d) {
                T v = T(0);
                if (!loc.gap) {
                    const long long s = loc.src + (d - loc_d);
                    if (s >= 0 && s < src_elems) v = src[s];
                    else outside = true;
                }
                dst[d] = v;
            }
        }
    }
    if (outside) atomicOr(P.status, VADX_CHUNKS_ST_SRC_RANGE);
}

inline bool pow2_in(long long v, long long lo, long long hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

}  // namespace chunks
}  // namespace vadx

using namespace vadx::chunks;

extern "C" size_t vadx_chunks_plan_bytes(int batch, int cap) {
    if (batch < 1 || cap < 1) return 0;
    return layout(batch, cap).bytes;
}

extern "C" int vadx_chunks_plan(const int64_t *segments, const int32_t *counts, const int64_t *clip_len, int batch, int cap, int mode, int align,
                                void *plan, size_t plan_bytes, void *stream) {
    VADX_REQUIRE(segments, "vadx_chunks_plan: segments is NULL");
    VADX_REQUIRE(counts, "vadx_chunks_plan: counts is NULL");
    VADX_REQUIRE(clip_len, "vadx_chunks_plan: clip_len is NULL");
    VADX_REQUIRE(plan, "vadx_chunks_plan: plan is NULL");
    VADX_REQUIRE(batch >= 1, "vadx_chunks_plan: batch=%d must be positive", batch);
    VADX_REQUIRE(cap >= 1, "vadx_chunks_plan: cap=%d must be positive", cap);
    VADX_REQUIRE(mode == VADX_CHUNKS_COLLECT || mode == VADX_CHUNKS_DROP, "vadx_chunks_plan: mode=%d must be VADX_CHUNKS_COLLECT or VADX_CHUNKS_DROP", mode);
    VADX_REQUIRE(pow2_in(align, 1, 4096), "vadx_chunks_plan: align=%d must be a power of two in [1, 4096]", align);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(segments) | reinterpret_cast<uintptr_t>(clip_len)) & 7) == 0 && (reinterpret_cast<uintptr_t>(counts) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(plan) & 15) == 0,
                 "vadx_chunks_plan: segments and clip_len must be 8-byte aligned, counts 4-byte, plan 16-byte");
    VADX_REQUIRE(plan_bytes >= layout(batch, cap).bytes, "vadx_chunks_plan: plan_bytes=%zu is smaller than vadx_chunks_plan_bytes(%d, %d)=%zu", plan_bytes,
                 batch, cap, layout(batch, cap).bytes);
    const Plan P = plan_of(plan, batch, cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(plan_clips_kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const long long *>(segments), counts,
                       reinterpret_cast<const long long *>(clip_len), batch, cap, mode, P);
    VADX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(plan_prefix_kernel, dim3(1), dim3(1024), 0, s, batch, cap, (long long)align, P);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_chunks_copy(const void *src, int64_t src_elems, const int64_t *clip_src, int elem_bytes, void *plan, size_t plan_bytes, int batch,
                                int cap, void *dst, int64_t dst_elems, void *stream) {
    VADX_REQUIRE(src, "vadx_chunks_copy: src is NULL");
    VADX_REQUIRE(clip_src, "vadx_chunks_copy: clip_src is NULL");
    VADX_REQUIRE(plan, "vadx_chunks_copy: plan is NULL");
    VADX_REQUIRE(dst, "vadx_chunks_copy: dst is NULL");
    VADX_REQUIRE(batch >= 1, "vadx_chunks_copy: batch=%d must be positive", batch);
    VADX_REQUIRE(cap >= 1, "vadx_chunks_copy: cap=%d must be positive", cap);
    VADX_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "vadx_chunks_copy: elem_bytes=%d must be 2 (int16) or 4 (float32)", elem_bytes);
    VADX_REQUIRE(src_elems >= 0 && dst_elems >= 0, "vadx_chunks_copy: src_elems=%lld and dst_elems=%lld must not be negative", (long long)src_elems,
                 (long long)dst_elems);
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(src) & 15) == 0, "vadx_chunks_copy: src must be 16-byte aligned");
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "vadx_chunks_copy: dst must be 16-byte aligned");
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(clip_src) & 7) == 0 && (reinterpret_cast<uintptr_t>(plan) & 15) == 0,
                 "vadx_chunks_copy: clip_src must be 8-byte aligned, plan 16-byte");
    VADX_REQUIRE(plan_bytes >= layout(batch, cap).bytes, "vadx_chunks_copy: plan_bytes=%zu is smaller than vadx_chunks_plan_bytes(%d, %d)=%zu", plan_bytes,
                 batch, cap, layout(batch, cap).bytes);
    const long long tile = TILE_BYTES / elem_bytes;
    const long long tiles = dst_elems / tile + (dst_elems % tile ? 1 : 0);
    VADX_REQUIRE(tiles < (1ll << 31), "vadx_chunks_copy: dst_elems=%lld makes %lld tiles of %lld elements, must be < 2^31", (long long)dst_elems, tiles, tile);
    const Plan P = plan_of(plan, batch, cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(tiles > 0 ? tiles : 1));         // one workgroup even for an empty dst: it is what reports an overflow
    if (elem_bytes == 2)
        hipLaunchKernelGGL(copy_kernel<int16_t>, grid, dim3(COPY_THREADS), 0, s, static_cast<const int16_t *>(src), (long long)src_elems,
                           reinterpret_cast<const long long *>(clip_src), P, batch, cap, static_cast<int16_t *>(dst), (long long)dst_elems);
    else
        hipLaunchKernelGGL(copy_kernel<uint32_t>, grid, dim3(COPY_THREADS), 0, s, static_cast<const uint32_t *>(src), (long long)src_elems,
                           reinterpret_cast<const long long *>(clip_src), P, batch, cap, static_cast<uint32_t *>(dst), (long long)dst_elems);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
