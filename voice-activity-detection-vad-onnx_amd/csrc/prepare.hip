// prepare.hip -- a ragged batch prepared on the device (include/vadx.h, "Prepare"): what the host does per clip between "PCM of B clips"
// and "the packed vector of vadx.ragged", for every clip at once and bit for bit:
//   normalize_to_int16   PEAK  p = max|x|, s = 32767 / p (1 when p = 0), y = trunc(x * s)                  (FSMN/Inference_FSMN_VAD_ONNX.py:60-63)
//   normalise_audio      RMS   r = sqrt(mean(x * x)); unless r > 0 the clip stays; g = target / (r + 1e-7),
//                              y = trunc(clip(x * g, -32768, 32767))                          (Inference_NVIDIA_MarbleNet_VAD_ONNX.py:110-118)
//   pad_to_window_grid   fill_k = int16(sqrt(mean(ref * ref)) * z_k), ref = the tail of y                  (FSMN/Inference_FSMN_VAD_ONNX.py:88-99)
//   vadx_prepare_stats   per (clip, 8192-sample chunk): the peak and the pairwise sum of squares -> workspace;
//   vadx_prepare_scale   per clip: the chunk partials folded in order -> s or g, then the RMS of the tail of the NORMALISED samples -> record;
//   vadx_prepare_write   per 16 KB of the packed output: normalised samples, then the noise fill.
// and, for the step before them, vadx_ingest_pcm16_ragged: ingest.hip's closed form over clips of any lengths, channel counts and rates.
//
// THE ARITHMETIC.  All of it is float32 that numpy does one rounded operation at a time, so
//   * nothing may be contracted: `r + x * x` as an FMA rounds once where numpy rounds the square and then the sum.  hipcc contracts device
//     code by default, so contraction is off for the whole file (as in timestamps.hip) and every product and sum is a plain operator
//     WRITTEN HERE.  __fmul_rn / __fadd_rn must not be used: they are plain operators too, but in a header compiled with contraction
//     on, and a product and a sum that both carry that licence are fused after inlining (seen: tail RMS values an ulp off);
//   * division and square root must be correctly rounded.  They are computed in float64 and rounded to float32 (div32, sqrt32 below):
//     float64 division and square root are IEEE operations on this hardware whatever the compile flags, and rounding a correctly rounded
//     53-bit quotient or root of float32 operands to 24 bits gives the correctly rounded float32 result (double rounding is innocuous
//     for / and sqrt once the wide format has 2 * 24 + 2 bits).  hipcc's __fsqrt_rn is NOT that: it is the native approximation unless
//     OCML_BASIC_ROUNDED_OPERATIONS is defined.  Each runs once per clip;
//   * the mean of squares is numpy's own summation order, `ms32`: the squares are summed in consecutive CHUNKS of 8192 elements (numpy's
//     reduction buffer), the chunk sums added in order; inside a chunk the sum is numpy's pairwise tree -- n < 8: in order; n <= 128:
//     eight accumulators r[j] += a[i + j], combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in order; otherwise the
//     halves split at n/2 - (n/2) % 8.  A chunk has at most 128 such leaves at a depth of at most 7: a workgroup of 1024 threads gives
//     every leaf eight lanes (the eight accumulators) and folds the tree through LDS.  float32 addition is commutative, so which lane
//     holds which side of a sum does not matter; the ASSOCIATION is what is kept.
#pragma clang fp contract(off)
#include "common.h"

namespace vadx {
namespace prepare {

constexpr int CHUNK = 8192;            // numpy's reduction buffer, in elements: part of the arithmetic contract
constexpr int LEAF = 128;              // numpy's PW_BLOCKSIZE
constexpr int MAX_LEAVES = 128;        // of a chunk of <= 8192 elements: sizes fall to <= 79 after seven splits
constexpr int THREADS = 8 * MAX_LEAVES;

struct Part {                          // one (clip, chunk): 8 bytes
    float sum;
    int peak;
};

struct Rec {                           // one clip: 16 bytes
    float scale, tail_rms;
    int status, reserved;
};

__host__ __device__ inline size_t parts_at(long long B) { return 16 * (size_t)B; }
__host__ __device__ inline size_t ws_bytes(long long B, long long tiles) { return (parts_at(B) + 8 * (size_t)tiles + 15) & ~(size_t)15; }

// What the clip's tables say about its source: usable only when [off, off + n) lies inside src.
__device__ __forceinline__ bool clip_bad(long long off, long long n, long long src_elems) {
    return n < 1 || off < 0 || off > src_elems || n > src_elems - off;
}

// pad_to_window_grid's pad count: a function of n, window and stride alone.
__device__ __forceinline__ long long pad_count(long long n, long long window, long long stride) {
    if (n <= window) return window - n;
    const long long w = (n - window + stride - 1) / stride + 1;
    return (w - 1) * stride + window - n;
}

__device__ __forceinline__ float div32(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt32(float a) { return (float)sqrt((double)a); }

__device__ __forceinline__ short norm(int x, int mode, float s) {
    if (mode == VADX_PREPARE_NONE) return (short)x;
    float v = (float)x * s;
    if (mode == VADX_PREPARE_RMS) v = fminf(fmaxf(v, -32768.0f), 32767.0f);
    return (short)(int)v;                                      // astype(int16): toward zero
}

// numpy's pairwise sum of a[i] * a[i] over the m <= CHUNK floats at `a` (LDS), by all THREADS threads of the workgroup; the result in
// every thread.  val: LDS float [MAX_LEAVES].  Thread 8 * l + j is accumulator j of the leaf whose path from the root is the bits of l,
// most significant first (0 = the first half); a path that reaches a leaf early is owned by the l whose remaining bits are zero.
__device__ __forceinline__ float chunk_sumsq(const float *a, int m, float *val, int tid) {
    const int l = tid >> 3, j = tid & 7;
    int off = 0, size = m, depth = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
        if (size > LEAF) {
            int n2 = size / 2;
            n2 -= n2 % 8;
            if ((l >> (6 - d)) & 1) {
                off += n2;
                size -= n2;
            } else {
                size = n2;
            }
            depth = d + 1;
        }
    }
    const bool owner = (l & ((1 << (7 - depth)) - 1)) == 0;    // uniform over the eight lanes of a leaf
    float r = 0.0f;
    int i = 8;
    if (owner && size >= 8) {
        const float v0 = a[off + j];
        r = v0 * v0;
        for (; i < size - size % 8; i += 8) {
            const float v = a[off + i + j];
            r = r + v * v;                                     // two roundings: contraction is off
        }
    }
    r = r + __shfl_xor(r, 1, 64);
    r = r + __shfl_xor(r, 2, 64);
    r = r + __shfl_xor(r, 4, 64);
    if (owner && j == 0) {
        if (size < 8) {
            r = 0.0f;
            i = 0;
        }
        for (; i < size; ++i) {
            const float v = a[off + i];
            r = r + v * v;                                     // two roundings: contraction is off
        }
        val[l] = r;
    }
    __syncthreads();
#pragma unroll
    for (int d = 6; d >= 0; --d) {
        if (j == 0 && d < depth && (l & ((1 << (7 - d)) - 1)) == 0) val[l] = val[l] + val[l | (1 << (6 - d))];
        __syncthreads();
    }
    const float total = val[0];
    __syncthreads();                                           // val and a may be written again
    return total;
}

// (clip, chunk) -> Part.  PEAK needs the peaks only, RMS the sums only.
__global__ __launch_bounds__(THREADS) void stats_kernel(const short *__restrict__ src, long long src_elems, const long long *__restrict__ src_off,
                                                        const long long *__restrict__ lengths, const int *__restrict__ tile_first,
                                                        const int *__restrict__ tile_clip, int B, int mode, Part *__restrict__ parts) {
    __shared__ float xs[CHUNK];
    __shared__ float val[MAX_LEAVES];
    __shared__ int wpeak[THREADS / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int b = tile_clip[tile];
    Part out{0.0f, 0};
    bool ok = b >= 0 && b < B;                                 // uniform
    long long off = 0, c0 = 0;
    int m = 0;
    if (ok) {
        off = src_off[b];
        const long long n = lengths[b];
        c0 = (long long)(tile - tile_first[b]) * CHUNK;
        ok = !clip_bad(off, n, src_elems) && c0 >= 0 && c0 < n;
        if (ok) m = (int)(n - c0 < CHUNK ? n - c0 : CHUNK);
    }
    if (ok) {
        int peak = 0;
        for (int i = tid; i < m; i += THREADS) {
            const int x = src[off + c0 + i];
            xs[i] = (float)x;
            const int ax = x < 0 ? -x : x;
            peak = ax > peak ? ax : peak;
        }
        if (mode == VADX_PREPARE_PEAK) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int o = __shfl_xor(peak, d, 64);
                peak = o > peak ? o : peak;
            }
            if ((tid & 63) == 0) wpeak[tid >> 6] = peak;
            __syncthreads();
            if (tid == 0) {
                for (int w = 0; w < THREADS / 64; ++w) peak = wpeak[w] > peak ? wpeak[w] : peak;
                out.peak = peak;
            }
        } else {
            __syncthreads();
            out.sum = chunk_sumsq(xs, m, val, tid);
        }
    }
    if (tid == 0) parts[tile] = out;
}

// One workgroup per clip: fold, scale, tail.
__global__ __launch_bounds__(THREADS) void scale_kernel(const short *__restrict__ src, long long src_elems, const long long *__restrict__ src_off,
                                                        const long long *__restrict__ lengths, const long long *__restrict__ dst_off,
                                                        const int *__restrict__ tile_first, int tiles, long long window, long long stride, int mode,
                                                        float target_rms, const Part *__restrict__ parts, Rec *__restrict__ recs) {
    __shared__ float xs[CHUNK];
    __shared__ float val[MAX_LEAVES];
    __shared__ float s_scale;
    const int tid = threadIdx.x, b = blockIdx.x;
    const long long off = src_off[b], n = lengths[b];
    const long long gap = dst_off[b + 1] - dst_off[b] - n;
    int status = 0;
    if (clip_bad(off, n, src_elems)) {                         // uniform
        if (tid == 0) recs[b] = Rec{1.0f, 0.0f, VADX_PREPARE_ST_SRC_RANGE, 0};
        return;
    }
    if (gap != 0 && gap != pad_count(n, window, stride)) status |= VADX_PREPARE_ST_GRID;
    if (tid == 0) {
        float scale = 1.0f;
        if (mode != VADX_PREPARE_NONE) {
            int t0 = tile_first[b], t1 = tile_first[b + 1];
            t0 = t0 < 0 ? 0 : t0;
            t1 = t1 > tiles ? tiles : t1;
            float sum = 0.0f;
            int peak = 0;
            for (int t = t0; t < t1; ++t) {                    // in order: the association numpy's chunked reduction has
                const Part p = parts[t];
                sum = sum + p.sum;
                peak = p.peak > peak ? p.peak : peak;
            }
            if (mode == VADX_PREPARE_PEAK) {
                if (peak > 0) scale = div32(32767.0f, (float)peak);
            } else {
                const float r = sqrt32(div32(sum, (float)n));
                if (r > 0.0f) scale = div32(target_rms, r + 1e-7f);
            }
        }
        s_scale = scale;
    }
    __syncthreads();
    const float scale = s_scale;
    const long long pad = gap > 0 ? gap : 0;
    const long long ref_len = pad == 0 ? 0 : (n > window ? (pad < n ? pad : n) : n);
    const long long ref0 = off + n - ref_len;
    float total = 0.0f;
    for (long long c0 = 0; c0 < ref_len; c0 += CHUNK) {
        const int m = (int)(ref_len - c0 < CHUNK ? ref_len - c0 : CHUNK);
        for (int i = tid; i < m; i += THREADS) xs[i] = (float)norm(src[ref0 + c0 + i], mode, scale);
        __syncthreads();
        total = total + chunk_sumsq(xs, m, val, tid);
    }
    if (tid == 0) {
        const float rt = ref_len > 0 ? sqrt32(div32(total, (float)ref_len)) : 0.0f;
        recs[b] = Rec{scale, rt, status, 0};
    }
}

// ---- the write ----------------------------------------------------------------------------------------------------------------------
constexpr int W_THREADS = 256, W_ROWS = 4, W_TILE = W_THREADS * W_ROWS * 8;       // 16 KB of destination per workgroup

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// largest i in [lo, hi] with a[i] <= x, or lo when there is none (a is non-decreasing)
__device__ __forceinline__ long long last_le(const long long *__restrict__ a, long long lo, long long hi, long long x) {
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Work is laid out over DESTINATION tiles: a thread owns W_ROWS vectors of 8 samples, 4 KB apart.  A vector that lies inside one clip's
// samples takes its 8 source samples as 16 bytes -- the two aligned vectors around them and a byte shift when the source has another
// residue than the destination -- wherever those vectors lie inside src; every other vector (the seam between samples and fill, a clip
// boundary inside the vector, the end of the output, a source within a vector of src's end) is put together element by element.  A whole
// vector is stored as 16 aligned bytes either way.
__global__ __launch_bounds__(W_THREADS) void write_kernel(const short *__restrict__ src, long long src_elems, const long long *__restrict__ src_off,
                                                          const long long *__restrict__ lengths, const long long *__restrict__ dst_off,
                                                          const double *__restrict__ noise, long long noise_elems,
                                                          const long long *__restrict__ noise_off, int B, int mode, Rec *__restrict__ recs,
                                                          short *__restrict__ dst, long long dst_elems) {
    const long long t0 = (long long)blockIdx.x * W_TILE;
    if (t0 >= dst_elems) return;
    const long long t1 = t0 + W_TILE < dst_elems ? t0 + W_TILE : dst_elems;
    const long long b_lo = last_le(dst_off, 0, B - 1, t0), b_hi = last_le(dst_off, b_lo, B - 1, t1 - 1);
    for (int r = 0; r < W_ROWS; ++r) {
        const long long d0 = t0 + ((long long)r * W_THREADS + threadIdx.x) * 8;
        if (d0 >= t1) break;
        long long b = last_le(dst_off, b_lo, b_hi, d0);
        long long at = dst_off[b], n = lengths[b], so = src_off[b];
        bool bad = clip_bad(so, n, src_elems);
        float scale = recs[b].scale;
        short v[8];
        const long long local = d0 - at;
        bool fast = false;
        if (!bad && local >= 0 && local + 8 <= n && d0 + 8 <= dst_off[b + 1] && d0 + 8 <= t1) {
            const long long s0 = so + local, sa = s0 & ~7ll;
            const int sh = (int)(s0 - sa) * 2;                  // bytes, 0 .. 14
            if (sa + (sh ? 16 : 8) <= src_elems) {             // sa >= 0 as s0 >= 0
                const u32x4 *in = reinterpret_cast<const u32x4 *>(src + sa);
                const u32x4 lo4 = in[0];
                u32x4 hi4 = lo4;
                if (sh) hi4 = in[1];
                const unsigned int w[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
                const int q = sh >> 2, bits = (sh & 3) * 8;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned int wl = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
                    const unsigned int wh = q == 0 ? w[k + 1] : q == 1 ? w[k + 2] : q == 2 ? w[k + 3] : w[k + 4];
                    const unsigned int o = (unsigned int)((((unsigned long long)wh << 32) | wl) >> bits);
                    v[2 * k] = norm((short)(o & 0xffffu), mode, scale);
                    v[2 * k + 1] = norm((short)(o >> 16), mode, scale);
                }
                fast = true;
            }
        }
        if (!fast) {
            int noise_bad = 0;
            float rt = recs[b].tail_rms;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long long d = d0 + k;
                short y = 0;
                if (d < t1) {
                    while (b < B - 1 && d >= dst_off[b + 1]) {  // the next clip starts inside this vector
                        ++b;
                        at = dst_off[b], n = lengths[b], so = src_off[b];
                        bad = clip_bad(so, n, src_elems);
                        scale = recs[b].scale;
                        rt = recs[b].tail_rms;
                    }
                    const long long i = d - at;
                    if (bad || i < 0 || d >= dst_off[b + 1]) {
                        y = 0;                                  // a refused clip, or an element no clip owns
                    } else if (i < n) {
                        y = norm(src[so + i], mode, scale);
                    } else {
                        const long long z = noise_off[b] + (i - n);
                        if (z >= 0 && z < noise_elems) y = (short)(long long)((double)rt * noise[z]);
                        else noise_bad = 1;
                    }
                }
                v[k] = y;
            }
            if (noise_bad) atomicOr(&recs[b].status, VADX_PREPARE_ST_NOISE_RANGE);
        }
        if (d0 + 8 <= t1) {
            u32x4 o;
            o.x = (unsigned int)(unsigned short)v[0] | ((unsigned int)(unsigned short)v[1] << 16);
            o.y = (unsigned int)(unsigned short)v[2] | ((unsigned int)(unsigned short)v[3] << 16);
            o.z = (unsigned int)(unsigned short)v[4] | ((unsigned int)(unsigned short)v[5] << 16);
            o.w = (unsigned int)(unsigned short)v[6] | ((unsigned int)(unsigned short)v[7] << 16);
            *reinterpret_cast<u32x4 *>(dst + d0) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (d0 + k < t1) dst[d0 + k] = v[k];
        }
    }
}

// ---- ragged ingest: ingest.hip's closed form per output sample, over tiles of I_TILE output samples with a (tile -> clip) table ----------
constexpr int I_THREADS = 256, I_ROWS = 4, I_TILE = I_THREADS * I_ROWS;

__device__ __forceinline__ long long floordiv(long long a, long long b) {      // b > 0
    const long long qd = a / b;
    return (a % b != 0 && a < 0) ? qd - 1 : qd;
}

__global__ __launch_bounds__(I_THREADS) void ingest_ragged_kernel(const short *__restrict__ src, long long src_elems, const long long *__restrict__ src_off,
                                                                  const long long *__restrict__ frames_in, const int *__restrict__ channels,
                                                                  const int *__restrict__ in_rate, int out_rate, const long long *__restrict__ dst_off,
                                                                  const int *__restrict__ tile_first, const int *__restrict__ tile_clip, int B,
                                                                  short *__restrict__ dst, long long dst_elems, int *__restrict__ status) {
    const int b = tile_clip[blockIdx.x];
    if (b < 0 || b >= B) return;
    const long long t = (long long)blockIdx.x - tile_first[b];
    if (t < 0) return;
    const long long frames = frames_in[b], so = src_off[b], at = dst_off[b];
    const int ch = channels[b], rate = in_rate[b];
    int st = 0;
    long long I = 1, O = 1;
    const bool sane = rate > 0 && frames >= 1 && frames < (1ll << 31);
    if (sane) {
        long long g = rate, h = out_rate;
        while (h) {
            const long long q = g % h;
            g = h;
            h = q;
        }
        I = rate / g;
        O = out_rate / g;
    }
    const long long fo = sane ? (frames - 1) * O / I + 1 : 0;  // vadx_ingest_out_frames: the clip's room in dst, written as zeros when refused
    if (!sane || (ch != 1 && ch != 2) || O >= 65536) st = VADX_INGEST_ST_BAD_CLIP;        // vadx_ingest_pcm16's refusals; I < 2^31 as rate is an int
    else if (so < 0 || so > src_elems || frames * ch > src_elems - so) st = VADX_INGEST_ST_SRC_RANGE;
    const bool room = at >= 0 && at <= dst_elems && fo <= dst_elems - at;
    if (!room) st |= VADX_INGEST_ST_DST_RANGE;
    if (t == 0 && threadIdx.x == 0) status[b] = st;
    if (!room) return;
    const short *row = src + so;
    for (int r = 0; r < I_ROWS; ++r) {
        const long long e = t * I_TILE + r * I_THREADS + threadIdx.x;
        if (e >= fo) break;
        short y = 0;
        if (st == 0) {
            const long long m = (e * I + O - 1) / O + 1, d = (m - 1) * O - e * I;
            long long prev = 0, cur = 0;
            if (ch == 1) {
                if (m >= 2) prev = row[m - 2];
                cur = row[m - 1];
            } else {
                if (m >= 2) prev = ((long long)row[2 * (m - 2)] + (long long)row[2 * (m - 2) + 1]) >> 1;       // floor((L + R) / 2)
                cur = ((long long)row[2 * (m - 1)] + (long long)row[2 * (m - 1) + 1]) >> 1;
            }
            y = (short)floordiv(prev * d + cur * (O - d), O);
        }
        dst[at + e] = y;
    }
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool mode_ok(int mode) { return mode == VADX_PREPARE_NONE || mode == VADX_PREPARE_PEAK || mode == VADX_PREPARE_RMS; }
inline bool grid_ok(long long v) { return v >= 8 && v % 8 == 0; }

}  // namespace prepare
}  // namespace vadx

using namespace vadx::prepare;

extern "C" size_t vadx_prepare_workspace_bytes(int batch, int tiles) {
    if (batch < 1 || tiles < 1) return 0;
    return ws_bytes(batch, tiles);
}

// the checks the three launches share
#define PREPARE_COMMON(name)                                                                                                                         \
    VADX_REQUIRE(src && src_off && lengths && workspace, name ": NULL pointer");                                                                     \
    VADX_REQUIRE(batch >= 1, name ": batch=%d must be positive", batch);                                                                             \
    VADX_REQUIRE(tiles >= 1, name ": tiles=%d must be positive", tiles);                                                                             \
    VADX_REQUIRE(src_elems >= 0, name ": src_elems=%lld must not be negative", (long long)src_elems);                                                \
    VADX_REQUIRE(mode_ok(mode), name ": mode=%d must be VADX_PREPARE_NONE, _PEAK or _RMS", mode);                                                    \
    VADX_REQUIRE(aligned(src, 16) && aligned(src_off, 8) && aligned(lengths, 8) && aligned(workspace, 16),                                           \
                 name ": src and workspace must be 16-byte aligned, the int64 tables 8-byte");                                                       \
    VADX_REQUIRE(workspace_bytes >= ws_bytes(batch, tiles), name ": workspace_bytes=%zu is smaller than vadx_prepare_workspace_bytes(%d, %d)=%zu",   \
                 workspace_bytes, batch, tiles, ws_bytes(batch, tiles))

extern "C" int vadx_prepare_stats(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int32_t *tile_first,
                                  const int32_t *tile_clip, int batch, int tiles, int mode, void *workspace, size_t workspace_bytes, void *stream) {
    PREPARE_COMMON("vadx_prepare_stats");
    VADX_REQUIRE(tile_first && tile_clip, "vadx_prepare_stats: NULL pointer");
    VADX_REQUIRE(aligned(tile_first, 4) && aligned(tile_clip, 4), "vadx_prepare_stats: the int32 tables must be 4-byte aligned");
    Part *parts = reinterpret_cast<Part *>(static_cast<char *>(workspace) + parts_at(batch));
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, static_cast<hipStream_t>(stream), src, (long long)src_elems,
                       reinterpret_cast<const long long *>(src_off), reinterpret_cast<const long long *>(lengths), tile_first, tile_clip, batch, mode, parts);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_prepare_scale(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int64_t *dst_off,
                                  const int32_t *tile_first, int batch, int tiles, int window, int stride, int mode, float target_rms, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    PREPARE_COMMON("vadx_prepare_scale");
    VADX_REQUIRE(dst_off && tile_first, "vadx_prepare_scale: NULL pointer");
    VADX_REQUIRE(aligned(dst_off, 8) && aligned(tile_first, 4), "vadx_prepare_scale: dst_off must be 8-byte aligned, tile_first 4-byte");
    VADX_REQUIRE(grid_ok(window) && grid_ok(stride), "vadx_prepare_scale: window=%d and stride=%d must be positive multiples of 8", window, stride);
    VADX_REQUIRE(target_rms > 0.0f && target_rms <= 3.0e38f, "vadx_prepare_scale: target_rms must be positive and finite");
    char *ws = static_cast<char *>(workspace);
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)batch), dim3(THREADS), 0, static_cast<hipStream_t>(stream), src, (long long)src_elems,
                       reinterpret_cast<const long long *>(src_off), reinterpret_cast<const long long *>(lengths),
                       reinterpret_cast<const long long *>(dst_off), tile_first, tiles, (long long)window, (long long)stride, mode, target_rms,
                       reinterpret_cast<const Part *>(ws + parts_at(batch)), reinterpret_cast<Rec *>(ws));
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_prepare_write(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int64_t *dst_off,
                                  const double *noise, int64_t noise_elems, const int64_t *noise_off, int batch, int tiles, int mode, void *workspace,
                                  size_t workspace_bytes, int16_t *dst, int64_t dst_elems, void *stream) {
    PREPARE_COMMON("vadx_prepare_write");
    VADX_REQUIRE(dst_off && noise && noise_off && dst, "vadx_prepare_write: NULL pointer");
    VADX_REQUIRE(aligned(dst_off, 8) && aligned(noise, 8) && aligned(noise_off, 8) && aligned(dst, 16),
                 "vadx_prepare_write: dst must be 16-byte aligned, noise and the int64 tables 8-byte");
    VADX_REQUIRE(noise_elems >= 0 && dst_elems >= 1, "vadx_prepare_write: noise_elems=%lld must not be negative, dst_elems=%lld must be positive",
                 (long long)noise_elems, (long long)dst_elems);
    const long long wtiles = (dst_elems + W_TILE - 1) / W_TILE;
    VADX_REQUIRE(wtiles < (1ll << 31), "vadx_prepare_write: dst_elems=%lld makes %lld tiles of %d samples, must be < 2^31", (long long)dst_elems, wtiles, W_TILE);
    hipLaunchKernelGGL(write_kernel, dim3((unsigned)wtiles), dim3(W_THREADS), 0, static_cast<hipStream_t>(stream), src, (long long)src_elems,
                       reinterpret_cast<const long long *>(src_off), reinterpret_cast<const long long *>(lengths),
                       reinterpret_cast<const long long *>(dst_off), noise, (long long)noise_elems, reinterpret_cast<const long long *>(noise_off), batch,
                       mode, reinterpret_cast<Rec *>(workspace), dst, (long long)dst_elems);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_ingest_pcm16_ragged(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *frames_in, const int32_t *channels,
                                        const int32_t *in_rate, int out_rate, const int64_t *dst_off, const int32_t *tile_first,
                                        const int32_t *tile_clip, int batch, int tiles, int16_t *dst, int64_t dst_elems, int32_t *status, void *stream) {
    VADX_REQUIRE(src && src_off && frames_in && channels && in_rate && dst_off && tile_first && tile_clip && dst && status,
                 "vadx_ingest_pcm16_ragged: NULL pointer");
    VADX_REQUIRE(batch >= 1 && tiles >= 1, "vadx_ingest_pcm16_ragged: batch=%d and tiles=%d must be positive", batch, tiles);
    VADX_REQUIRE(out_rate > 0, "vadx_ingest_pcm16_ragged: out_rate=%d must be positive", out_rate);
    VADX_REQUIRE(src_elems >= 0 && dst_elems >= 0, "vadx_ingest_pcm16_ragged: src_elems=%lld and dst_elems=%lld must not be negative",
                 (long long)src_elems, (long long)dst_elems);
    VADX_REQUIRE(aligned(src, 2) && aligned(dst, 2) && aligned(src_off, 8) && aligned(frames_in, 8) && aligned(dst_off, 8) && aligned(channels, 4) &&
                     aligned(in_rate, 4) && aligned(tile_first, 4) && aligned(tile_clip, 4) && aligned(status, 4),
                 "vadx_ingest_pcm16_ragged: a table is not aligned to its element size");
    hipLaunchKernelGGL(ingest_ragged_kernel, dim3((unsigned)tiles), dim3(I_THREADS), 0, static_cast<hipStream_t>(stream), src, (long long)src_elems,
                       reinterpret_cast<const long long *>(src_off), reinterpret_cast<const long long *>(frames_in), channels, in_rate, out_rate,
                       reinterpret_cast<const long long *>(dst_off), tile_first, tile_clip, batch, dst, (long long)dst_elems, status);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
