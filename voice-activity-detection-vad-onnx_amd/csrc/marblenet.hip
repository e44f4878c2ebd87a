// marblenet.hip -- MarbleNet (NeMo Jasper, depthwise-separable 1-D convs) building blocks for gfx950.
// Reference wrapper: NVIDIA_Frame_VAD_Multilingual_MarbleNet/Export_NVIDIA_MarbleNet_VAD.py:222-275
// (encoder/decoder classes are NeMo's, un-vendored; BatchNorm is folded on the host like :58-151).
//
// sepconv_block_kernel = ONE fused launch per Jasper sub-block, tile = 1 clip x 32 output frames:
//   stage the input tile + receptive-field halo in LDS  [C_in][32*stride + (k-1)*dil]
//   -> depthwise FIR on the VALU  -> k-major [C_in][32]
//   -> pointwise 1x1 (+ folded BN bias) as an f32-MFMA GEMM, weights streamed from L2
//   -> optional residual branch (1x1 conv + folded BN of the block input) as a second GEMM
//   -> add, ReLU, coalesced store [B][C_out][T_out].
#include "common.h"
#include "layers.h"
#include "split_scheme.h"
#include "layers_split.h"

#include <math.h>
#include <type_traits>

namespace vadx {
namespace marblenet {

constexpr int THREADS = 512;
constexpr int TILE = 32, A_LD = 36;     // frames per tile, k-major row stride
constexpr int IN_LD_MAX = 100;          // largest halo tile row stride (>= 31*stride + (k-1)*dil + 1, % 8 == 4)
constexpr int MAXC = 128;
// LDS is carved per launch from the block's real shape (Cfg::in_ld, channel counts): a 64-channel k=13 block needs
// 47 KB instead of the 125 KB worst case, i.e. three workgroups per CU instead of one -- a tile is a short serial chain
// (stage -> FIR -> GEMM -> store), so with one workgroup per CU the launch was pure latency (72 rounds x ~6 us).
// A block without a residual branch whose depthwise stage has consumed the input tile writes its output over that tile
// (out_alias): the prologue (80 -> 128 channels, k = 11, stride 2) drops from 56.8 to 38.4 KB -- three workgroups per CU, not two.
static bool out_aliases_in(int cinp, int coutp, int cresp, int in_ld, bool has_dw) {
    return has_dw && !cresp && (size_t)coutp * A_LD <= (size_t)cinp * in_ld;
}
static size_t lds_floats(int cinp, int coutp, int cresp, int in_ld, bool has_dw) {
    return (size_t)cinp * in_ld + (has_dw ? (size_t)cinp * A_LD : 0) + (out_aliases_in(cinp, coutp, cresp, in_ld, has_dw) ? 0 : (size_t)coutp * A_LD) +
           (cresp ? (size_t)(cresp + coutp) * A_LD : 0);
}

struct Cfg {
    int cin, cout, k, stride, dil, pad, has_dw, cres, relu, cinp, coutp, cresp, in_ld, out_alias;
};

// A FIR thread's register window / its eight outputs as 16-byte LDS accesses (rows and window starts are multiples of four floats).
// As single floats the window reads of a wave fell on 8 of the 32 banks (every address a multiple of four floats apart: row strides
// = 4 mod 8, starts = 0 mod 8) -- four-way conflicts on every read, half of all LDS cycles of these kernels (profiles/r03_marblenet).
template <int N>
__device__ __forceinline__ void window_load(float (&win)[N], const float *row) {
#pragma unroll
    for (int v = 0; v < (N + 3) / 4; ++v) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(row + 4 * v);      // (the last one may read <= 3 floats of row padding)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * v + e < N) win[4 * v + e] = t[e];
    }
}
__device__ __forceinline__ void store8(float *dst, const float (&o)[8]) {
    *reinterpret_cast<f32x4 *>(dst) = f32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
}

// KT / DT / ST: compile-time kernel size, dilation and stride of the depthwise stage (0 = take them from `c` at run
// time: the generic fallback).  With constants the FIR is a register-window filter -- a thread owns 8 consecutive
// outputs of one channel, reads its (8-1)*stride + (k-1)*dil + 1 inputs and its k taps ONCE, and everything after
// is FMAs on registers -- and every staging load is unconditional (index clamped, value selected): a guarded load
// compiles to a branch plus a full wait, which used to serialise ~20 memory round trips per thread.
// ---- fp16 x 2 helpers of the single-block kernels (prologue, tail): 128 output channels = eight row tiles, one per wave
// split pass: k-major float32 rows src[ch][col] (ch < rows; beyond: zeros) -> B planes [kgroups][TILE][8] x 2 (item = (8 channels, frame):
// eight conflict-free reads, 24 VALU, one 16-byte store per plane)
__device__ __forceinline__ void split_rows_to_planes(const float *src, int ld, int rows, int kgroups, unsigned char *planes, float &amax) {
    const int pl = kgroups * TILE * 16;
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
    for (int it = threadIdx.x; it < kgroups * TILE; it += THREADS) {
        const int kg = it / TILE, col = it - kg * TILE;
        f32x4 lo4, hi4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo4[e] = 8 * kg + e < rows ? src[(8 * kg + e) * ld + col] : 0.f;
            hi4[e] = 8 * kg + 4 + e < rows ? src[(8 * kg + 4 + e) * ld + col] : 0.f;
        }
        u32x2 a0, a1, b0, b1;
        vadx::split2x4(lo4, a0, a1, amax);
        vadx::split2x4(hi4, b0, b1, amax);
        *reinterpret_cast<u32x4_ *>(planes + (kg * TILE + col) * 16) = u32x4_{a0[0], a0[1], b0[0], b0[1]};
        *reinterpret_cast<u32x4_ *>(planes + pl + (kg * TILE + col) * 16) = u32x4_{a1[0], a1[1], b1[0], b1[1]};
    }
}
// eight row tiles = one per wave, both column tiles of the 32-frame tile (layers_split.h's qlayer<> carries a paired-tile path that does
// not fit the 80 registers of six waves per SIMD).  OUT_PLANES as in layers_split.h.
template <bool OUT_PLANES>
__device__ __forceinline__ void gemm8_h2(const vadx::QLayerArgs &a, float &amax) {
    typedef vadx::SchemeH2 SC;
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int i = lane & 15;
    f32x4 hi[1][2], lo[1][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { hi[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f}; lo[0][mt] = hi[0][mt]; }
    const float *const w[1] = {a.W + (size_t)wave * a.nchunks * SC::NP * vadx::QFRAG};
    vadx::qgemm_group<SC, 1, 2, OUT_PLANES>(hi, lo, w, 0, a.nchunks, a.act, a.act_pl, [=](int kgrp, int mt) { return (kgrp * TILE + mt * 16 + i) * 16; }, lane);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) vadx::qlayer_store<SC, 2, OUT_PLANES>(a, wave, mt, SC::join(hi[0][mt], lo[0][mt]), lane, amax);
}

// ---------------------------------------------------------------------------------------------
// Ragged launches (include/vadx.h: vadx_marblenet_ragged).  The three kernels below take a compile-time flag RG.  RG = false is the
// rectangular launch: blockIdx.x -> (clip, tile) with a uniform tile count, every clip T frames of a [B][C][T] buffer; its trailing
// argument is an empty struct and nothing about it reaches the code.  RG = true: one workgroup per 32-frame tile of ANY clip;
// tile_clip[blockIdx.x] names the clip and tile_first[b] its first tile -- two uniform loads instead of a search of the prefix (the
// table is one int per 32 frames, 1 / 2048 of the smallest activation it describes).  Clip b's activations are [C][T_b] at float offset
// C * dst_first[b]; the prologue reads the time-major log-mel rows src_first[b] .. of clip b.  A workgroup whose entries do not
// describe a tile inside the buffers returns before its first read or write of them (ok = false).
// ---------------------------------------------------------------------------------------------
struct Ragged {
    const int *tile_first, *tile_clip, *dst_first, *src_first;      // src_first: the prologue only (elsewhere = dst_first)
    int clips, n_tiles, dst_total, src_total;
};
struct NoTables {};
// Live streams (include/vadx.h: vadx_marblenet_stream_tick), RG = 2: a workgroup's tile is a tile of the stream's VIRTUAL CLIP.  Frame
// indices are global (frame 0 = the stream's first encoder frame since its reset); the launch's input is the stream's row buffer whose
// column 0 holds global frame g0 (history columns first, then what the launch in front wrote this tick), frames outside [0, T_in) read
// as zeros exactly where the rectangular kernels mask them, and frame t of the output goes to column t + ocol of the next row buffer.
// plan[s] = what stream_open_kernel derived from the record and the tick's inputs; a stream it refused or found idle costs no tile.
constexpr int PLAN_WORDS = 16;
enum PlanWord { PL_ACTIVE = 0, PL_J = 1, PL_N = 2, PL_FINAL = 3, PL_KF = 4, PL_NOUT = 5, PL_MEL_END = 6, PL_END = 7 };      // PL_END + stage: o1 of stage 0 .. 4
struct Stream {
    const int *plan;
    int stage, off_out, off_in, in_h, out_h, in_w, out_w, tiles, streams;      // off_*: position of a stage behind the fed frame count J
};
template <int RG> struct TablesOf { typedef NoTables type; };
template <> struct TablesOf<1> { typedef Ragged type; };
template <> struct TablesOf<2> { typedef Stream type; };
struct StreamTile { bool ok; int s, t0, T_in, t_end, g0, ocol; };
__device__ __forceinline__ StreamTile stream_tile(const Stream &r) {
    StreamTile k;
    k.ok = false; k.s = 0; k.t0 = 0; k.T_in = 0; k.t_end = 0; k.g0 = 0; k.ocol = 0;
    const int s = blockIdx.x / r.tiles, tile = blockIdx.x - s * r.tiles;
    if (s >= r.streams) return k;
    const int *p = r.plan + (size_t)s * PLAN_WORDS;
    if (p[PL_ACTIVE] != 1) return k;
    const int J = p[PL_J], o0 = J - r.off_out, o1 = p[PL_END + r.stage];
    const int t0 = o0 + tile * TILE;
    if (o1 <= 0 || t0 >= o1 || t0 + TILE <= 0) return k;             // nothing of this tile is a frame of the clip
    k.ok = true; k.s = s; k.t0 = t0; k.t_end = o1;
    k.T_in = r.stage == 0 ? p[PL_MEL_END] : p[PL_END + r.stage - 1];
    k.g0 = (r.stage == 0 ? 2 * J - 1 : J - r.off_in) - r.in_h;
    k.ocol = r.out_h - o0;
    return k;
}
// column of global frame tc in a row buffer of width w whose column 0 is frame g0 (clamped: an index is never outside the buffer)
__device__ __forceinline__ int stream_col(int tc, int g0, int w) {
    const int c = tc - g0;
    return c < 0 ? 0 : (c >= w ? w - 1 : c);
}
struct RaggedTile { bool ok; int t0, T, T_src; long long first, src_row; };
template <bool STRIDE2>
__device__ __forceinline__ RaggedTile ragged_tile(const Ragged &r) {
    RaggedTile k;
    k.ok = false; k.t0 = 0; k.T = 0; k.T_src = 0; k.first = 0; k.src_row = 0;
    const int tile = blockIdx.x;
    if (tile >= r.n_tiles) return k;
    const int b = r.tile_clip[tile];
    if (b < 0 || b >= r.clips) return k;
    const int first = r.tile_first[b], next = r.tile_first[b + 1], d0 = r.dst_first[b], d1 = r.dst_first[b + 1];
    if (first < 0 || tile < first || tile >= next || d0 < 0 || d1 <= d0 || d1 > r.dst_total) return k;
    const int T = d1 - d0;
    if (next - first != (T + TILE - 1) / TILE) return k;            // the two tables disagree about this clip
    int T_src = T;
    long long src_row = d0;
    if (STRIDE2) {
        const int s0 = r.src_first[b], s1 = r.src_first[b + 1];
        if (s0 < 0 || s1 <= s0 || s1 > r.src_total || T != (s1 - s0 - 1) / 2 + 1) return k;
        T_src = s1 - s0; src_row = s0;
    }
    k.ok = true; k.t0 = (tile - first) * TILE; k.T = T; k.T_src = T_src; k.first = d0; k.src_row = src_row;
    return k;
}

// AR = 2: the prologue form only (depthwise, no residual branch, 128 filters): filter -> split pass -> gemm8_h2 (fp16 x 2 split products)
// RG (instantiated for the prologue <11, 1, 2> only): T_in / T_out come from the tables, x is time-major with row stride xs_t
template <int KT, int DT, int ST, int AR = 0, int RG = 0>
__global__ __launch_bounds__(THREADS, 2) void sepconv_block_kernel(
    Cfg c, const float *__restrict__ dw_w, const float *__restrict__ pw_w, const float *__restrict__ pw_b,
    const float *__restrict__ res_w, const float *__restrict__ res_b, const float *__restrict__ x,
    long long xs_b, long long xs_c, long long xs_t, int T_in, const float *__restrict__ xres,
    float *__restrict__ y, int T_out, int tiles, unsigned *__restrict__ range_flag, const typename TablesOf<RG>::type rg) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int IN_LD = c.in_ld;
    float *IN = lds, *D = IN + c.cinp * IN_LD, *OUT = c.out_alias ? IN : D + (c.has_dw ? c.cinp * A_LD : 0), *RIN = OUT + c.coutp * A_LD,
          *ROUT = RIN + c.cresp * A_LD;           // (out_alias implies no residual branch: RIN / ROUT are unused then)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b, t0;
    long long first = 0, src_off = 0;           // RG: the clip's first output frame in the packed buffers / first float in x
    int g0 = 0, ocol = 0, in_w = 0, out_w = 0;  // RG = 2: the stream's row buffers (see Stream)
    if constexpr (RG == 1) {
        const RaggedTile k = ragged_tile<true>(rg);
        if (!k.ok) return;
        b = 0; t0 = k.t0; T_in = k.T_src; T_out = k.T; first = k.first; src_off = k.src_row * xs_t;
    } else if constexpr (RG == 2) {
        const StreamTile k = stream_tile(rg);
        if (!k.ok) return;
        b = k.s; t0 = k.t0; T_in = k.T_in; T_out = k.t_end; g0 = k.g0; ocol = k.ocol; in_w = rg.in_w; out_w = rg.out_w;
        src_off = (long long)b * in_w * xs_t;
    } else {
        b = blockIdx.x / tiles; t0 = (blockIdx.x - b * tiles) * TILE;
    }
    const int K = KT ? KT : c.k, DIL = KT ? DT : c.dil, STR = KT ? ST : c.stride;
    const int width = (TILE - 1) * STR + (K - 1) * DIL + 1;
    const float *xb = x + (RG ? src_off : (long long)b * xs_b);
    const int tin0 = t0 * STR - c.pad;
    if (xs_c == 1) {            // time-major source (front-end output): channel fastest -> lane = channel, wave = time
        for (int j0 = 0; j0 < width; j0 += 4 * (THREADS / 64)) {
            float v[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = j0 + u * (THREADS / 64) + wave, ch = lane + 64 * h, ti = tin0 + j;
                    const int tc = ti < 0 ? 0 : (ti >= T_in ? T_in - 1 : ti), cc = ch < c.cin ? ch : c.cin - 1;
                    v[u][h] = xb[(long long)(RG == 2 ? stream_col(tc, g0, in_w) : tc) * xs_t + cc];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = j0 + u * (THREADS / 64) + wave, ch = lane + 64 * h, ti = tin0 + j;
                    if (j < width && ch < c.cinp) IN[ch * IN_LD + j] = (ch < c.cin && ti >= 0 && ti < T_in) ? v[u][h] : 0.f;
                }
        }
    } else {                    // channel-first source: time fastest -> lane = time, wave = channel
        for (int ch0 = 0; ch0 < c.cinp; ch0 += 4 * (THREADS / 64)) {
            float v[4][2];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ch = ch0 + u * (THREADS / 64) + wave, j = lane + 64 * h, ti = tin0 + j;
                    const int tc = ti < 0 ? 0 : (ti >= T_in ? T_in - 1 : ti), cc = ch < c.cin ? ch : c.cin - 1;
                    v[u][h] = xb[(long long)cc * xs_c + (long long)tc * xs_t];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int ch = ch0 + u * (THREADS / 64) + wave, j = lane + 64 * h, ti = tin0 + j;
                    if (j < width && ch < c.cinp) IN[ch * IN_LD + j] = (ch < c.cin && ti >= 0 && ti < T_in) ? v[u][h] : 0.f;
                }
        }
    }
    if (c.cres) {               // residual input tile [cres][32]: lane&31 = frame, 16 rows per pass
        const float *rb = xres + (long long)b * c.cres * T_out;
        const int m = tid & 31, tm = (t0 + m < T_out) ? t0 + m : T_out - 1;
        for (int ch0 = 0; ch0 < c.cresp; ch0 += 4 * (THREADS / 32)) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ch = ch0 + u * (THREADS / 32) + (tid >> 5), cc = ch < c.cres ? ch : c.cres - 1;
                v[u] = rb[(long long)cc * T_out + tm];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ch = ch0 + u * (THREADS / 32) + (tid >> 5);
                if (ch < c.cresp) RIN[ch * A_LD + m] = (ch < c.cres && t0 + m < T_out) ? v[u] : 0.f;
            }
        }
    }
    __syncthreads();
    const float *act = IN;
    int lda = IN_LD;
    if (c.has_dw) {
        if (KT) {               // register-window FIR: thread = (channel tid >> 2, 8 outputs starting at 8 * (tid & 3))
            constexpr int KK = KT ? KT : 1, WIN = 7 * (ST ? ST : 1) + (KK - 1) * (DT ? DT : 1) + 1;
            const int ch = tid >> 2, m0 = 8 * (tid & 3);
            if (ch < c.cinp) {
                const int cc = ch < c.cin ? ch : c.cin - 1;
                float wk[KK], win[WIN];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) wk[kk] = dw_w[cc * KK + kk];
                const float *row = IN + ch * IN_LD + m0 * (ST ? ST : 1);
                window_load(win, row);
                float o8[8];
#pragma unroll
                for (int o = 0; o < 8; ++o) {
                    float s2 = 0.f;
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) s2 = fmaf(wk[kk], win[o * (ST ? ST : 1) + kk * (DT ? DT : 1)], s2);
                    o8[o] = ch < c.cin ? s2 : 0.f;
                }
                store8(D + ch * A_LD + m0, o8);
            }
        } else {
            for (int e = tid; e < c.cinp * TILE; e += THREADS) {
                const int ch = e / TILE, m = e - ch * TILE;
                float s2 = 0.f;
                if (ch < c.cin) {
                    const float *row = IN + ch * IN_LD + m * c.stride;
                    const float *wk = dw_w + ch * c.k;
                    for (int kk = 0; kk < c.k; ++kk) s2 = fmaf(wk[kk], row[kk * c.dil], s2);
                }
                D[ch * A_LD + m] = s2;
            }
        }
        __syncthreads();
        act = D;
        lda = A_LD;
    }
    if constexpr (AR == vadx::VADX_AR_H2) {          // (launcher: has_dw, out_alias, no residual, coutp == 128; planes behind D)
        float amax = 0.f;
        const int kgroups = ((c.cinp + 31) / 32) * 4;
        unsigned char *DP = reinterpret_cast<unsigned char *>(D + c.cinp * A_LD);
        split_rows_to_planes(D, A_LD, c.cinp, kgroups, DP, amax);
        __syncthreads();
        gemm8_h2<false>(vadx::QLayerArgs{pw_w, c.coutp / 16, kgroups / 4, pw_b, c.relu ? 1 : 0, DP, kgroups * TILE * 16,
                                         reinterpret_cast<unsigned char *>(OUT), 0, A_LD, nullptr}, amax);
        vadx::range_flag_raise(range_flag, amax);
    } else {
        LayerArgs a{pw_w, c.cinp, c.coutp / 16, 1, c.cinp / 16, 0, 0, pw_b, (c.relu && !c.cres) ? 1 : 0,
                    act, lda, 0, OUT, A_LD, 0, nullptr, nullptr};
        layer<2, false>(a);
    }
    if (c.cres) {
        LayerArgs r{res_w, c.cresp, c.coutp / 16, 1, c.cresp / 16, 0, 0, res_b, 0, RIN, A_LD, 0, ROUT, A_LD, 0, nullptr, nullptr};
        layer<2, false>(r);
    }
    __syncthreads();
    float *yb = y + (RG == 2 ? (long long)b * c.cout * out_w : RG ? first * c.cout : (long long)b * c.cout * T_out);
    for (int e = tid; e < c.cout * TILE; e += THREADS) {
        const int ch = e / TILE, m = e - ch * TILE;
        if (t0 + m < T_out) {
            float v = OUT[ch * A_LD + m];
            if (c.cres) { v += ROUT[ch * A_LD + m]; if (c.relu) v = fmaxf(v, 0.f); }
            if constexpr (RG == 2) {
                const int col = t0 + m + ocol;
                if (t0 + m >= 0 && col >= 0 && col < out_w) yb[(long long)ch * out_w + col] = v;
            } else {
                yb[(long long)ch * T_out + t0 + m] = v;
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// Fused Jasper block (the three residual blocks of MarbleNet 3x2x64: two separable sub-blocks + the residual 1x1 branch of
// the block input): ONE launch per block instead of two, and the 64-channel tensor between the sub-blocks never leaves LDS.
// Tile = 1 clip x 32 output frames; sub-block 0 is evaluated on the 32 + (K - 1) frames sub-block 1's depthwise filter needs
// (48 columns = 3 m-tiles: <= 1.5 x recompute of a layer that is a quarter of the block's work), masked to zero outside
// [0, T) -- the zero padding sub-block 1 sees in the reference.
//   IN  [cin][48 + K - 1]   block input, frames t0 - (K-1) ..; the residual 1x1 (operand: columns K - 1 ..) runs FIRST, into
//   ROUT[c2][32]; then depthwise 0 overwrites IN in place (every thread reads its windows, barrier, writes) -> D0 [cin][48];
//   H1  [c1][48]            relu(pw0 D0 + b0);  depthwise 1 -> D1 [c1][32] in IN's place;  pw1 -> OUT [c2][32] in H1's place.
// Three live regions instead of four: 53 KB for the 128-channel block -- three workgroups per CU like the 64-channel blocks
// (it ran two at 80 KB; a tile is a short serial chain, so this kernel lives on workgroups per CU).
// ---------------------------------------------------------------------------------------------
struct Blk2 {
    int cin, cinp, c1, c2, in_ld, T;      // c1 = c2 = 64 here; cinp = cin padded to 16
};
constexpr int W1 = 48, H_LD = 52;

// GEMM of the fused block: 64 output channels = four row tiles for eight waves.  As whole-tile work items (layer<>) that was one
// (row tile, column tile) chain per wave opened by an L2 round trip -- the three GEMMs took 61 % of the kernel for 1.5 us of MFMA
// issue per tile.  Here wave = (row tile nt = wave & 3, K half kh = wave >> 2): every wave multiplies its half of K for ALL MT column
// tiles, its weight fragments (KB/2 <= 4 of them) are requested a phase EARLY (kgemm_pre: before the depthwise filter in front of
// the GEMM) and the two halves meet in the destination rows: the kh = 1 wave stores its partial tile, the kh = 0 wave adds its own
// and the bias behind a barrier -- a fixed order, so the result is reproducible.
struct KPre { f32x4 w[4]; };

__device__ __forceinline__ KPre kgemm_pre(const float *__restrict__ W, int kdim) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int nt = wave & 3, kh = wave >> 2, nb = kdim >> 5;      // 16-k blocks per half: 2 (K = 64) or 4 (K = 128)
    const float *base = vadx::frag_ptr(W, kdim, nt, 16 * kh * nb, lane);
    KPre p;
#pragma unroll
    for (int u = 0; u < 4; ++u) p.w[u] = vadx::ldg4(base + vadx::FRAG * (u < nb ? u : nb - 1));      // unconditional, clamped
    return p;
}

template <int MT>
__device__ __forceinline__ void kgemm(const KPre &p, int kdim, const float *act, int lda, int acol0, float *dst, int ldd,
                                      const float *__restrict__ bias, bool relu) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int q = lane >> 4, i = lane & 15, nt = wave & 3, kh = wave >> 2, nb = kdim >> 5;
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *ap = act + (16 * kh * nb + 4 * q) * lda + acol0 + i;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < nb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = vadx::mfma16(ap[(16 * u + j) * lda + mt * 16], p.w[u][j], acc[mt]);
            }
        }
    }
    float *dp = dst + (nt * 16 + i) * ldd + 4 * q;
    if (kh == 1)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4 *>(dp + mt * 16) = acc[mt];
    __syncthreads();
    if (kh == 0) {
        const float b = bias[nt * 16 + i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x4 v = *reinterpret_cast<const f32x4 *>(dp + mt * 16);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = (v[r] + acc[mt][r]) + b; if (relu) v[r] = fmaxf(v[r], 0.f); }
            *reinterpret_cast<f32x4 *>(dp + mt * 16) = v;
        }
    }
}

// The same GEMM on fp16 x 2 split products (split2.h): three v_mfma_f32_16x16x32_f16 per 32 channels and column tile instead of eight
// v_mfma_f32_16x16x4_f32 -- on this kernel the f32 MFMAs shared the vector datapath with the depthwise filters (with one MFMA in eight
// the three block launches ran 4.14 -> 2.72 ms).  The depthwise filters leave k-major float32 rows (a thread owns eight consecutive
// frames of ONE channel), so there are no planes to read: a wave splits its own operand -- lane (q, i) reads the eight channels
// 16 (e >> 2) + 4 q + (e & 3), e = 0..7, of frame i (the f32 kernel's conflict-free row pattern: quarters 4 rows = 16 banks apart),
// splits them (3 VALU per value) and uses them as the A operand; the weights are the B operand, their fragments packed on the host in
// the same k-slot order (vadx_frag_h2_host).  The four row-tile waves of a K half split the same values (4 x redundant, 28 VALU per
// fragment): still a third of the datapath time of the f32 MFMAs they replace.
struct KPreH { f16x8 w[2][2]; };         // [chunk of this wave's K half][plane]

__device__ __forceinline__ KPreH kgemm_pre_h(const float *__restrict__ W, int kdim) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int nt = wave & 3, kh = wave >> 2, nc = kdim >> 6;      // 32-k chunks per half: 1 (K = 64) or 2 (K = 128)
    const float *base = W + (size_t)((nt * 2 * nc + kh * nc) * 2) * vadx::HFRAG;
    KPreH p;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) p.w[u][pl] = vadx::ldh(base + (size_t)((u < nc ? u : nc - 1) * 2 + pl) * vadx::HFRAG, lane);      // unconditional, clamped
    return p;
}

template <int MT>
__device__ __forceinline__ void kgemm_h(const KPreH &p, int kdim, const float *act, int lda, int acol0, float *dst, int ldd,
                                        const float *__restrict__ bias, bool relu, float &amax) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int q = lane >> 4, i = lane & 15, nt = wave & 3, kh = wave >> 2, nc = kdim >> 6;
    f32x4 hi[MT], mid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { hi[mt] = f32x4{0.f, 0.f, 0.f, 0.f}; mid[mt] = hi[mt]; }
    const float *ap = act + (32 * kh * nc + 4 * q) * lda + acol0 + i;
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (u < nc) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 lo4, hi4;
#pragma unroll
                for (int j = 0; j < 4; ++j) { lo4[j] = ap[(32 * u + j) * lda + mt * 16]; hi4[j] = ap[(32 * u + 16 + j) * lda + mt * 16]; }
                u32x2 a0, a1, b0, b1;
                vadx::split2x4(lo4, a0, a1, amax);
                vadx::split2x4(hi4, b0, b1, amax);
                const f16x8 x0 = __builtin_bit_cast(f16x8, u32x4_{a0[0], a0[1], b0[0], b0[1]});
                const f16x8 x1 = __builtin_bit_cast(f16x8, u32x4_{a1[0], a1[1], b1[0], b1[1]});
                mid[mt] = vadx::mfma_f16(x1, p.w[u][0], mid[mt]);
                mid[mt] = vadx::mfma_f16(x0, p.w[u][1], mid[mt]);
                hi[mt] = vadx::mfma_f16(x0, p.w[u][0], hi[mt]);
            }
        }
    }
    float *dp = dst + (nt * 16 + i) * ldd + 4 * q;
    if (kh == 1)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4 *>(dp + mt * 16) = vadx::join2(hi[mt], mid[mt]);
    __syncthreads();
    if (kh == 0) {
        const float b = bias[nt * 16 + i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x4 v = *reinterpret_cast<const f32x4 *>(dp + mt * 16);
            const f32x4 own = vadx::join2(hi[mt], mid[mt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = (v[r] + own[r]) + b; if (relu) v[r] = fmaxf(v[r], 0.f); }
            *reinterpret_cast<f32x4 *>(dp + mt * 16) = v;
        }
    }
}

// ---- AR = 3: the plane form of the fp16 x 2 GEMMs, for the 64-channel blocks (their 40 KB leave room for 12 KB of planes at three
// workgroups per CU; the 128-channel block sits at 53.2 KB and keeps kgemm_h).  The operand is split ONCE by a transposing pass (item = (8
// channels, column): eight conflict-free reads, 24 VALU, one 16-byte store per plane) instead of by each of the four row-tile waves, and
// with no split to share a wave takes a whole K: wave = (row tile, column-tile parity), no partial sums, no barrier inside the GEMM -- the
// pass's barrier takes its place.  Weights: vadx_frag_h2_host, VADX_H2_K_PLAIN.
__device__ __forceinline__ void split_rows_to_planes_n(const float *src, int ld, int col0, int kgroups, int ncol, unsigned char *planes, float &amax) {
    const int pl = kgroups * ncol * 16;
    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
    for (int it = threadIdx.x; it < kgroups * ncol; it += THREADS) {
        const int kg = it / ncol, col = it - kg * ncol;
        f32x4 lo4, hi4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo4[e] = src[(8 * kg + e) * ld + col0 + col]; hi4[e] = src[(8 * kg + 4 + e) * ld + col0 + col]; }
        u32x2 a0, a1, b0, b1;
        vadx::split2x4(lo4, a0, a1, amax);
        vadx::split2x4(hi4, b0, b1, amax);
        *reinterpret_cast<u32x4_ *>(planes + (kg * ncol + col) * 16) = u32x4_{a0[0], a0[1], b0[0], b0[1]};
        *reinterpret_cast<u32x4_ *>(planes + pl + (kg * ncol + col) * 16) = u32x4_{a1[0], a1[1], b1[0], b1[1]};
    }
}
__device__ __forceinline__ KPreH kgemm_pre_p(const float *__restrict__ W) {      // K = 64: this wave's row tile, both chunks, both planes
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const float *base = W + (size_t)((wave & 3) * 2 * 2) * vadx::HFRAG;
    KPreH p;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) p.w[u][pl] = vadx::ldh(base + (size_t)(u * 2 + pl) * vadx::HFRAG, lane);
    return p;
}
template <int MT>
__device__ __forceinline__ void pgemm(const KPreH &p, const unsigned char *planes, int ncol, float *dst, int ldd, const float *__restrict__ bias, bool relu) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    asm volatile("" : "+v"(lane), "+v"(wave));
    const int q = lane >> 4, i = lane & 15, nt = wave & 3, mh = wave >> 2, plb = 8 * ncol * 16;
    const float b = bias[nt * 16 + i];
#pragma unroll
    for (int mt0 = 0; mt0 < MT; mt0 += 2) {
        const int mt = mt0 + mh;
        if (mt < MT) {
            f32x4 hi = {0.f, 0.f, 0.f, 0.f}, mid = hi;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const unsigned char *ap = planes + ((4 * u + q) * ncol + mt * 16 + i) * 16;
                const f16x8 a0 = *reinterpret_cast<const f16x8 *>(ap), a1 = *reinterpret_cast<const f16x8 *>(ap + plb);
                mid = vadx::mfma_f16(a1, p.w[u][0], mid);
                hi = vadx::mfma_f16(a0, p.w[u][0], hi);
                mid = vadx::mfma_f16(a0, p.w[u][1], mid);
            }
            f32x4 v = vadx::join2(hi, mid);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] += b; if (relu) v[r] = fmaxf(v[r], 0.f); }
            *reinterpret_cast<f32x4 *>(dst + (nt * 16 + i) * ldd + mt * 16 + 4 * q) = v;
        }
    }
}
// AR: 0 = float32 MFMAs (kgemm), 2 = fp16 x 2 split products (kgemm_h); one body for both
template <int AR> struct KPreOf { typedef KPre type; };
template <> struct KPreOf<vadx::VADX_AR_H2> { typedef KPreH type; };
template <> struct KPreOf<3> { typedef KPreH type; };          // 3 = fp16 x 2, plane form (pgemm)
template <int AR>
__device__ __forceinline__ typename KPreOf<AR>::type kpre(const float *__restrict__ W, int kdim) {
    if constexpr (AR == 3) return kgemm_pre_p(W);
    else if constexpr (AR == vadx::VADX_AR_H2) return kgemm_pre_h(W, kdim);
    else return kgemm_pre(W, kdim);
}
template <int AR, int MT>
__device__ __forceinline__ void kmul(const typename KPreOf<AR>::type &p, int kdim, const float *act, int lda, int acol0, float *dst, int ldd,
                                     const float *__restrict__ bias, bool relu, float &amax) {
    if constexpr (AR == vadx::VADX_AR_H2) kgemm_h<MT>(p, kdim, act, lda, acol0, dst, ldd, bias, relu, amax);
    else kgemm<MT>(p, kdim, act, lda, acol0, dst, ldd, bias, relu);
}

template <int K, int AR, int RG = 0>
__global__ __launch_bounds__(THREADS, 6) void jasper_block2_kernel(
    Blk2 c, const float *__restrict__ dw0, const float *__restrict__ pw0, const float *__restrict__ b0,
    const float *__restrict__ dw1, const float *__restrict__ pw1, const float *__restrict__ b1,
    const float *__restrict__ rw, const float *__restrict__ rb, const float *__restrict__ x, float *__restrict__ y, int tiles,
    unsigned *__restrict__ range_flag, const typename TablesOf<RG>::type rg) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int b, t0;
    long long first = 0;                        // RG: the clip's first frame in the packed buffers; c.T becomes the clip's frame count
    int g0 = 0, ocol = 0, in_w = 0, out_w = 0, t_end = 0;      // RG = 2: the stream's row buffers (see Stream); c.T becomes the input's end
    if constexpr (RG == 1) {
        const RaggedTile k = ragged_tile<false>(rg);
        if (!k.ok) return;
        b = 0; t0 = k.t0; c.T = k.T; first = k.first;
    } else if constexpr (RG == 2) {
        const StreamTile k = stream_tile(rg);
        if (!k.ok) return;
        b = k.s; t0 = k.t0; c.T = k.T_in; t_end = k.t_end; g0 = k.g0; ocol = k.ocol; in_w = rg.in_w; out_w = rg.out_w;
    } else {
        b = blockIdx.x / tiles; t0 = (blockIdx.x - b * tiles) * TILE;
    }
    typedef typename KPreOf<AR>::type KP;
    float amax = 0.f;
    constexpr int PAD = (K - 1) / 2, WIN0 = W1 + K - 1;
    const int IN_LD = c.in_ld;
    float *IN = lds, *H1 = IN + c.cinp * IN_LD, *ROUT = H1 + c.c1 * H_LD;
    float *D0 = IN, *D1 = IN, *OUT = H1;
    unsigned char *PL = reinterpret_cast<unsigned char *>(ROUT + c.c2 * A_LD);      // AR = 3: operand planes [8 k-groups][<= 48 columns][8] x 2
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xb = x + (RG == 2 ? (long long)b * c.cin * in_w : RG ? first * c.cin : (long long)b * c.cin * c.T);
    const int tin0 = t0 - 2 * PAD;
    const KP wres = kpre<AR>(rw, c.cinp);                    // in flight while the input tile is staged
    // ---- stage the block input (channel-first source: lane = time, wave = channel), unconditional clamped loads
    for (int ch0 = 0; ch0 < c.cinp; ch0 += 8 * (THREADS / 64)) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ch = ch0 + u * (THREADS / 64) + wave, ti = tin0 + lane;
            const int tc = ti < 0 ? 0 : (ti >= c.T ? c.T - 1 : ti), cc = ch < c.cin ? ch : c.cin - 1;
            v[u] = RG == 2 ? xb[(long long)cc * in_w + stream_col(tc, g0, in_w)] : xb[(long long)cc * c.T + tc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ch = ch0 + u * (THREADS / 64) + wave, ti = tin0 + lane;
            if (lane < WIN0 && ch < c.cinp) IN[ch * IN_LD + lane] = (ch < c.cin && ti >= 0 && ti < c.T) ? v[u] : 0.f;
        }
    }
    __syncthreads();
    // pointwise 0's weights: in flight through the residual GEMM and depthwise 0 -- except at K = 17, whose 24-value window + 17 taps +
    // 16 prefetched weight registers no longer fit the 80 VGPRs of six waves per SIMD (20 B of scratch per lane doubled the kernel's
    // HBM writes): there they are requested behind the filter
    KP wpw0;
    if (K < 17) wpw0 = kpre<AR>(pw0, c.cinp);
    // residual 1x1 of the block input (frames t0 .. t0 + 31 sit at column 2 PAD), before the input is overwritten
    if constexpr (AR == 3) {
        split_rows_to_planes_n(IN, IN_LD, 2 * PAD, 8, TILE, PL, amax);
        __syncthreads();            // (the residual GEMM reads the planes only: depthwise 0 may overwrite IN behind this barrier)
        pgemm<2>(wres, PL, TILE, ROUT, A_LD, rb, false);
    } else {
        kmul<AR, 2>(wres, c.cinp, IN, IN_LD, 2 * PAD, ROUT, A_LD, rb, false, amax);
        __syncthreads();            // every residual operand is read: depthwise 0 may overwrite IN
    }
    // ---- depthwise 0 IN PLACE: register-window FIR, item = (channel, 8 outputs).  The six items of a channel are six neighbouring
    // lanes of ONE wave: a wave's window reads all precede its writes in program order (the FMAs in between depend on them), and
    // no two waves share a channel, so the overwrite needs no further barrier.
    for (int ch0 = 0; ch0 < c.cinp; ch0 += 10 * (THREADS / 64)) {
        const int ch = ch0 + wave * 10 + lane / 6, m0 = 8 * (lane % 6);
        if (lane < 60 && ch < c.cinp) {
            const int cc = ch < c.cin ? ch : c.cin - 1;
            float wk[K], win[7 + K];
#pragma unroll
            for (int kk = 0; kk < K; ++kk) wk[kk] = dw0[cc * K + kk];
            float *row = IN + ch * IN_LD + m0;
            window_load(win, row);
            float o8[8];
#pragma unroll
            for (int o = 0; o < 8; ++o) {
                float s2 = 0.f;
#pragma unroll
                for (int kk = 0; kk < K; ++kk) s2 = fmaf(wk[kk], win[o + kk], s2);
                o8[o] = ch < c.cin ? s2 : 0.f;
            }
            __builtin_amdgcn_wave_barrier();                // keep every lane's reads above every lane's writes in the schedule
            store8(row, o8);
        }
    }
    if (K >= 17) wpw0 = kpre<AR>(pw0, c.cinp);
    __syncthreads();
    KP wpw1;                                                 // pointwise 1's weights: in flight through pointwise 0 and depthwise 1
    if (K < 17) wpw1 = kpre<AR>(pw1, c.c1);
    // pointwise 0 + folded BN + ReLU on 48 columns
    if constexpr (AR == 3) {
        split_rows_to_planes_n(D0, IN_LD, 0, 8, W1, PL, amax);       // (every wave is past the residual GEMM: the barrier behind depthwise 0)
        __syncthreads();
        pgemm<3>(wpw0, PL, W1, H1, H_LD, b0, true);
    } else {
        kmul<AR, 3>(wpw0, c.cinp, D0, IN_LD, 0, H1, H_LD, b0, true, amax);
    }
    __syncthreads();
    // ---- depthwise 1 on H1 (column j = frame t0 - PAD + j; frames outside the clip are the conv's zero padding)
    for (int it = tid; it < c.c1 * (TILE / 8); it += THREADS) {
        const int ch = it / (TILE / 8), m0 = 8 * (it - ch * (TILE / 8));
        float wk[K], win[7 + K];
#pragma unroll
        for (int kk = 0; kk < K; ++kk) wk[kk] = dw1[ch * K + kk];
        const float *row = H1 + ch * H_LD + m0;
        window_load(win, row);
#pragma unroll
        for (int u = 0; u < 7 + K; ++u) {
            const int fr = t0 - PAD + m0 + u;
            win[u] = (fr >= 0 && fr < c.T) ? win[u] : 0.f;
        }
        float o8[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float s2 = 0.f;
#pragma unroll
            for (int kk = 0; kk < K; ++kk) s2 = fmaf(wk[kk], win[o + kk], s2);
            o8[o] = s2;
        }
        store8(D1 + ch * A_LD + m0, o8);                                // D1 sits in IN's region (D0 is dead since the barrier above)
    }
    if (K >= 17) wpw1 = kpre<AR>(pw1, c.c1);
    __syncthreads();                // every H1 read is done: OUT may overwrite it
    if constexpr (AR == 3) {
        split_rows_to_planes_n(D1, A_LD, 0, 8, TILE, PL, amax);
        __syncthreads();
        pgemm<2>(wpw1, PL, TILE, OUT, A_LD, b1, false);
    } else {
        kmul<AR, 2>(wpw1, c.c1, D1, A_LD, 0, OUT, A_LD, b1, false, amax);
    }
    __syncthreads();
    float *yb = y + (RG == 2 ? (long long)b * c.c2 * out_w : RG ? first * c.c2 : (long long)b * c.c2 * c.T);
    for (int e = tid; e < c.c2 * TILE; e += THREADS) {
        const int ch = e / TILE, m = e - ch * TILE;
        if constexpr (RG == 2) {
            const int col = t0 + m + ocol;
            if (t0 + m >= 0 && t0 + m < t_end && col >= 0 && col < out_w) yb[(long long)ch * out_w + col] = fmaxf(OUT[ch * A_LD + m] + ROUT[ch * A_LD + m], 0.f);
        } else {
            if (t0 + m < c.T) yb[(long long)ch * c.T + t0 + m] = fmaxf(OUT[ch * A_LD + m] + ROUT[ch * A_LD + m], 0.f);
        }
    }
    if (AR >= vadx::VADX_AR_H2) vadx::range_flag_raise(range_flag, amax);          // an operand left the fp16 range: the host recomputes this batch on float32
}

// ---------------------------------------------------------------------------------------------
// Tail of the encoder + decoder in one launch: block 5 (depthwise k = 29, dilation 2, 64 -> 128, ReLU), block 6 (plain 1x1,
// 128 -> 128, ReLU), Linear(128 -> 2), softmax: the two 128-channel tensors and the encoder output never reach HBM -- only
// the two scores per frame leave the kernel (wrapper :265-274).
//   IN [64][32 + 56] -> D [64][32] -> H [128][32] -> OUT [128][32] (in IN's place) -> scores
// ---------------------------------------------------------------------------------------------
struct Tail { int cin, cmid, k, dil, in_ld, T; };

// AR = 2 (fp16 x 2 split products, layers_split.h: qlayer): the two 1x1 convs are GEMM -> GEMM, so only the filter's k-major float32 output
// needs a transposing split pass (item = (8 channels, frame): eight conflict-free reads, 24 VALU, one 16-byte store per plane into the dead
// input tile's place); block 5's conv takes the weights as its A operand and stores its ReLU output straight into block 6's B planes
// [channel / 8][frame][8] (8-byte stores, in H's place), block 6 takes the activations as A and stores float32 rows for the decoder.
template <int AR, int RG = 0>
__global__ __launch_bounds__(THREADS, 6) void marblenet_tail_kernel(
    Tail c, const float *__restrict__ dw, const float *__restrict__ pw, const float *__restrict__ pb,
    const float *__restrict__ w6, const float *__restrict__ b6, const float *__restrict__ dec_w, const float *__restrict__ dec_b,
    const float *__restrict__ x, float *__restrict__ s0, float *__restrict__ s1, int tiles, unsigned *__restrict__ range_flag,
    const typename TablesOf<RG>::type rg) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int b, t0;
    long long first = 0;                        // RG: the clip's first frame in the packed buffers; c.T becomes the clip's frame count
    int g0 = 0, ocol = 0, in_w = 0, out_w = 0, t_end = 0;      // RG = 2: the stream's row buffer (see Stream); out_w = the score rows' cap
    if constexpr (RG == 1) {
        const RaggedTile k = ragged_tile<false>(rg);
        if (!k.ok) return;
        b = 0; t0 = k.t0; c.T = k.T; first = k.first;
    } else if constexpr (RG == 2) {
        const StreamTile k = stream_tile(rg);
        if (!k.ok) return;
        b = k.s; t0 = k.t0; c.T = k.T_in; t_end = k.t_end; g0 = k.g0; in_w = rg.in_w; out_w = rg.out_w;
        ocol = k.ocol < 0 ? k.ocol : 0;         // (out_h = 0: ocol = -o0) a score row starts at the stream's first REAL frame this tick, max(o0, 0)
    } else {
        b = blockIdx.x / tiles; t0 = (blockIdx.x - b * tiles) * TILE;
    }
    constexpr int K = 29, DIL = 2, PAD = 28, WIN0 = TILE + 2 * PAD;
    const int IN_LD = c.in_ld;
    float amax = 0.f;
    float *IN = lds, *D = IN + c.cin * IN_LD, *H = D + c.cin * A_LD, *OUT = IN;
    float *red = D;                                 // [16 parts][32 frames][2] once D is dead
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xb = x + (RG == 2 ? (long long)b * c.cin * in_w : RG ? first * c.cin : (long long)b * c.cin * c.T);
    const int tin0 = t0 - PAD;
    for (int ch0 = 0; ch0 < c.cin; ch0 += 4 * (THREADS / 64)) {
        float v[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = ch0 + u * (THREADS / 64) + wave, ti = tin0 + lane + 64 * h;
                const int tc = ti < 0 ? 0 : (ti >= c.T ? c.T - 1 : ti), cc = ch < c.cin ? ch : c.cin - 1;
                v[u][h] = RG == 2 ? xb[(long long)cc * in_w + stream_col(tc, g0, in_w)] : xb[(long long)cc * c.T + tc];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = ch0 + u * (THREADS / 64) + wave, j = lane + 64 * h, ti = tin0 + j;
                if (j < WIN0 && ch < c.cin) IN[ch * IN_LD + j] = (ti >= 0 && ti < c.T) ? v[u][h] : 0.f;
            }
    }
    __syncthreads();
    for (int it = tid; it < c.cin * (TILE / 8); it += THREADS) {       // register-window FIR, dilation 2
        const int ch = it / (TILE / 8), m0 = 8 * (it - ch * (TILE / 8));
        float wk[K], win[7 + (K - 1) * DIL + 1];
#pragma unroll
        for (int kk = 0; kk < K; ++kk) wk[kk] = dw[ch * K + kk];
        const float *row = IN + ch * IN_LD + m0;
        window_load(win, row);
        float o8[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            float s2 = 0.f;
#pragma unroll
            for (int kk = 0; kk < K; ++kk) s2 = fmaf(wk[kk], win[o + kk * DIL], s2);
            o8[o] = s2;
        }
        store8(D + ch * A_LD + m0, o8);
    }
    __syncthreads();
    if constexpr (AR == vadx::VADX_AR_H2) {
        unsigned char *DP = reinterpret_cast<unsigned char *>(IN), *HP = reinterpret_cast<unsigned char *>(H);      // the input tile is dead
        const int dp_pl = (c.cin / 8) * TILE * 16, hp_pl = (c.cmid / 8) * TILE * 16;                                  // bytes per plane
        split_rows_to_planes(D, A_LD, c.cin, c.cin / 8, DP, amax);
        __syncthreads();
        gemm8_h2<true>(vadx::QLayerArgs{pw, c.cmid / 16, c.cin / 32, pb, 1, DP, dp_pl, HP, hp_pl, TILE, nullptr}, amax);
        __syncthreads();            // D and its planes are dead
        gemm8_h2<false>(vadx::QLayerArgs{w6, c.cmid / 16, c.cmid / 32, b6, 1, HP, hp_pl, reinterpret_cast<unsigned char *>(OUT), 0, A_LD, nullptr}, amax);
    } else {
        {
            LayerArgs a{pw, c.cin, c.cmid / 16, 1, c.cin / 16, 0, 0, pb, 1, D, A_LD, 0, H, A_LD, 0, nullptr, nullptr};
            layer<2, false>(a);
        }
        __syncthreads();            // IN and D are dead
        {
            LayerArgs a{w6, c.cmid, c.cmid / 16, 1, c.cmid / 16, 0, 0, b6, 1, H, A_LD, 0, OUT, A_LD, 0, nullptr, nullptr};
            layer<2, false>(a);
        }
    }
    __syncthreads();
    {   // decoder: thread = (part of 8 channels, frame); partial logits meet in LDS and are summed in part order
        const int m = tid & 31, part = tid >> 5;
        float z0 = 0.f, z1 = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int ch = part * 8 + u;
            const float v = OUT[ch * A_LD + m];
            z0 = fmaf(dec_w[ch], v, z0);
            z1 = fmaf(dec_w[c.cmid + ch], v, z1);
        }
        red[(part * TILE + m) * 2] = z0;
        red[(part * TILE + m) * 2 + 1] = z1;
    }
    __syncthreads();
    if constexpr (RG == 2) {                        // the frame's place in the stream's score row
        const int col = t0 + tid + ocol;
        if (tid < TILE && t0 + tid >= 0 && t0 + tid < t_end && col >= 0 && col < out_w) {
            float z0 = dec_b[0], z1 = dec_b[1];
#pragma unroll
            for (int part = 0; part < THREADS / 32; ++part) { z0 += red[(part * TILE + tid) * 2]; z1 += red[(part * TILE + tid) * 2 + 1]; }
            const float mx = fmaxf(z0, z1), e0 = expf(z0 - mx), e1 = expf(z1 - mx), inv = 1.0f / (e0 + e1);
            s0[(long long)b * out_w + col] = e0 * inv;
            s1[(long long)b * out_w + col] = e1 * inv;
        }
    } else if (tid < TILE && t0 + tid < c.T) {
        float z0 = dec_b[0], z1 = dec_b[1];
#pragma unroll
        for (int part = 0; part < THREADS / 32; ++part) { z0 += red[(part * TILE + tid) * 2]; z1 += red[(part * TILE + tid) * 2 + 1]; }
        const float mx = fmaxf(z0, z1), e0 = expf(z0 - mx), e1 = expf(z1 - mx), inv = 1.0f / (e0 + e1);
        s0[(RG ? first : (long long)b * c.T) + t0 + tid] = e0 * inv;
        s1[(RG ? first : (long long)b * c.T) + t0 + tid] = e1 * inv;
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(range_flag, amax);
}

// decoder Linear(C -> 2) + softmax (wrapper :270-274): one thread per (clip, frame)
__global__ void frame_classifier_kernel(const float *__restrict__ enc, const float *__restrict__ w, const float *__restrict__ bias,
                                        int B, int C, int T, float *__restrict__ s0, float *__restrict__ s1) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * T) return;
    const int b = (int)(idx / T), t = (int)(idx - (long long)b * T);
    const float *e = enc + (long long)b * C * T + t;
    float z0 = 0.f, z1 = 0.f;
    for (int c2 = 0; c2 < C; ++c2) {
        const float v = e[(long long)c2 * T];
        z0 = fmaf(w[c2], v, z0);
        z1 = fmaf(w[C + c2], v, z1);
    }
    z0 += bias[0]; z1 += bias[1];
    const float m = fmaxf(z0, z1), e0 = expf(z0 - m), e1 = expf(z1 - m), inv = 1.0f / (e0 + e1);
    s0[idx] = e0 * inv;
    s1[idx] = e1 * inv;
}

// ---------------------------------------------------------------------------------------------
// Live streams: the device record and the two kernels around a tick's launches (include/vadx.h: vadx_marblenet_stream_tick).
// A stream that has been fed 320 J samples stands, stage by stage, a fixed distance behind J: log-mel frames 0 .. 2J - 2 are complete,
// the prologue has written encoder frames < J - 3, blocks 2 / 3 / 4 frames < J - 15 / J - 29 / J - 45, and score frames < J - 73 are out
// (negative = none yet).  The record keeps, per launch boundary, the frames in front of that position the next launch's filter reaches
// back to; an index below 0 is the layers' zero padding, which is what an all-zero record holds: zero bytes = a fresh stream.
//   words (4 bytes)   0 ..   800  log-mel history   [10 frames][80]  (time-major)      frames 2J - 11 .. 2J - 2
//                   800 ..  3872  prologue output   [128][24]                           frames  J - 27 ..  J - 4
//                  3872 ..  5664  block 2 output    [64][28]                            frames  J - 43 ..  J - 16
//                  5664 ..  7712  block 3 output    [64][32]                            frames  J - 61 ..  J - 30
//                  7712 .. 11296  block 4 output    [64][56]                            frames  J - 101 .. J - 46
//                 11296 .. 11508  audio carry       417 int16 (the last 416 samples + the pre-emphasis tap in front), zero-padded
//                 11508, 11509    samples fed since the reset (int64);   11510, 11511   score frames emitted since the reset (int64)
// ---------------------------------------------------------------------------------------------
constexpr int R_MEL = 0, R_P = 800, R_B2 = 3872, R_B3 = 5664, R_B4 = 7712, R_PCM = 11296, R_FED = 11508, R_EMIT = 11510, R_WORDS = 11512;
constexpr int CARRY = 417, HOP2 = 320, LOOKAHEAD = 73, K_MAX = 256, J_CLAMP = 1 << 24;
constexpr int ST_OFF[5] = {3, 15, 29, 45, 73};       // position of the prologue, blocks 2 - 4 and the scores behind J
// INVARIANT the row buffers rest on: they are scratch that nobody initialises, so every column a launch may read must have been written
// this tick -- by stream_open_kernel (the history columns) or by the launch in front (the new ones).  That holds because the history
// width of a boundary EQUALS the reach of the stage behind it: 2 * pad of the prologue (k 11: 10 log-mel frames) and of the tail (k 29,
// dilation 2: 56), 4 * pad of a fused block (two sub-blocks of k 13 / 15 / 17: 24 / 28 / 32), and because ST_OFF[i] - ST_OFF[i - 1] is
// half of that, so a tile's first input column is column 0.  Columns below frame 0 may hold anything (an early-out tile wrote nothing):
// every load masks them by index and stream_close_kernel writes zeros for them.  Change a kernel size and all three tables change with it;
// a width short of the reach reads unwritten memory (possibly NaN, which raises the range flag), a longer one carries dead columns.
constexpr int ST_HIST[5] = {10, 24, 28, 32, 56};     // history frames IN FRONT of stage i (its input's): log-mel, prologue, blocks 2 - 4
constexpr int ST_EXTRA[5] = {4, 16, 30, 46, 73};     // frames beyond k a stage can write on a stream's final tick
constexpr int ST_CH[4] = {128, 64, 64, 64};          // channels of the prologue's and the blocks' outputs
constexpr int ST_REC[5] = {R_MEL, R_P, R_B2, R_B3, R_B4};

// the workspace of one tick: plan, the front-end's two tables, the sample rows, then one row buffer per launch boundary
struct StreamWs {
    int *plan, *fe_len, *fe_frames;
    int16_t *pcm;
    float *rows[5];          // log-mel [S][w[0]][80]; prologue [S][128][w[1]]; blocks 2 - 4 [S][64][w[2 .. 4]]
    int pcm_w, w[5];
};
static size_t stream_ws_layout(int streams, int k, StreamWs *ws, char *base) {
    size_t at = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + at : nullptr; at += (bytes + 255) & ~(size_t)255; return p; };
    ws->pcm_w = (CARRY + HOP2 * k + 7) & ~7;
    ws->w[0] = ST_HIST[0] + 2 * k + 2;
    for (int i = 1; i < 5; ++i) ws->w[i] = ST_HIST[i] + k + ST_EXTRA[i - 1];
    ws->plan = reinterpret_cast<int *>(take((size_t)streams * PLAN_WORDS * 4));
    ws->fe_len = reinterpret_cast<int *>(take((size_t)streams * 4));
    ws->fe_frames = reinterpret_cast<int *>(take((size_t)streams * 4));
    ws->pcm = reinterpret_cast<int16_t *>(take((size_t)streams * ws->pcm_w * 2));
    ws->rows[0] = reinterpret_cast<float *>(take((size_t)streams * ws->w[0] * 80 * 4));
    for (int i = 1; i < 5; ++i) ws->rows[i] = reinterpret_cast<float *>(take((size_t)streams * ST_CH[i - 1] * ws->w[i] * 4));
    return at;
}

struct StreamIO {
    const int16_t *samples;
    long long sample_stride;
    const int *n_samples;
    const unsigned char *reset, *final;
    const unsigned *state_in;
    unsigned *state_out;
    float *score0, *score1;
    int *n_out;
    int k, cap;
};

// One workgroup per stream, before the tick's launches: checks the stream's inputs, writes its plan, and for a stream that runs lays
// out `carry || new` samples and the histories in the row buffers.  A refused stream (n_samples outside its range, a record whose
// counter no tick could have written) touches nothing but its plan; an idle one (no samples, not final) copies its record.
__global__ __launch_bounds__(256) void stream_open_kernel(StreamIO io, StreamWs ws) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const unsigned *rin = io.state_in + (size_t)s * R_WORDS;
    unsigned *rout = io.state_out + (size_t)s * R_WORDS;
    int *plan = ws.plan + (size_t)s * PLAN_WORDS;
    const int n = io.n_samples[s];
    const bool rs = io.reset && io.reset[s], fin = io.final && io.final[s];
    const long long fed0 = rs ? 0 : *reinterpret_cast<const long long *>(rin + R_FED);
    const long long emit0 = rs ? 0 : *reinterpret_cast<const long long *>(rin + R_EMIT);
    const bool ok = n >= 0 && n <= io.k * HOP2 && (fin || n % HOP2 == 0) && fed0 >= 0 && fed0 % HOP2 == 0 && emit0 >= 0;
    if (!ok) {
        if (tid == 0) { plan[PL_ACTIVE] = -1; ws.fe_len[s] = 0; ws.fe_frames[s] = 0; }
        return;
    }
    float *sc0 = io.score0 + (size_t)s * io.cap, *sc1 = io.score1 + (size_t)s * io.cap;
    for (int e = tid; e < io.cap; e += 256) { sc0[e] = __builtin_nanf(""); sc1[e] = __builtin_nanf(""); }
    if (n == 0 && !fin) {
        if (tid == 0) { plan[PL_ACTIVE] = 0; ws.fe_len[s] = 0; ws.fe_frames[s] = 0; io.n_out[s] = 0; }
        for (int e = tid; e < R_WORDS; e += 256) rout[e] = rs ? 0u : rin[e];
        return;
    }
    const long long J64 = fed0 / HOP2;
    const int J = J64 > J_CLAMP ? J_CLAMP : (int)J64;         // only the distance to frame 0 matters, and only while it is below the look-ahead
    const int kf = n / HOP2;
    const int T1 = J + kf + 1, F = 2 * J + n / 160 + 1;       // final: the virtual clip's encoder / log-mel frame counts
    const int mel_end = fin ? F : 2 * (J + kf) - 1;
    const int sc_end = fin ? T1 - 1 : J + kf - LOOKAHEAD;
    const int o0 = J - LOOKAHEAD;
    const int nout = (sc_end > 0 ? sc_end : 0) - (o0 > 0 ? o0 : 0);
    if (tid == 0) {
        plan[PL_ACTIVE] = 1; plan[PL_J] = J; plan[PL_N] = n; plan[PL_FINAL] = fin ? 1 : 0; plan[PL_KF] = kf;
        plan[PL_NOUT] = nout > 0 ? nout : 0; plan[PL_MEL_END] = mel_end;
        for (int i = 0; i < 4; ++i) plan[PL_END + i] = fin ? T1 : J + kf - ST_OFF[i];
        plan[PL_END + 4] = sc_end;
        ws.fe_len[s] = CARRY + n;
        ws.fe_frames[s] = mel_end - (2 * J - 1);
        io.n_out[s] = nout > 0 ? nout : 0;
    }
    const int16_t *carry = reinterpret_cast<const int16_t *>(rin + R_PCM);
    const int16_t *src = io.samples + (long long)s * io.sample_stride;
    int16_t *row = ws.pcm + (size_t)s * ws.pcm_w;
    for (int e = tid; e < ws.pcm_w; e += 256) row[e] = e < CARRY ? (rs ? (int16_t)0 : carry[e]) : (e - CARRY < n ? src[e - CARRY] : (int16_t)0);
    float *mel = ws.rows[0] + (size_t)s * ws.w[0] * 80;
    for (int e = tid; e < ST_HIST[0] * 80; e += 256) mel[e] = rs ? 0.f : __uint_as_float(rin[R_MEL + e]);
#pragma unroll
    for (int i = 1; i < 5; ++i) {
        const int H = ST_HIST[i], Cn = ST_CH[i - 1], W = ws.w[i];
        float *dst = ws.rows[i] + (size_t)s * Cn * W;
        for (int e = tid; e < Cn * H; e += 256) {
            const int ch = e / H, col = e - ch * H;
            dst[(size_t)ch * W + col] = rs ? 0.f : __uint_as_float(rin[ST_REC[i] + e]);
        }
    }
}

// One workgroup per stream, behind the tick's launches: the record a stream that ran leaves -- all zeros after its final tick, else the
// last frames of every row buffer (a frame below 0 is padding and stays zero), the last 417 samples and the two counters.
__global__ __launch_bounds__(256) void stream_close_kernel(StreamIO io, StreamWs ws) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int *plan = ws.plan + (size_t)s * PLAN_WORDS;
    if (plan[PL_ACTIVE] != 1) return;
    const unsigned *rin = io.state_in + (size_t)s * R_WORDS;
    unsigned *rout = io.state_out + (size_t)s * R_WORDS;
    if (plan[PL_FINAL]) {
        for (int e = tid; e < R_WORDS; e += 256) rout[e] = 0u;
        return;
    }
    const int J = plan[PL_J], kf = plan[PL_KF], n = plan[PL_N];
    const bool rs = io.reset && io.reset[s];
    const float *mel = ws.rows[0] + (size_t)s * ws.w[0] * 80;
    for (int e = tid; e < ST_HIST[0] * 80; e += 256) {
        const int r = e / 80 + 2 * kf;                          // row r of the buffer = log-mel frame 2J - 11 + r
        rout[R_MEL + e] = 2 * J - 11 + r >= 0 ? __float_as_uint(mel[(size_t)r * 80 + (e % 80)]) : 0u;
    }
#pragma unroll
    for (int i = 1; i < 5; ++i) {
        const int H = ST_HIST[i], Cn = ST_CH[i - 1], W = ws.w[i], g0 = J - ST_OFF[i - 1] - H;
        const float *src = ws.rows[i] + (size_t)s * Cn * W;
        for (int e = tid; e < Cn * H; e += 256) {
            const int ch = e / H, col = e - ch * H + kf;
            rout[ST_REC[i] + e] = g0 + col >= 0 ? __float_as_uint(src[(size_t)ch * W + col]) : 0u;
        }
    }
    const int16_t *row = ws.pcm + (size_t)s * ws.pcm_w;
    for (int e = tid; e < (R_FED - R_PCM); e += 256) {           // two samples per word
        const int a = 2 * e, b = 2 * e + 1;
        const unsigned lo = a < CARRY ? (unsigned short)row[n + a] : 0u, hi = b < CARRY ? (unsigned short)row[n + b] : 0u;
        rout[R_PCM + e] = lo | (hi << 16);
    }
    if (tid == 0) {
        const long long fed0 = rs ? 0 : *reinterpret_cast<const long long *>(rin + R_FED);
        const long long emit0 = rs ? 0 : *reinterpret_cast<const long long *>(rin + R_EMIT);
        *reinterpret_cast<long long *>(rout + R_FED) = fed0 + n;
        *reinterpret_cast<long long *>(rout + R_EMIT) = emit0 + plan[PL_NOUT];
    }
}

}  // namespace marblenet
}  // namespace vadx

using namespace vadx::marblenet;

// the derived fields of a Cfg whose shape fields are set and checked: the halo tile's row stride and whether the output overwrites it
static void finish_cfg(Cfg *c) {
    const int width = (TILE - 1) * c->stride + (c->k - 1) * c->dil + 1;
    c->in_ld = c->has_dw ? (((width + 7) & ~7) + 4) : A_LD;      // % 8 == 4; a plain 1x1 block feeds IN straight to the GEMM
    c->out_alias = out_aliases_in(c->cinp, c->coutp, c->cresp, c->in_ld, c->has_dw) ? 1 : 0;
}
// bytes of the fp16 x 2 prologue's operand planes behind D
static size_t prologue_plane_bytes(const Cfg &c) { return (size_t)((c.cinp + 31) / 32) * 4 * TILE * 16 * 2; }
// the fused block's / the tail's geometry and LDS (the rectangular and the ragged entry points launch the same tiles)
static Blk2 make_blk2(int cin, int kernel, int frames) {
    Blk2 c;
    c.cin = cin; c.cinp = (cin + 15) & ~15; c.c1 = 64; c.c2 = 64; c.T = frames;
    const int width = W1 + kernel - 1;
    c.in_ld = width + ((4 - width % 8) + 8) % 8;             // smallest row stride >= width with stride % 8 == 4
    return c;
}
static size_t blk2_lds(const Blk2 &c, bool planes) {
    return ((size_t)c.cinp * c.in_ld + (size_t)c.c1 * H_LD + (size_t)c.c2 * A_LD) * sizeof(float) + (planes ? 2 * 8 * W1 * 16 : 0);
}
static Tail make_tail(int frames) {
    Tail c;
    c.cin = 64; c.cmid = 128; c.k = 29; c.dil = 2; c.T = frames;
    c.in_ld = ((TILE + 56 + 7) & ~7) + 4;
    return c;
}
static size_t tail_lds(const Tail &c) { return ((size_t)c.cin * c.in_ld + (size_t)c.cin * A_LD + (size_t)c.cmid * A_LD) * sizeof(float); }

extern "C" int vadx_sepconv_block(const vadx_sepconv_cfg *cfg, const float *dw_w, const float *pw_w, const float *pw_b,
                                  const float *res_w, const float *res_b, const float *x, int64_t xs_b, int64_t xs_c,
                                  int64_t xs_t, int t_in, const float *xres, float *y, int batch, int t_out, void *stream,
                                  const vadx_marblenet_cfg *mcfg) {
    VADX_REQUIRE(cfg && pw_w && pw_b && x && y, "vadx_sepconv_block: NULL argument");
    const int ar = vadx::arith_internal(mcfg ? mcfg->arithmetic : VADX_ARITH_AUTO, vadx::VADX_AR_F32);
    VADX_REQUIRE(ar == vadx::VADX_AR_F32 || ar == vadx::VADX_AR_H2, "vadx_sepconv_block: arithmetic must be AUTO / F32 or F16X2");
    unsigned *flag = mcfg ? static_cast<unsigned *>(mcfg->range_flag) : nullptr;
    Cfg c;
    c.cin = cfg->cin; c.cout = cfg->cout; c.k = cfg->kernel; c.stride = cfg->stride; c.dil = cfg->dilation;
    c.has_dw = cfg->depthwise ? 1 : 0; c.cres = cfg->residual_cin; c.relu = cfg->relu ? 1 : 0;
    c.pad = (c.dil * (c.k - 1)) / 2;
    c.cinp = (c.cin + 15) & ~15; c.coutp = (c.cout + 15) & ~15; c.cresp = (c.cres + 15) & ~15;
    VADX_REQUIRE(c.cin > 0 && c.cin <= MAXC && c.cout > 0 && c.cout <= MAXC && c.cres >= 0 && c.cres <= MAXC,
                 "vadx_sepconv_block: channels must be in [1,128]");
    VADX_REQUIRE(c.k >= 1 && c.stride >= 1 && c.dil >= 1 && (TILE - 1) * c.stride + (c.k - 1) * c.dil + 1 <= IN_LD_MAX,
                 "vadx_sepconv_block: receptive field of a 32-frame tile exceeds %d samples", IN_LD_MAX);
    finish_cfg(&c);
    size_t lds_bytes = lds_floats(c.cinp, c.coutp, c.cresp, c.in_ld, c.has_dw) * sizeof(float);
    if (ar == vadx::VADX_AR_H2) {
        VADX_REQUIRE(flag && c.has_dw && !c.cres && c.out_alias && c.coutp == 128 && c.k == 11 && c.dil == 1 && c.stride == 2,
                     "vadx_sepconv_block: F16X2 is built for the MarbleNet prologue (depthwise k 11 stride 2, 128 filters, no residual; pw_w from "
                     "vadx_frag_h2_host VADX_H2_K_PLAIN) and needs mcfg->range_flag");
        lds_bytes += prologue_plane_bytes(c);
    }
    VADX_REQUIRE(c.has_dw ? dw_w != nullptr : (c.k == 1 && c.stride == 1), "vadx_sepconv_block: plain conv must be k=1, stride 1");
    VADX_REQUIRE(!c.cres || (res_w && res_b && xres), "vadx_sepconv_block: residual branch needs res_w/res_b/xres");
    VADX_REQUIRE(batch > 0 && t_in > 0 && t_out > 0 && t_out == (t_in + 2 * c.pad - c.dil * (c.k - 1) - 1) / c.stride + 1,
                 "vadx_sepconv_block: t_out=%d inconsistent with t_in=%d", t_out, t_in);
    // the residual tile is read as xres[b][ch][t0 + m] with row length t_out: the block input must have this sub-block's output frames
    VADX_REQUIRE(!c.cres || (c.stride == 1 && t_in == t_out),
                 "vadx_sepconv_block: a residual branch needs stride 1 and t_in == t_out (xres is [B][residual_cin][t_out]); got stride=%d "
                 "t_in=%d t_out=%d", c.stride, t_in, t_out);
    const int tiles = (t_out + TILE - 1) / TILE;
    VADX_REQUIRE((long long)batch * tiles < (1LL << 31), "vadx_sepconv_block: too many tiles");
#define SEPCONV_LAUNCH(...)                                                                                                     \
    do {                                                                                                                        \
        VADX_DYN_LDS((sepconv_block_kernel<__VA_ARGS__>), 128 * 1024);                                                          \
        hipLaunchKernelGGL((sepconv_block_kernel<__VA_ARGS__>), dim3((unsigned)(batch * tiles)), dim3(THREADS),                 \
                           lds_bytes, static_cast<hipStream_t>(stream), c, dw_w, pw_w, pw_b, res_w, res_b, x,                   \
                           (long long)xs_b, (long long)xs_c, (long long)xs_t, t_in, xres, y, t_out, tiles, flag, NoTables{});    \
    } while (0)
    // the depthwise shapes of the published MarbleNet 3x2x64 get compile-time FIRs; anything else runs the generic kernel
    if (ar == vadx::VADX_AR_H2) SEPCONV_LAUNCH(11, 1, 2, 2);
    else if (c.has_dw && c.k == 11 && c.dil == 1 && c.stride == 2) SEPCONV_LAUNCH(11, 1, 2);
    else if (c.has_dw && c.k == 13 && c.dil == 1 && c.stride == 1) SEPCONV_LAUNCH(13, 1, 1);
    else if (c.has_dw && c.k == 15 && c.dil == 1 && c.stride == 1) SEPCONV_LAUNCH(15, 1, 1);
    else if (c.has_dw && c.k == 17 && c.dil == 1 && c.stride == 1) SEPCONV_LAUNCH(17, 1, 1);
    else if (c.has_dw && c.k == 29 && c.dil == 2 && c.stride == 1) SEPCONV_LAUNCH(29, 2, 1);
    else SEPCONV_LAUNCH(0, 0, 0);
#undef SEPCONV_LAUNCH
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}


extern "C" int vadx_marblenet_block2(int cin, int kernel, const float *dw0, const float *pw0, const float *b0, const float *dw1,
                                     const float *pw1, const float *b1, const float *res_w, const float *res_b, const float *x,
                                     float *y, int batch, int frames, void *stream, const vadx_marblenet_cfg *cfg) {
    VADX_REQUIRE(dw0 && pw0 && b0 && dw1 && pw1 && b1 && res_w && res_b && x && y, "vadx_marblenet_block2: NULL argument");
    const int ar = vadx::arith_internal(cfg ? cfg->arithmetic : VADX_ARITH_AUTO, vadx::VADX_AR_F32);
    VADX_REQUIRE(ar == vadx::VADX_AR_F32 || ar == vadx::VADX_AR_H2, "vadx_marblenet_block2: arithmetic must be AUTO / F32 (fragment-major weights) or "
                 "F16X2 (vadx_frag_h2_host weights)");
    VADX_REQUIRE(ar != vadx::VADX_AR_H2 || cfg->range_flag, "vadx_marblenet_block2: F16X2 needs cfg->range_flag (two device words)");
    unsigned *flag = cfg ? static_cast<unsigned *>(cfg->range_flag) : nullptr;
    VADX_REQUIRE((cin == 64 || cin == 128) && (kernel == 13 || kernel == 15 || kernel == 17) && batch > 0 && frames > 0,
                 "vadx_marblenet_block2: built for the published MarbleNet 3x2x64 residual blocks (cin 64/128, 64 filters, kernel 13/15/17)");
    const Blk2 c = make_blk2(cin, kernel, frames);
    const int tiles = (frames + TILE - 1) / TILE;
    VADX_REQUIRE((long long)batch * tiles < (1LL << 31), "vadx_marblenet_block2: too many tiles");
    const bool planes = ar == vadx::VADX_AR_H2 && cin == 64;      // the plane form (AR = 3): 12 KB more, still three workgroups per CU
    const size_t lds = blk2_lds(c, planes);
    VADX_REQUIRE(c.cinp * c.in_ld >= c.c1 * A_LD, "vadx_marblenet_block2: the depthwise-1 output does not fit the input region");
#define BLK2_LAUNCH(KK, AR)                                                                                                    \
    do {                                                                                                                       \
        VADX_DYN_LDS((jasper_block2_kernel<KK, AR>), 128 * 1024);                                                              \
        hipLaunchKernelGGL((jasper_block2_kernel<KK, AR>), dim3((unsigned)(batch * tiles)), dim3(THREADS), lds,                \
                           static_cast<hipStream_t>(stream), c, dw0, pw0, b0, dw1, pw1, b1, res_w, res_b, x, y, tiles, flag,    \
                           NoTables{});                                                                                        \
    } while (0)
    if (planes) {
        if (kernel == 13) BLK2_LAUNCH(13, 3);
        else if (kernel == 15) BLK2_LAUNCH(15, 3);
        else BLK2_LAUNCH(17, 3);
    } else if (ar == vadx::VADX_AR_H2) {
        if (kernel == 13) BLK2_LAUNCH(13, 2);
        else if (kernel == 15) BLK2_LAUNCH(15, 2);
        else BLK2_LAUNCH(17, 2);
    } else {
        if (kernel == 13) BLK2_LAUNCH(13, 0);
        else if (kernel == 15) BLK2_LAUNCH(15, 0);
        else BLK2_LAUNCH(17, 0);
    }
#undef BLK2_LAUNCH
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_marblenet_tail(const float *dw, const float *pw, const float *pb, const float *w6, const float *b6,
                                   const float *dec_w, const float *dec_b, const float *x, float *score0, float *score1,
                                   int batch, int frames, void *stream, const vadx_marblenet_cfg *cfg) {
    VADX_REQUIRE(dw && pw && pb && w6 && b6 && dec_w && dec_b && x && score0 && score1, "vadx_marblenet_tail: NULL argument");
    const int ar = vadx::arith_internal(cfg ? cfg->arithmetic : VADX_ARITH_AUTO, vadx::VADX_AR_F32);
    VADX_REQUIRE(ar == vadx::VADX_AR_F32 || ar == vadx::VADX_AR_H2, "vadx_marblenet_tail: arithmetic must be AUTO / F32 (fragment-major weights) or "
                 "F16X2 (vadx_frag_h2_host weights, VADX_H2_K_PLAIN)");
    VADX_REQUIRE(ar != vadx::VADX_AR_H2 || cfg->range_flag, "vadx_marblenet_tail: F16X2 needs cfg->range_flag (two device words)");
    unsigned *flag = cfg ? static_cast<unsigned *>(cfg->range_flag) : nullptr;
    VADX_REQUIRE(batch > 0 && frames > 0, "vadx_marblenet_tail: bad shape");
    const Tail c = make_tail(frames);
    const int tiles = (frames + TILE - 1) / TILE;
    VADX_REQUIRE((long long)batch * tiles < (1LL << 31), "vadx_marblenet_tail: too many tiles");
    const size_t lds = tail_lds(c);
    if (ar == vadx::VADX_AR_H2) {
        VADX_DYN_LDS(marblenet_tail_kernel<2>, 128 * 1024);
        hipLaunchKernelGGL(marblenet_tail_kernel<2>, dim3((unsigned)(batch * tiles)), dim3(THREADS), lds, static_cast<hipStream_t>(stream),
                           c, dw, pw, pb, w6, b6, dec_w, dec_b, x, score0, score1, tiles, flag, NoTables{});
    } else {
        VADX_DYN_LDS(marblenet_tail_kernel<0>, 128 * 1024);
        hipLaunchKernelGGL(marblenet_tail_kernel<0>, dim3((unsigned)(batch * tiles)), dim3(THREADS), lds, static_cast<hipStream_t>(stream),
                           c, dw, pw, pb, w6, b6, dec_w, dec_b, x, score0, score1, tiles, flag, NoTables{});
    }
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

// ---- ragged launches: the same tiles, (clip, tile) from the tables of a vadx_marblenet_ragged
// Host-side checks shared by the three entry points (`who` names the caller in the message); fills the device-side table struct
static int ragged_tables(const char *who, const vadx_marblenet_ragged *rt, bool with_src, Ragged *r) {
    VADX_REQUIRE(rt && rt->tile_first && rt->tile_clip && rt->frame_first && (!with_src || rt->src_first), "%s: NULL table", who);
    VADX_REQUIRE(rt->clips >= 1 && rt->n_tiles >= 1 && rt->frames_total >= 1, "%s: clips=%d n_tiles=%d frames_total=%d must be positive", who,
                 rt->clips, rt->n_tiles, rt->frames_total);
    // every clip has at least one frame and every tile at least one of its <= 32 frames
    VADX_REQUIRE(rt->clips <= rt->n_tiles && rt->n_tiles <= rt->frames_total && (long long)rt->frames_total <= (long long)rt->n_tiles * TILE,
                 "%s: clips=%d, n_tiles=%d and frames_total=%d do not fit each other (clips <= n_tiles <= frames_total <= %d * n_tiles)", who,
                 rt->clips, rt->n_tiles, rt->frames_total, TILE);
    // T1 = (F - 1) / 2 + 1 per clip, so sum T1 <= sum F <= 2 * sum T1
    VADX_REQUIRE(!with_src || (rt->src_total >= rt->frames_total && (long long)rt->src_total <= 2LL * rt->frames_total),
                 "%s: src_total=%d does not fit frames_total=%d (the stride-2 prologue: frames_total <= src_total <= 2 * frames_total)", who,
                 rt->src_total, rt->frames_total);
    r->tile_first = rt->tile_first; r->tile_clip = rt->tile_clip; r->dst_first = rt->frame_first;
    r->src_first = with_src ? rt->src_first : rt->frame_first;
    r->clips = rt->clips; r->n_tiles = rt->n_tiles; r->dst_total = rt->frames_total; r->src_total = with_src ? rt->src_total : rt->frames_total;
    return VADX_OK;
}
// AUTO / F32 -> VADX_AR_F32, F16X2 (with a flag) -> VADX_AR_H2, anything else refused by name
static int ragged_arith(const char *who, const vadx_marblenet_cfg *cfg, int *ar, unsigned **flag) {
    *ar = vadx::arith_internal(cfg ? cfg->arithmetic : VADX_ARITH_AUTO, vadx::VADX_AR_F32);
    VADX_REQUIRE(*ar == vadx::VADX_AR_F32 || *ar == vadx::VADX_AR_H2, "%s: arithmetic %d is not built: AUTO / F32 (fragment-major weights) or F16X2 "
                 "(vadx_frag_h2_host weights)", who, cfg ? cfg->arithmetic : VADX_ARITH_AUTO);
    *flag = cfg ? static_cast<unsigned *>(cfg->range_flag) : nullptr;
    VADX_REQUIRE(*ar != vadx::VADX_AR_H2 || *flag, "%s: F16X2 needs cfg->range_flag (two device words)", who);
    return VADX_OK;
}

extern "C" int vadx_sepconv_block_ragged(const vadx_sepconv_cfg *cfg, const float *dw_w, const float *pw_w, const float *pw_b, const float *x,
                                         int64_t xs_t, float *y, const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *mcfg) {
    static const char who[] = "vadx_sepconv_block_ragged";
    VADX_REQUIRE(cfg && dw_w && pw_w && pw_b && x && y, "%s: NULL argument", who);
    int ar;
    unsigned *flag;
    Ragged r;
    if (int rc = ragged_arith(who, mcfg, &ar, &flag)) return rc;
    if (int rc = ragged_tables(who, rt, true, &r)) return rc;
    VADX_REQUIRE(cfg->depthwise && cfg->kernel == 11 && cfg->stride == 2 && cfg->dilation == 1 && cfg->residual_cin == 0 && cfg->cin > 0 &&
                 cfg->cin <= MAXC && cfg->cout > 0 && cfg->cout <= MAXC && xs_t >= cfg->cin,
                 "%s: built for the MarbleNet prologue (depthwise k 11 stride 2, no residual, <= 128 channels) on time-major rows of xs_t >= cin floats", who);
    Cfg c;
    c.cin = cfg->cin; c.cout = cfg->cout; c.k = 11; c.stride = 2; c.dil = 1; c.has_dw = 1; c.cres = 0; c.relu = cfg->relu ? 1 : 0;
    c.pad = 5;
    c.cinp = (c.cin + 15) & ~15; c.coutp = (c.cout + 15) & ~15; c.cresp = 0;
    finish_cfg(&c);
    size_t lds_bytes = lds_floats(c.cinp, c.coutp, c.cresp, c.in_ld, c.has_dw) * sizeof(float);
    if (ar == vadx::VADX_AR_H2) {
        VADX_REQUIRE(c.out_alias && c.coutp == 128, "%s: F16X2 needs 128 filters (pw_w from vadx_frag_h2_host VADX_H2_K_PLAIN)", who);
        lds_bytes += prologue_plane_bytes(c);
        VADX_DYN_LDS((sepconv_block_kernel<11, 1, 2, 2, true>), 128 * 1024);
        hipLaunchKernelGGL((sepconv_block_kernel<11, 1, 2, 2, true>), dim3((unsigned)r.n_tiles), dim3(THREADS), lds_bytes, static_cast<hipStream_t>(stream),
                           c, dw_w, pw_w, pw_b, nullptr, nullptr, x, 0LL, 1LL, (long long)xs_t, 0, nullptr, y, 0, 0, flag, r);
    } else {
        VADX_DYN_LDS((sepconv_block_kernel<11, 1, 2, 0, true>), 128 * 1024);
        hipLaunchKernelGGL((sepconv_block_kernel<11, 1, 2, 0, true>), dim3((unsigned)r.n_tiles), dim3(THREADS), lds_bytes, static_cast<hipStream_t>(stream),
                           c, dw_w, pw_w, pw_b, nullptr, nullptr, x, 0LL, 1LL, (long long)xs_t, 0, nullptr, y, 0, 0, flag, r);
    }
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_marblenet_block2_ragged(int cin, int kernel, const float *dw0, const float *pw0, const float *b0, const float *dw1,
                                            const float *pw1, const float *b1, const float *res_w, const float *res_b, const float *x, float *y,
                                            const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *cfg) {
    static const char who[] = "vadx_marblenet_block2_ragged";
    VADX_REQUIRE(dw0 && pw0 && b0 && dw1 && pw1 && b1 && res_w && res_b && x && y, "%s: NULL argument", who);
    int ar;
    unsigned *flag;
    Ragged r;
    if (int rc = ragged_arith(who, cfg, &ar, &flag)) return rc;
    if (int rc = ragged_tables(who, rt, false, &r)) return rc;
    VADX_REQUIRE((cin == 64 || cin == 128) && (kernel == 13 || kernel == 15 || kernel == 17),
                 "%s: built for the published MarbleNet 3x2x64 residual blocks (cin 64/128, 64 filters, kernel 13/15/17)", who);
    const Blk2 c = make_blk2(cin, kernel, 0);                // (T comes from the tables)
    VADX_REQUIRE(c.cinp * c.in_ld >= c.c1 * A_LD, "%s: the depthwise-1 output does not fit the input region", who);
    const bool planes = ar == vadx::VADX_AR_H2 && cin == 64;
    const size_t lds = blk2_lds(c, planes);
#define BLK2_RAGGED(KK, AR)                                                                                                    \
    do {                                                                                                                       \
        VADX_DYN_LDS((jasper_block2_kernel<KK, AR, true>), 128 * 1024);                                                        \
        hipLaunchKernelGGL((jasper_block2_kernel<KK, AR, true>), dim3((unsigned)r.n_tiles), dim3(THREADS), lds,                \
                           static_cast<hipStream_t>(stream), c, dw0, pw0, b0, dw1, pw1, b1, res_w, res_b, x, y, 0, flag, r);    \
    } while (0)
    if (planes) {
        if (kernel == 13) BLK2_RAGGED(13, 3);
        else if (kernel == 15) BLK2_RAGGED(15, 3);
        else BLK2_RAGGED(17, 3);
    } else if (ar == vadx::VADX_AR_H2) {
        if (kernel == 13) BLK2_RAGGED(13, 2);
        else if (kernel == 15) BLK2_RAGGED(15, 2);
        else BLK2_RAGGED(17, 2);
    } else {
        if (kernel == 13) BLK2_RAGGED(13, 0);
        else if (kernel == 15) BLK2_RAGGED(15, 0);
        else BLK2_RAGGED(17, 0);
    }
#undef BLK2_RAGGED
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_marblenet_tail_ragged(const float *dw, const float *pw, const float *pb, const float *w6, const float *b6,
                                          const float *dec_w, const float *dec_b, const float *x, float *score0, float *score1,
                                          const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *cfg) {
    static const char who[] = "vadx_marblenet_tail_ragged";
    VADX_REQUIRE(dw && pw && pb && w6 && b6 && dec_w && dec_b && x && score0 && score1, "%s: NULL argument", who);
    int ar;
    unsigned *flag;
    Ragged r;
    if (int rc = ragged_arith(who, cfg, &ar, &flag)) return rc;
    if (int rc = ragged_tables(who, rt, false, &r)) return rc;
    const Tail c = make_tail(0);                             // (T comes from the tables)
    const size_t lds = tail_lds(c);
    if (ar == vadx::VADX_AR_H2) {
        VADX_DYN_LDS((marblenet_tail_kernel<2, true>), 128 * 1024);
        hipLaunchKernelGGL((marblenet_tail_kernel<2, true>), dim3((unsigned)r.n_tiles), dim3(THREADS), lds, static_cast<hipStream_t>(stream),
                           c, dw, pw, pb, w6, b6, dec_w, dec_b, x, score0, score1, 0, flag, r);
    } else {
        VADX_DYN_LDS((marblenet_tail_kernel<0, true>), 128 * 1024);
        hipLaunchKernelGGL((marblenet_tail_kernel<0, true>), dim3((unsigned)r.n_tiles), dim3(THREADS), lds, static_cast<hipStream_t>(stream),
                           c, dw, pw, pb, w6, b6, dec_w, dec_b, x, score0, score1, 0, flag, r);
    }
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

// ---- live streams: one tick = open, the stream front-end, the five encoder launches on the streams' row buffers, close
extern "C" int vadx_marblenet_stream_max_frames(void) { return K_MAX; }
extern "C" int vadx_marblenet_stream_cap(int k) { return k >= 1 && k <= K_MAX ? k + LOOKAHEAD : 0; }
extern "C" size_t vadx_marblenet_stream_state_bytes(int streams) { return streams >= 1 ? (size_t)streams * R_WORDS * 4 : 0; }
extern "C" size_t vadx_marblenet_stream_workspace_bytes(int streams, int k) {
    if (streams < 1 || k < 1 || k > K_MAX) return 0;
    StreamWs ws;
    return stream_ws_layout(streams, k, &ws, nullptr);
}

extern "C" int vadx_marblenet_stream_tick(const vadx_frontend_cfg *fe, const float *fe_packed, const int32_t *mel_kb_host,
                                          const vadx_marblenet_stream_weights *w, const int16_t *samples, int64_t sample_stride,
                                          const int32_t *n_samples, const uint8_t *reset, const uint8_t *final, int streams, int k,
                                          const void *state_in, void *state_out, float *score0, float *score1, int32_t *n_out,
                                          void *workspace, size_t workspace_bytes, void *stream, const vadx_marblenet_cfg *cfg) {
    static const char who[] = "vadx_marblenet_stream_tick";
    VADX_REQUIRE(fe && fe_packed && mel_kb_host && w && samples && n_samples && state_in && state_out && score0 && score1 && n_out && workspace,
                 "%s: NULL argument", who);
    VADX_REQUIRE(w->p_dw && w->p_pw && w->p_pb && w->t_dw && w->t_pw && w->t_pb && w->t_w6 && w->t_b6 && w->dec_w && w->dec_b, "%s: NULL weight", who);
    for (int i = 0; i < 3; ++i)
        VADX_REQUIRE(w->b_dw0[i] && w->b_pw0[i] && w->b_b0[i] && w->b_dw1[i] && w->b_pw1[i] && w->b_b1[i] && w->b_rw[i] && w->b_rb[i],
                     "%s: NULL weight of block %d", who, i + 2);
    VADX_REQUIRE(streams >= 1, "%s: streams=%d must be at least 1", who, streams);
    VADX_REQUIRE(k >= 1 && k <= K_MAX, "%s: k=%d frames per tick is outside [1, %d]", who, k, K_MAX);
    VADX_REQUIRE(sample_stride >= (int64_t)k * HOP2, "%s: sample_stride=%lld is shorter than a row of k * 320 = %d samples", who,
                 (long long)sample_stride, k * HOP2);
    int ar;
    unsigned *flag;
    if (int rc = ragged_arith(who, cfg, &ar, &flag)) return rc;
    // the front-end's own refusals, by name and before any HIP call (vadx_frontend_logmel_stream repeats them)
    VADX_REQUIRE(fe->fold == VADX_FE_KIND_SPLIT_H2 || fe->fold == VADX_FE_KIND_SPLIT_B3, "%s: DFT product kind %d is not built for streams "
                 "(VADX_FE_KIND_SPLIT_H2 = %d or VADX_FE_KIND_SPLIT_B3 = %d)", who, fe->fold, (int)VADX_FE_KIND_SPLIT_H2, (int)VADX_FE_KIND_SPLIT_B3);
    VADX_REQUIRE(fe->prep == 1 && fe->hop == 160 && fe->in_window_len <= 0 && fe->n_mels == 80 && fe->center_pad == 256,
                 "%s: front-end prep %d, hop %d, in_window_len %d, n_mels %d, centre pad %d is not the MarbleNet preset at 16 kHz (prep 1, hop 160, "
                 "no in-graph resampling, 80 mels, centre pad 256)", who, fe->prep, fe->hop, fe->in_window_len, fe->n_mels, fe->center_pad);
    StreamWs ws;
    const size_t need = stream_ws_layout(streams, k, &ws, static_cast<char *>(workspace));
    VADX_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, vadx_marblenet_stream_workspace_bytes(%d, %d) = %zu", who, workspace_bytes,
                 streams, k, need);
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(state_in) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(state_out) & 15) == 0, "%s: workspace and records must be 16-byte aligned", who);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, vadx_marblenet_stream_state_bytes(streams)),
                 "%s: state_out must be a second record (state_in is never written)", who);
    const int cap = k + LOOKAHEAD;
    int tiles[5];
    for (int i = 0; i < 5; ++i) tiles[i] = (k + ST_EXTRA[i] + TILE - 1) / TILE;
    VADX_REQUIRE((long long)streams * tiles[4] < (1LL << 31), "%s: too many tiles", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const StreamIO io{samples, (long long)sample_stride, n_samples, reset, final, static_cast<const unsigned *>(state_in),
                      static_cast<unsigned *>(state_out), score0, score1, n_out, k, cap};
    hipLaunchKernelGGL(stream_open_kernel, dim3((unsigned)streams), dim3(256), 0, st, io, ws);
    VADX_HIP_TRY(hipGetLastError());
    if (int rc = vadx_frontend_logmel_stream(fe, fe_packed, mel_kb_host, ws.pcm, ws.pcm_w, ws.fe_len, ws.fe_frames, streams, 2 * k + 2, ws.rows[0],
                                             ws.w[0], ST_HIST[0], stream))
        return rc;
    auto tables = [&](int stage) {
        return Stream{ws.plan, stage, ST_OFF[stage], stage ? ST_OFF[stage - 1] : 0, ST_HIST[stage], stage < 4 ? ST_HIST[stage + 1] : 0,
                      ws.w[stage], stage < 4 ? ws.w[stage + 1] : cap, tiles[stage], streams};
    };
    {   // the prologue on the time-major log-mel rows
        Cfg c;
        c.cin = 80; c.cout = 128; c.k = 11; c.stride = 2; c.dil = 1; c.has_dw = 1; c.cres = 0; c.relu = 1; c.pad = 5;
        c.cinp = 80; c.coutp = 128; c.cresp = 0;
        finish_cfg(&c);
        size_t lds_bytes = lds_floats(c.cinp, c.coutp, c.cresp, c.in_ld, c.has_dw) * sizeof(float);
        const Stream r = tables(0);
        if (ar == vadx::VADX_AR_H2) {
            VADX_REQUIRE(c.out_alias, "%s: the fp16 x 2 prologue needs its output in the input tile's place", who);
            lds_bytes += prologue_plane_bytes(c);
            VADX_DYN_LDS((sepconv_block_kernel<11, 1, 2, 2, 2>), 128 * 1024);
            hipLaunchKernelGGL((sepconv_block_kernel<11, 1, 2, 2, 2>), dim3((unsigned)(streams * r.tiles)), dim3(THREADS), lds_bytes, st, c, w->p_dw,
                               w->p_pw, w->p_pb, nullptr, nullptr, ws.rows[0], 0LL, 1LL, 80LL, 0, nullptr, ws.rows[1], 0, 0, flag, r);
        } else {
            VADX_DYN_LDS((sepconv_block_kernel<11, 1, 2, 0, 2>), 128 * 1024);
            hipLaunchKernelGGL((sepconv_block_kernel<11, 1, 2, 0, 2>), dim3((unsigned)(streams * r.tiles)), dim3(THREADS), lds_bytes, st, c, w->p_dw,
                               w->p_pw, w->p_pb, nullptr, nullptr, ws.rows[0], 0LL, 1LL, 80LL, 0, nullptr, ws.rows[1], 0, 0, flag, r);
        }
        VADX_HIP_TRY(hipGetLastError());
    }
    for (int i = 0; i < 3; ++i) {
        const int cin = i == 0 ? 128 : 64, kernel = 13 + 2 * i;
        const Blk2 c = make_blk2(cin, kernel, 0);                // (T comes from the plan)
        VADX_REQUIRE(c.cinp * c.in_ld >= c.c1 * A_LD, "%s: the depthwise-1 output does not fit the input region", who);
        const bool planes = ar == vadx::VADX_AR_H2 && cin == 64;
        const size_t lds = blk2_lds(c, planes);
        const Stream r = tables(1 + i);
#define BLK2_STREAM(KK, AR)                                                                                                        \
    do {                                                                                                                           \
        VADX_DYN_LDS((jasper_block2_kernel<KK, AR, 2>), 128 * 1024);                                                               \
        hipLaunchKernelGGL((jasper_block2_kernel<KK, AR, 2>), dim3((unsigned)(streams * r.tiles)), dim3(THREADS), lds, st, c,      \
                           w->b_dw0[i], w->b_pw0[i], w->b_b0[i], w->b_dw1[i], w->b_pw1[i], w->b_b1[i], w->b_rw[i], w->b_rb[i],      \
                           ws.rows[1 + i], ws.rows[2 + i], 0, flag, r);                                                            \
    } while (0)
        // the arithmetics of the whole-clip launches: block 2 (128 channels in) splits in the GEMM waves, blocks 3 / 4 read operand planes
        if (ar != vadx::VADX_AR_H2) {
            if (i == 0) BLK2_STREAM(13, 0);
            else if (i == 1) BLK2_STREAM(15, 0);
            else BLK2_STREAM(17, 0);
        } else {
            if (i == 0) BLK2_STREAM(13, 2);
            else if (i == 1) BLK2_STREAM(15, 3);
            else BLK2_STREAM(17, 3);
        }
#undef BLK2_STREAM
        VADX_HIP_TRY(hipGetLastError());
    }
    {
        const Tail c = make_tail(0);
        const size_t lds = tail_lds(c);
        const Stream r = tables(4);
        if (ar == vadx::VADX_AR_H2) {
            VADX_DYN_LDS((marblenet_tail_kernel<2, 2>), 128 * 1024);
            hipLaunchKernelGGL((marblenet_tail_kernel<2, 2>), dim3((unsigned)(streams * r.tiles)), dim3(THREADS), lds, st, c, w->t_dw, w->t_pw, w->t_pb,
                               w->t_w6, w->t_b6, w->dec_w, w->dec_b, ws.rows[4], score0, score1, 0, flag, r);
        } else {
            VADX_DYN_LDS((marblenet_tail_kernel<0, 2>), 128 * 1024);
            hipLaunchKernelGGL((marblenet_tail_kernel<0, 2>), dim3((unsigned)(streams * r.tiles)), dim3(THREADS), lds, st, c, w->t_dw, w->t_pw, w->t_pb,
                               w->t_w6, w->t_b6, w->dec_w, w->dec_b, ws.rows[4], score0, score1, 0, flag, r);
        }
        VADX_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(stream_close_kernel, dim3((unsigned)streams), dim3(256), 0, st, io, ws);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_frame_classifier(const float *enc, const float *dec_w, const float *dec_b, int batch, int channels,
                                     int frames, float *score0, float *score1, void *stream) {
    VADX_REQUIRE(enc && dec_w && dec_b && score0 && score1, "vadx_frame_classifier: NULL argument");
    VADX_REQUIRE(batch > 0 && channels > 0 && frames > 0, "vadx_frame_classifier: bad shape");
    const long long n = (long long)batch * frames;
    hipLaunchKernelGGL(frame_classifier_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), enc, dec_w, dec_b, batch, channels, frames, score0, score1);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
