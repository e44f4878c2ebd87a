// dfsmn.hip -- DFSMN near+far VAD (SDAEC ICCRN echo canceller + mask-net) building blocks for gfx950.
// Reference: DFSMN/near_and_far_end_audio/Export_DFSMN_VAD.py:65-354.
//
// Activation layout ("FT", frame-tiled): a tensor with C channels over F bins and T frames is stored as
//     [tile = chunk*NT + t/16][C][F][16]        element (c, f, t) at ((tile*C + c)*F + f)*16 + t%16
// so the 16 frames of a tile are the 16 COLUMNS of every MFMA tile: every op of the ICCRN that is
// independent per frame (LayerNorm over (C,F), 1x1 / (3,1) convs, the length-160 DFT of CepsUnit, the
// bi-LSTMs that run ALONG the frequency axis) becomes an f32-MFMA GEMM whose other operand (weights,
// DFT tables) is stationary in VGPRs.  The LSTMs that run along TIME use 16 bins as the columns.
// LSTM recurrences keep h and c in registers: with gate rows ordered (unit-quad q, gate r) the D
// fragment of step t is exactly the B fragment of step t+1 -- no LDS, no shuffles.
#include "common.h"
#include "split_scheme.h"
#include "layers.h"

#include <math.h>
#include <type_traits>
#include <string.h>

namespace vadx {
namespace dfsmn {

struct View {            // channel slice [c_off, c_off + c) of an FT tensor with c_total channels
    const float *ptr;
    int c_total, c_off, c;
};
struct ViewW {
    float *ptr;
    int c_total, c_off, c;
};

__device__ __forceinline__ size_t ft_idx(int tile, int c_total, int c, int F, int f) {
    return (((size_t)tile * c_total + c) * F + f) * 16;
}

__device__ __forceinline__ float c_first(const View &a, const View &b, int tile, int F, int t) {
    return a.c > 0 ? a.ptr[ft_idx(tile, a.c_total, a.c_off, F, 0) + t] : b.ptr[ft_idx(tile, b.c_total, b.c_off, F, 0) + t];
}

// ---------------------------------------------------------------------------------------------
// LayerNorm statistics over (C, F) per frame: stats[tile][16][2] = (mean, 1/(std_unbiased + 1e-6))
// (LayerNorm.forward, Export_DFSMN_VAD.py:163-167).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void frame_stats_kernel(View a, View b, int F, float *__restrict__ stats) {
    // thread = (row group tid>>2, frame quad tid&3): 16-B loads, a wave reads 1 KiB contiguous.  ONE pass over the
    // tile: sums of d = x - K and d^2 with the shift K = the frame's first element (|K - mean| is of the order of the
    // standard deviation, so var = (S2 - S1^2/n) / (n-1) has none of the cancellation of the raw-moment formula).
    __shared__ f32x4 red1[64][4], red2[64][4];
    const int tile = blockIdx.x, tid = threadIdx.x, tq = tid & 3, rg = tid >> 2;
    const int n = (a.c + b.c) * F;
    auto at = [&](int e) -> f32x4 {
        const int c = e / F, f = e - c * F;
        const float *ptr = c < a.c ? a.ptr + ft_idx(tile, a.c_total, a.c_off + c, F, f)
                                   : b.ptr + ft_idx(tile, b.c_total, b.c_off + c - a.c, F, f);
        return *reinterpret_cast<const f32x4 *>(ptr + 4 * tq);
    };
    const f32x4 K = at(0);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    int e = rg;
    for (; e + 192 < n; e += 256) {          // four independent loads in flight per thread
        const f32x4 d0 = at(e) - K, d1 = at(e + 64) - K, d2 = at(e + 128) - K, d3 = at(e + 192) - K;
        s1 += (d0 + d1) + (d2 + d3);
        s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    for (; e < n; e += 64) { const f32x4 d = at(e) - K; s1 += d; s2 += d * d; }
    red1[rg][tq] = s1;
    red2[rg][tq] = s2;
    __syncthreads();
    if (tid < 16) {
        float S1 = 0.f, S2 = 0.f;
        for (int g = 0; g < 64; ++g) { S1 += red1[g][tid >> 2][tid & 3]; S2 += red2[g][tid >> 2][tid & 3]; }
        const float k = (c_first(a, b, tile, F, tid));
        const float mean = k + S1 / (float)n;
        const float var = fmaxf(S2 - S1 * S1 / (float)n, 0.f) / (float)(n - 1);
        stats[((size_t)tile * 16 + tid) * 2] = mean;
        stats[((size_t)tile * 16 + tid) * 2 + 1] = 1.0f / (sqrtf(var) + 1e-6f);
    }
}

// ---------------------------------------------------------------------------------------------
// Fused LayerNorm statistics.  The kernels that PRODUCE a tensor (pw_conv, the forward dft_f) also emit, per frame, the
// (count, mean, M2 = sum (x - mean)^2) of what the workgroup wrote -- "partial statistics" [tile][PARTS][16][4] -- so
// that the consumer's (mean, 1/(std + eps)) come from a tiny merge kernel instead of another pass over the tensor
// (frame_stats re-read 1.4 GB per LayerNorm, 41 times per forward).  Accumulation: every thread owns one frame quad of
// the coalesced write-out, sums d = x - K and d^2 against its own first value K (no cancellation), and the partials
// are merged pairwise with Chan's update in a fixed order (reproducible).
// ---------------------------------------------------------------------------------------------
constexpr int STAT_PARTS = 2;            // partial slots per tile (pw_conv runs one or two workgroups per tile)

struct StatAcc {                         // short-lived: one write-out pass of one thread
    f32x4 K, s1, s2;
    float n;
    __device__ __forceinline__ void init() { K = s1 = s2 = f32x4{0.f, 0.f, 0.f, 0.f}; n = 0.f; }
    __device__ __forceinline__ void add(f32x4 v) {
        if (n == 0.f) K = v;
        const f32x4 d = v - K;
        s1 += d; s2 += d * d; n += 1.f;
    }
};

__device__ __forceinline__ void chan_merge(float &na, float &ma, float &Ma, float nb, float mb, float Mb) {
    const float n = na + nb, f = n > 0.f ? nb / n : 0.f, d = mb - ma;      // nb == 0 or both empty: nothing moves
    ma += d * f;
    Ma += Mb + d * d * (na * f);
    na = n;
}

struct StatRun {                         // a thread's running (count, mean, M2) of its frame quad: 9 registers
    f32x4 mean, M2;
    float n;
    __device__ __forceinline__ void init() { mean = M2 = f32x4{0.f, 0.f, 0.f, 0.f}; n = 0.f; }
    __device__ __forceinline__ void merge(float nb, f32x4 mb, f32x4 Mb) {
        float nn = n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = mean[r], M = M2[r];
            nn = n;
            chan_merge(nn, m, M, nb, mb[r], Mb[r]);
            mean[r] = m; M2[r] = M;
        }
        n = nn;
    }
    __device__ __forceinline__ void merge(const StatAcc &a) {
        if (a.n == 0.f) return;
        const float inv = 1.0f / a.n;
        f32x4 m, M;
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[r] = a.K[r] + a.s1[r] * inv; M[r] = fmaxf(a.s2[r] - a.s1[r] * a.s1[r] * inv, 0.f); }
        merge(a.n, m, M);
    }
};

// All 256 threads call this (tid & 3 is the thread's frame quad); `red` = 144 floats of LDS nobody else is using any
// more.  Lanes with the same frame quad are merged with wave shuffles (4 steps), the four waves through LDS.  Writes
// slot `part` of the tile; `zero_other` also clears the other slot (single-workgroup tiles).
__device__ __forceinline__ void stat_reduce_store(StatRun a, float *red, float *__restrict__ dst, int tile, int part, bool zero_other) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) {
        f32x4 mb, Mb;
        const float nb = __shfl_xor(a.n, off);
#pragma unroll
        for (int r = 0; r < 4; ++r) { mb[r] = __shfl_xor(a.mean[r], off); Mb[r] = __shfl_xor(a.M2[r], off); }
        a.merge(nb, mb, Mb);
    }
    if (lane < 4) {
        float *o = red + (wave * 4 + lane) * 9;
        o[0] = a.n;
#pragma unroll
        for (int r = 0; r < 4; ++r) { o[1 + r] = a.mean[r]; o[5 + r] = a.M2[r]; }
    }
    __syncthreads();
    if (tid < 16) {
        const int tq = tid >> 2, r = tid & 3;
        float n = 0.f, m = 0.f, M = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) chan_merge(n, m, M, red[(w * 4 + tq) * 9], red[(w * 4 + tq) * 9 + 1 + r], red[(w * 4 + tq) * 9 + 5 + r]);
        float *o = dst + (((size_t)tile * STAT_PARTS + part) * 16 + tid) * 4;
        o[0] = n; o[1] = m; o[2] = M; o[3] = 0.f;
        if (zero_other) { float *z = dst + (((size_t)tile * STAT_PARTS + (part ^ 1)) * 16 + tid) * 4; z[0] = z[1] = z[2] = z[3] = 0.f; }
    }
    __syncthreads();
}

// stats[tile][16][2] = (mean, 1/(unbiased std + 1e-6)) of the concatenation of the tensors whose partials are given
__global__ void stats_merge_kernel(const float *__restrict__ pa, const float *__restrict__ pb, int tiles, float *__restrict__ stats) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tiles * 16) return;
    const int tile = idx >> 4, fr = idx & 15;
    float n = 0.f, m = 0.f, M = 0.f;
    for (int s2 = 0; s2 < 2; ++s2) {
        const float *src = s2 ? pb : pa;
        if (!src) continue;
        for (int part = 0; part < STAT_PARTS; ++part) {
            const float *o = src + (((size_t)tile * STAT_PARTS + part) * 16 + fr) * 4;
            chan_merge(n, m, M, o[0], o[1], o[2]);
        }
    }
    stats[(size_t)idx * 2] = m;
    stats[(size_t)idx * 2 + 1] = 1.0f / (sqrtf(M / (n - 1.f)) + 1e-6f);
}

struct LN {              // LayerNorm applied on the fly to an input view: (x - mean) * inv * w[c][f] + b[c][f]
    const float *stats, *w, *b;        // stats NULL = identity
};

__device__ __forceinline__ float ln_apply(const LN &ln, int tile, int t, int cf, float x) {
    const float mean = ln.stats[((size_t)tile * 16 + t) * 2], inv = ln.stats[((size_t)tile * 16 + t) * 2 + 1];
    return (x - mean) * inv * ln.w[cf] + ln.b[cf];
}

__device__ __forceinline__ float ln_apply2(const LN &ln, float mean, float inv, int cf, float x) {
    return (x - mean) * inv * ln.w[cf] + ln.b[cf];
}

// ---------------------------------------------------------------------------------------------
// pw_conv: convolution over channels with KF (1 or 3) taps along F ('same' zero padding), per frame.
//   rows = output channels (MT tiles of 16, zero padded), K = KF * C_in (KS k-steps of 4), cols = frames.
//   Weights W[MT*16][KF*C_in] are loaded once per wave into VGPRs; each wave walks the bins.
// MODE 0: out0 = act(conv(in) + b)                       act: 0 none, 1 sigmoid
// MODE 1: CFB front (:87-90): g = sigmoid(convG(LN(in)) + bg); xi = convI(in) + bi;
//                             out0 = g*xi; out1 = xi - g*xi
// MODE 2: CFB back  (:91-92): out0 = conv31(LN(in)) + b + add
// `in` is the channel concatenation of views a and b.
// ---------------------------------------------------------------------------------------------
struct PwArgs {
    View a, b;
    LN ln;
    const float *W, *bias;             // MODE 1: gate weights / bias
    const float *W2, *bias2;           // MODE 1: input-conv weights / bias
    View add;                          // MODE 2
    ViewW out0, out1;
    float *part0, *part1;              // optional partial statistics of out0 / out1 (see StatAcc)
    int F, co, act;
    int fc, nchunk;                    // bins per workgroup chunk, chunks per tile
};

// Shape of one pw_conv instantiation.  Everything that indexes memory is a compile-time constant: the kernel was first
// written against run-time (cin, co, fc) and spent 12.7 VALU instructions per MFMA -- 60 per staged 16-B item, 125 per
// written item, mostly signed run-time divisions, 64-bit address arithmetic and per-row predication -- i.e. the SIMDs'
// issue slots, not HBM, were what the 3.2 TB/s it reached was bound by (profiles/r02_dfsmn: SQ_INSTS_VALU 131 G against
// 10.3 G MFMAs for the (3,1) conv).
template <int CO, int CIN, int KF, int MODE>
struct PwShape {
    static constexpr int MT = (CO + 15) / 16, K = KF * CIN, KS = K / 4, HALO = (KF - 1) / 2, NOUT = MODE == 1 ? 2 : 1;
    static constexpr int lds_floats(int fc) { return CIN * ((fc + 2 * HALO) | 1) * 18 + NOUT * CO * fc * 16; }
    // bins per chunk: the largest multiple of 4 (one bin per wave per round) up to 32 that keeps the workgroup's LDS
    // within 52 KB (three workgroups per CU).  (Smaller chunks for more workgroups per CU were measured -- LDS caps of
    // 40 / 26 / 16 KB: pw_conv 80 -> 94 / 105 / 111 ms per 1920 windows: shorter contiguous runs per channel and more
    // halo rows cost more than the occupancy buys.)
    static constexpr int pick_fc() { int fc = 32; while (fc > 4 && lds_floats(fc) * 4 > 52 * 1024) fc -= 4; return fc; }
    static constexpr int FC = pick_fc(), FH = FC + 2 * HALO, FS = FH | 1;      // bins, staged rows per channel, their (odd) LDS pitch
    static constexpr int LDS_FLOATS = lds_floats(FC);
    static_assert(K % 4 == 0, "kf * cin must be a multiple of 4");
};

// A workgroup owns (tile, chunk of FC bins); it stages the chunk's input rows (+1 halo bin each side for the (3,1)
// conv) into LDS with 16-B coalesced loads -- a channel's bins are contiguous in the FT layout, so every run is
// FH*64 B -- together with the LayerNorm weight/bias of each (channel, bin); the MFMA loop reads its B operand
// from LDS (row stride FS*16 floats with FS odd: the four k-quarters land 16 banks apart), results go to an LDS
// output block and leave as 16-B coalesced stores (+ the residual `add` of MODE 2, read the same way).
template <int CO, int CIN, int KF, int MODE>
__global__ __launch_bounds__(256, 3) void pw_conv_kernel(PwArgs p) {
    using S = PwShape<CO, CIN, KF, MODE>;
    constexpr int MT = S::MT, KS = S::KS, K = S::K, HALO = S::HALO, FC = S::FC, FH = S::FH, FS = S::FS;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, i = lane & 15, tq = tid & 3, rg = tid >> 2;
    // LayerNorm: MODE 0 has none; MODE 2 consumes only LN(in), applied while staging; MODE 1 needs the raw rows too
    // (input conv) and normalises on the fly with the per-row (weight, bias) pairs staged next to them
    constexpr bool LN_STAGE = MODE == 2, LN_FLY = MODE == 1;
    float *raw = lds;                                   // [CIN][FS][16]
    float *wb = raw + CIN * FS * 16;                    // [CIN][FS][2]   MODE 1: LayerNorm (weight, bias); (0, 0) outside [0, F)
    float *o0 = wb + CIN * FS * 2;                      // [CO][FC][16]
    float *o1 = o0 + CO * FC * 16;                      // MODE 1 only

    // weights stay in VGPRs for every chunk of the tile
    float wa[MT][KS], wg[MODE == 1 ? MT : 1][MODE == 1 ? KS : 1];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            wa[mt][s] = p.W[(mt * 16 + i) * K + 4 * s + q];
            if (MODE == 1) wg[mt][s] = p.W2[(mt * 16 + i) * K + 4 * s + q];
        }
    // (a persistent variant -- one resident wave of workgroups walking the tiles with their weights kept -- was slower
    // here, 1.30 -> 1.54 ms: the per-workgroup set-up is small and the hoisted per-tile state costs occupancy)
    const int tile = blockIdx.x, F = p.F;
    float ln_mean = 0.f, ln_inv = 1.f;                  // MODE 1: this lane's frame (column i) is fixed
    f32x4 st_mean = {0.f, 0.f, 0.f, 0.f}, st_inv = {1.f, 1.f, 1.f, 1.f};      // MODE 2: the staging thread's frame quad
    if (LN_FLY) { ln_mean = p.ln.stats[(tile * 16 + i) * 2]; ln_inv = p.ln.stats[(tile * 16 + i) * 2 + 1]; }
    if (LN_STAGE)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            st_mean[r] = p.ln.stats[(tile * 16 + 4 * tq + r) * 2];
            st_inv[r] = p.ln.stats[(tile * 16 + 4 * tq + r) * 2 + 1];
        }
    // this lane's k rows: k = 4s + q -> (tap, channel) = (s / (CIN/4), 4 (s % (CIN/4)) + q) as CIN % 4 == 0 -> LDS row
    // (channel*FS + tap): ONE address register (k-step 0, bin `wave` of round 0); k-steps, rounds are compile-time offsets
    static_assert(CIN % 4 == 0, "a k-step of four channels must not straddle two taps");
    const int kaddr0 = (q * FS + wave) * 16 + i;
    auto koffs = [](int s) constexpr { return (4 * (s % (CIN / 4)) * FS + s / (CIN / 4)) * 16; };
    float bias_r[MT][4], bias2_r[MODE == 1 ? MT : 1][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = min(mt * 16 + 4 * q + r, CO - 1);
            bias_r[mt][r] = p.bias[co];
            if (MODE == 1) bias2_r[mt][r] = p.bias2[co];
        }
    // per-thread global bases of the tile (the in-tile offsets below are 32-bit): view b is addressed with channel c - a.c
    const int ac = p.a.c;
    const float *abase = p.a.ptr + ((size_t)tile * p.a.c_total + p.a.c_off) * F * 16 + 4 * tq;
    const float *bbase = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(p.b.ptr) +
                             (((size_t)tile * p.b.c_total + p.b.c_off) * F * 16 + 4 * tq) * sizeof(float) - (size_t)ac * F * 16 * sizeof(float));
    float *obase0 = p.out0.ptr + ((size_t)tile * p.out0.c_total + p.out0.c_off) * F * 16 + 4 * tq;
    float *obase1 = MODE == 1 ? p.out1.ptr + ((size_t)tile * p.out1.c_total + p.out1.c_off) * F * 16 + 4 * tq : nullptr;
    const float *addbase = MODE == 2 ? p.add.ptr + ((size_t)tile * p.add.c_total + p.add.c_off) * F * 16 + 4 * tq : nullptr;

    StatRun run0, run1;
    run0.init(); run1.init();
    for (int chunk = blockIdx.y; chunk < p.nchunk; chunk += gridDim.y) {
        const int f0 = chunk * FC, fcv = min(FC, F - f0);
        // the row -> (channel, bin) maps below do not depend on the chunk; left visible, the compiler hoists all of them
        // out of this loop and spills (the kernel has 168 VGPRs at three workgroups per CU)
        int rgc = rg;
        asm volatile("" : "+v"(rgc));
        // ---- stage the input rows: thread = (row (c, ffl), frame quad), rows rg + 64 j; four unconditional (clamped) loads
        // in flight per thread, then the stores -- a load-store pair per iteration is one serialised round trip each.
        // (One batch of six loads per thread -- the whole chunk in a single round trip -- was measured: pw_conv 80 -> 90 ms per
        // 1920 windows; the extra live registers cost the third workgroup per CU.)
        {
            constexpr int NROW = CIN * FH, NIT = (NROW + 63) / 64;
#pragma unroll
            for (int j0 = 0; j0 < NIT; j0 += 4) {
                f32x4 v[4];
                float w[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < NIT) {
                        const int rowi = (j0 + u + 1) * 64 <= NROW ? rgc + 64 * (j0 + u) : min(rgc + 64 * (j0 + u), NROW - 1);
                        const int c = rowi / FH, ffl = rowi - c * FH, ff = f0 - HALO + ffl;
                        const int cf = c * F + max(0, min(ff, F - 1));
                        v[u] = *reinterpret_cast<const f32x4 *>((c < ac ? abase : bbase) + cf * 16);
                        if (LN_STAGE) { w[u] = p.ln.w[cf]; b[u] = p.ln.b[cf]; }
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < NIT) {
                        const int rowi = rgc + 64 * (j0 + u);
                        if ((j0 + u + 1) * 64 <= NROW || rowi < NROW) {
                            const int c = rowi / FH, ffl = rowi - c * FH, ff = f0 - HALO + ffl;
                            f32x4 x = v[u];
                            if (LN_STAGE) x = (x - st_mean) * st_inv * w[u] + b[u];
                            if (HALO && (ff < 0 || ff >= F)) x = f32x4{0.f, 0.f, 0.f, 0.f};
                            *reinterpret_cast<f32x4 *>(raw + (c * FS + ffl) * 16 + 4 * tq) = x;
                        }
                    }
            }
        }
        if (LN_FLY) {                                           // (weight, bias) per staged row: unconditional clamped loads
            constexpr int NROW = CIN * FH, NIT = (NROW + 255) / 256;
            float w[NIT], b[NIT];
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                const int rowi = min(tid + 256 * u, NROW - 1), c = rowi / FH, ffl = rowi - c * FH;
                const int cf = c * F + min(f0 + ffl, F - 1);
                w[u] = p.ln.w[cf]; b[u] = p.ln.b[cf];
            }
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                const int rowi = tid + 256 * u;
                if (rowi < NROW) {
                    const int c = rowi / FH, ffl = rowi - c * FH;
                    *reinterpret_cast<float2 *>(wb + 2 * (c * FS + ffl)) = f0 + ffl < F ? float2{w[u], b[u]} : float2{0.f, 0.f};
                }
            }
        }
        __syncthreads();

        // ---- MFMA: wave walks the chunk's bins (bin = wave + 4 * round; the loop is unrolled so that every LDS address is
        // one operand / output base register plus a compile-time offset).  The operands of a bin are fetched as one batch of
        // independent LDS reads (left alone the compiler emits read -> wait -> LayerNorm -> wait -> 2 MFMAs per k-step: two
        // exposed LDS round trips each); MODE 0 / 2 also request the next bin's batch before this bin's MFMAs issue.
        {
            float xc[KS], xn[LN_FLY ? 1 : KS];
            float2 wbc[LN_FLY ? KS : 1];
            const int wbaddr0 = 2 * (q * FS + wave);          // MODE 1 (KF = 1): row 4s + q, bin `wave`
            const int obase = ((4 * q) * FC + wave) * 16 + i;   // row 4q (+ 16 mt + r), bin `wave` (+ 4 round)
            if constexpr (!LN_FLY) {
                if (wave < fcv) {
#pragma unroll
                    for (int s = 0; s < KS; ++s) xc[s] = raw[kaddr0 + koffs(s)];
                }
            }
#pragma unroll
            for (int rd = 0; rd < FC / 4; ++rd) {
                const int fl = wave + 4 * rd;
                if (fl < fcv) {
                    if constexpr (LN_FLY) {
#pragma unroll
                        for (int s = 0; s < KS; ++s) { xc[s] = raw[kaddr0 + koffs(s) + rd * 64]; wbc[s] = *reinterpret_cast<const float2 *>(wb + wbaddr0 + 8 * s * FS + rd * 8); }
                    } else if (rd + 1 < FC / 4) {
                        if (fl + 4 < fcv) {
#pragma unroll
                            for (int s = 0; s < KS; ++s) xn[s] = raw[kaddr0 + koffs(s) + (rd + 1) * 64];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 acc[MT], acc2[MODE == 1 ? MT : 1];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) { acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f}; if (MODE == 1) acc2[mt] = acc[mt]; }
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const float x = xc[s];
                        float lnv = x;
                        if constexpr (LN_FLY) lnv = (x - ln_mean) * ln_inv * wbc[s].x + wbc[s].y;
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            acc[mt] = mfma16(wa[mt][s], lnv, acc[mt]);
                            if (MODE == 1) acc2[mt] = mfma16(wg[mt][s], x, acc2[mt]);
                        }
                    }
                    if constexpr (!LN_FLY) {
#pragma unroll
                        for (int s = 0; s < KS; ++s) xc[s] = xn[s];
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        if ((mt + 1) * 16 <= CO || mt * 16 + 4 * q < CO) {          // a lane's four rows are valid together (CO % 4 == 0) ...
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (CO % 4 == 0 || (mt + 1) * 16 <= CO || mt * 16 + 4 * q + r < CO) {      // ... or checked one by one
                                    const float v = acc[mt][r] + bias_r[mt][r];
                                    const int o = obase + ((mt * 16 + r) * FC + 4 * rd) * 16;
                                    if (MODE == 0) {
                                        o0[o] = p.act == 1 ? gate_sigmoid(v) : v;
                                    } else if (MODE == 1) {
                                        const float g = gate_sigmoid(v), xi = acc2[mt][r] + bias2_r[mt][r], gx = g * xi;
                                        o0[o] = gx;
                                        o1[o] = xi - gx;
                                    } else {
                                        o0[o] = v;
                                    }
                                }
                        }
                }
            }
        }
        __syncthreads();

        // ---- coalesced write-out: thread = (row (co, fl), frame quad), rows rg + 64 j over the [CO][FC] block (bins past a
        // short last chunk are skipped); the residual `add` rows of a batch are requested together before the stores
        {
            StatAcc st0, st1;
            st0.init(); st1.init();
            constexpr int NROW = CO * FC, NIT = (NROW + 63) / 64;
            const int f016 = f0 * 16;
#pragma unroll
            for (int j0 = 0; j0 < NIT; j0 += 4) {
                f32x4 av[4];
                if (MODE == 2) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (j0 + u < NIT) {
                            const int rowi = (j0 + u + 1) * 64 <= NROW ? rgc + 64 * (j0 + u) : min(rgc + 64 * (j0 + u), NROW - 1);
                            const int co = rowi / FC, fl = min(rowi - co * FC, fcv - 1);
                            av[u] = *reinterpret_cast<const f32x4 *>(addbase + f016 + (co * F + fl) * 16);
                        }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < NIT) {
                        const int rowi = rgc + 64 * (j0 + u), co = rowi / FC, fl = rowi - co * FC;
                        if (((j0 + u + 1) * 64 <= NROW || rowi < NROW) && fl < fcv) {
                            f32x4 v = *reinterpret_cast<const f32x4 *>(o0 + rowi * 16 + 4 * tq);
                            if (MODE == 2) v += av[u];
                            *reinterpret_cast<f32x4 *>(obase0 + f016 + (co * F + fl) * 16) = v;
                            if (p.part0) st0.add(v);
                            if (MODE == 1) {
                                const f32x4 v1 = *reinterpret_cast<const f32x4 *>(o1 + rowi * 16 + 4 * tq);
                                *reinterpret_cast<f32x4 *>(obase1 + f016 + (co * F + fl) * 16) = v1;
                                if (p.part1) st1.add(v1);
                            }
                        }
                    }
            }
            if (p.part0) run0.merge(st0);
            if (MODE == 1 && p.part1) run1.merge(st1);
        }
        // the next chunk's staging writes raw/wb (last read before the barrier above); o0/o1 are rewritten only after
        // the next chunk's first barrier, i.e. after every thread has finished this write-out
    }
    if (p.part0 || p.part1) {
        __syncthreads();                                   // the last write-out is done with the LDS
        if (p.part0) stat_reduce_store(run0, lds, p.part0, tile, blockIdx.y, gridDim.y == 1);
        if (MODE == 1 && p.part1) stat_reduce_store(run1, lds, p.part1, tile, blockIdx.y, gridDim.y == 1);
    }
}

// ---------------------------------------------------------------------------------------------
// dft_f: GEMM along the frequency axis, per channel:  out[c][m][t] = sum_k Tbl[m][k] * B_c[k][t]
//   FWD (CepsUnit :134-138): B_c = LN2(in)[c][f] (k = f, 160);  rows m = (cos k' = 0..80 | sin k' = 1..79): the sine rows of
//        bins 0 and 80 are identically zero, so the 162 outputs are 160 table rows = TEN tiles of 16 (they were padded to
//        96 + 96 = twelve); out channel c <- cos rows, C + c <- sin rows (bins 0 and 80 written as zeros), Fout = 81.
//   INV (:141-153): k = (re k' = 0..80 | im k' = 1..79) (160: the pseudo-inverse has zero columns for the two vanishing imaginary
//        parts; the host checks that); B_c = complex product of the LSTM output (pr, pi) = lo[c], lo[C+c] with the raw
//        spectrum (re, im) = li[c], li[C+c]; rows m = f (160).
// Table rows live in VGPRs.  Four waves (one per SIMD) own 3 + 3 + 2 + 2 row tiles; two workgroups share a CU and the dispatcher
// rotates their starting SIMD, so a SIMD carries at most six and typically five tiles per channel pair where the padded layout
// cost six always.  The channel's B matrix is staged through LDS.
// ---------------------------------------------------------------------------------------------
struct DftArgs {
    View in;             // FWD: r (C ch, F=160).  INV: li (2C ch, F=81)
    View lo;             // INV only: LSTM+linear output (2C ch, F=81)
    LN ln;               // FWD only
    const float *tbl;    // [160][160] row-major
    ViewW out;           // FWD: li (2C ch, 81).  INV: ceps_out (C ch, 160)
    float *part;         // FWD, optional: partial statistics of out (slot 0; slot 1 cleared)
    int C, tiles;
};

constexpr int DFT_K = 160, DFT_KS = DFT_K / 4, DFT_ROWS = 160, DFT_NT = 256;

// Memory path: channel c+1's rows are requested as 16-B coalesced loads before channel c's MFMAs issue and parked in
// the other half of the LDS double buffer afterwards; results leave through a (double-buffered) LDS output block as
// 16-B coalesced stores -- an output channel's bins are contiguous in the FT layout.
// RT = this wave's number of row tiles, rt0 = its first one (the two instantiations meet at the same barriers).
template <bool INV, int RT>
__device__ __forceinline__ void dft_f_body(const DftArgs &p, const int rt0, float (*Bs)[DFT_K * 16], float (*Os)[DFT_ROWS * 16]) {
    constexpr int KS = DFT_KS, NT = DFT_NT;
    constexpr int ITEMS = INV ? 81 * 4 : 160 * 4, NR = (ITEMS + NT - 1) / NT;      // staging work items (row, frame quad)
    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, i = lane & 15;
    float ta[RT][KS];                                       // loaded once: the workgroup walks tiles blockIdx.x, + gridDim.x, ...
#pragma unroll
    for (int h = 0; h < RT; ++h)
#pragma unroll
        for (int s = 0; s < KS; ++s) ta[h][s] = p.tbl[((rt0 + h) * 16 + i) * DFT_K + 4 * s + q];
    const int tq = tid & 3;                                 // NT is a multiple of 4: a thread's frame quad is fixed
    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    f32x4 ln_mean = {0.f, 0.f, 0.f, 0.f}, ln_inv = {1.f, 1.f, 1.f, 1.f};
    if (!INV)                        // the forward direction always normalises (LN2; the launcher requires it)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ln_mean[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2];
            ln_inv[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2 + 1];
        }
    f32x4 pre[NR][INV ? 4 : 1];
    float lw[NR], lb[NR];
    // every load is unconditional (the item index is clamped; surplus lanes re-read the last row): a load under a
    // condition costs a branch and a full wait, i.e. one serialised memory round trip per item
    auto request = [&](int c) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int e = min(tid + NT * r, ITEMS - 1), k = e >> 2;
            if (!INV) {
                pre[r][0] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + c, 160, k) + 4 * tq);
                lw[r] = p.ln.w[c * 160 + k];
                lb[r] = p.ln.b[c * 160 + k];
            } else {
                pre[r][0] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + c, 81, k) + 4 * tq);
                pre[r][1] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + p.C + c, 81, k) + 4 * tq);
                pre[r][2] = *reinterpret_cast<const f32x4 *>(p.lo.ptr + ft_idx(tile, p.lo.c_total, p.lo.c_off + c, 81, k) + 4 * tq);
                pre[r][3] = *reinterpret_cast<const f32x4 *>(p.lo.ptr + ft_idx(tile, p.lo.c_total, p.lo.c_off + p.C + c, 81, k) + 4 * tq);
            }
        }
    };
    auto park = [&](float *dst) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int e = tid + NT * r, k = e >> 2;
            if (e >= ITEMS) continue;
            if (!INV) {
                *reinterpret_cast<f32x4 *>(dst + k * 16 + 4 * tq) = (pre[r][0] - ln_mean) * ln_inv * lw[r] + lb[r];
            } else {
                const f32x4 re = pre[r][0], im = pre[r][1], pr = pre[r][2], pi = pre[r][3];
                *reinterpret_cast<f32x4 *>(dst + k * 16 + 4 * tq) = pr * re - pi * im;
                if (k >= 1 && k <= 79) *reinterpret_cast<f32x4 *>(dst + (80 + k) * 16 + 4 * tq) = pr * im + pi * re;
            }
        }
    };
    StatRun run;
    run.init();
    request(0);
    park(Bs[0]);
    __syncthreads();
    for (int c = 0; c < p.C; ++c) {
        const float *B = Bs[c & 1];
        float *O = Os[c & 1];
        if (c + 1 < p.C) request(c + 1);
        f32x4 acc[RT];
#pragma unroll
        for (int h = 0; h < RT; ++h) acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the B column is read KB k-steps at a time, the next batch requested before this batch's MFMAs issue (left to
        // itself the compiler emits read -> wait -> 2 MFMAs: one exposed LDS round trip per k-step)
        constexpr int KB = 8;
        float bcur[KB], bnxt[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) bcur[u] = B[(4 * u + q) * 16 + i];
#pragma unroll
        for (int s0 = 0; s0 < KS; s0 += KB) {
#pragma unroll
            for (int u = 0; u < KB; ++u) bnxt[u] = B[(4 * min(s0 + KB + u, KS - 1) + q) * 16 + i];
            __builtin_amdgcn_sched_barrier(0);           // keep the reads above the MFMAs (the scheduler sinks them back)
#pragma unroll
            for (int u = 0; u < KB; ++u)
                if (s0 + u < KS) {
#pragma unroll
                    for (int h = 0; h < RT; ++h) acc[h] = mfma16(ta[h][s0 + u], bcur[u], acc[h]);
                }
#pragma unroll
            for (int u = 0; u < KB; ++u) bcur[u] = bnxt[u];
        }
#pragma unroll
        for (int h = 0; h < RT; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) O[((rt0 + h) * 16 + 4 * q + r) * 16 + i] = acc[h][r];
        if (c + 1 < p.C) park(Bs[(c + 1) & 1]);
        __syncthreads();
        // copy-out of channel c (reads O; O is next written two channels later, after the next barrier)
        if (!INV) {          // rows 0..80 = cos bins -> channel c; rows 81..159 = sin bins 1..79 -> channel C + c, whose bins 0, 80 are zero
            StatAcc st;
            st.init();
            for (int e = tid; e < 2 * 81 * 4; e += NT) {
                const int half = e >= 81 * 4, rowq = e - half * 81 * 4, kk = rowq >> 2, oq = rowq & 3;      // oq == tid & 3
                const bool zero = half && (kk == 0 || kk == 80);
                f32x4 v = *reinterpret_cast<const f32x4 *>(O + (zero ? 0 : half * 80 + kk) * 16 + 4 * oq);
                if (zero) v = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4 *>(p.out.ptr + ft_idx(tile, p.out.c_total, p.out.c_off + (half ? p.C + c : c), 81, kk) + 4 * oq) = v;
                if (p.part) st.add(v);
            }
            if (p.part) run.merge(st);
        } else {
            for (int e = tid; e < 160 * 4; e += NT)
                *reinterpret_cast<f32x4 *>(p.out.ptr + ft_idx(tile, p.out.c_total, p.out.c_off + c, 160, e >> 2) + 4 * (e & 3)) =
                    *reinterpret_cast<const f32x4 *>(O + (e >> 2) * 16 + 4 * (e & 3));
        }
    }
    if (!INV && p.part) {
        __syncthreads();                                   // the last copy-out is done with Os
        stat_reduce_store(run, &Os[0][0], p.part, tile, 0, true);
    }
    __syncthreads();                                        // Bs / Os are free for the next tile
    }
}

// bit mask of the two waves that own three row tiles: 0 and 2 measured best (fwd 1.30 ms; {0,1} 1.39, {0,3} 1.40, {1,2} 1.41)
constexpr int DFT_HEAVY = 0x5;
template <bool INV>
__global__ __launch_bounds__(DFT_NT, 2) void dft_f_kernel(DftArgs p) {
    __shared__ __attribute__((aligned(16))) float Bs[2][DFT_K * 16];
    __shared__ __attribute__((aligned(16))) float Os[2][DFT_ROWS * 16];
    const int wave = threadIdx.x >> 6;
    const bool heavy = (DFT_HEAVY >> wave) & 1;
    const int rank = __builtin_popcount((heavy ? DFT_HEAVY : ~DFT_HEAVY & 0xf) & ((1 << wave) - 1));     // 0 or 1 among its kind
    if (heavy) dft_f_body<INV, 3>(p, 3 * rank, Bs, Os);
    else dft_f_body<INV, 2>(p, 6 + 2 * rank, Bs, Os);
}

// ---------------------------------------------------------------------------------------------
// lstm_f: bidirectional LSTM (hidden 20) ALONG the frequency axis, batch = the tile's 16 frames
// (CH_LSTM_F :270-284: in_ch_lstm IN=4 F=160; CepsUnit IN=40 F=81 with LayerNorm on the input).
// One wave per direction.  Gate rows are ordered so that m-tile mt, fragment row 4q+r holds gate r of
// hidden unit 4*mt+q: the cell update is lane-local and the new h IS the next step's B fragment.
// Output channels: [0,20) forward h, [20,40) backward h.
// ---------------------------------------------------------------------------------------------
struct LstmFArgs {
    View in;
    LN ln;
    const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2];      // per direction, torch layouts [80][IN], [80][20], [80]
    ViewW out;           // 40 channels
    int F;
};

// Input path: the recurrence consumes one bin (IN rows of 64 B) per step, far too little to cover HBM latency with
// per-step loads, so each wave streams CHUNKS of NB bins: all rows of a chunk are requested as 16-B coalesced loads
// (5 per lane for IN = 40, together with their LayerNorm weight / bias) two chunks ahead, then LayerNorm'd and parked
// in the wave's private LDS double buffer, from where the MFMA B operand is read ([row][16 frames]: the k-quarters
// land 16 banks apart).  Waves never share LDS data, so no workgroup barrier is needed.  NB = 2 for IN = 40: 20 KB per
// workgroup, so the four workgroups (two waves per SIMD) that the registers allow also fit the LDS -- with NB = 4 the
// 40 KB x 4 = 160 KB did not, and a third of the wave slots stayed empty.
template <int IN>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void lstm_f_kernel(LstmFArgs p) {
    constexpr int KI = IN / 4, H = 20, MT = 5, NB = IN == 40 ? 2 : 4;
    constexpr int CH_FLOATS = NB * IN * 16, NLD = NB * IN / 16;      // floats per chunk; float4 loads per lane per chunk
    __shared__ __attribute__((aligned(16))) float xs[2][2][CH_FLOATS];      // [direction][buffer]
    const int tile = blockIdx.x, lane = threadIdx.x & 63, dir = threadIdx.x >> 6, q = lane >> 4, i = lane & 15;
    const int grow = (i & 3) * H + (i >> 2);          // A-fragment row i <-> gate (i&3), unit-in-quad (i>>2)
    float wi[MT][KI], wh[MT][MT], bias[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = grow + 4 * mt;
#pragma unroll
        for (int s = 0; s < KI; ++s) wi[mt][s] = p.w_ih[dir][(size_t)row * IN + 4 * s + q];
#pragma unroll
        for (int s = 0; s < MT; ++s) wh[mt][s] = p.w_hh[dir][(size_t)row * H + 4 * s + q];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[mt][r] = p.b_ih[dir][r * H + 4 * mt + q] + p.b_hh[dir][r * H + 4 * mt + q];
    }
    float h[MT], c[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { h[mt] = 0.f; c[mt] = 0.f; }
    // staging role of this lane: float4 number e = lane + 64 r of the chunk -> row e/4 = (bin b, channel ch), frames 4 (lane&3)..+3
    const int tq = lane & 3;
    f32x4 ln_mean = {0.f, 0.f, 0.f, 0.f}, ln_inv = {1.f, 1.f, 1.f, 1.f};
    if (IN == 40)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ln_mean[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2];
            ln_inv[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2 + 1];
        }
    const int nchunk = (p.F + NB - 1) / NB;
    auto bin_of = [&](int ck, int b) { const int st = ck * NB + b; return dir ? p.F - 1 - st : st; };      // may run past the end
    constexpr bool HAS_LN = IN == 40;                 // CepsUnit normalises its LSTM input, in_ch_lstm does not (launcher checks)
    f32x4 pre[NLD];
    float lw[HAS_LN ? NLD : 1], lb[HAS_LN ? NLD : 1];   // LayerNorm (weight, bias) of the requested rows
    auto request = [&](int ck) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int row = (lane >> 2) + 16 * r, b = row / IN, ch = row - b * IN, f = bin_of(ck, b);
            pre[r] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int fcl = f < 0 ? 0 : (f >= p.F ? p.F - 1 : f);        // unconditional (clamped) loads; bins past the end are never used
            pre[r] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + ch, p.F, fcl) + 4 * tq);
            if constexpr (HAS_LN) { lw[r] = p.ln.w[ch * p.F + fcl]; lb[r] = p.ln.b[ch * p.F + fcl]; }
        }
    };
    auto park = [&](float *dst) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            f32x4 v = pre[r];
            if constexpr (HAS_LN) v = (v - ln_mean) * ln_inv * lw[r] + lb[r];
            *reinterpret_cast<f32x4 *>(dst + ((lane >> 2) + 16 * r) * 16 + 4 * tq) = v;
        }
    };
    // (Requests arranged so that every one covers a whole, aligned 128-B line -- F = 81 is odd, so for every other channel the two
    // bins of a chunk straddle two lines -- were built and change nothing (2.04 vs 2.05 ms): the rocprofv3 FETCH_SIZE of this
    // kernel equals the tensor's bytes UNdoubled, i.e. 64-B requests are tallied at 64 B and there never was an over-fetch.)
    // The step is software-pipelined inside the wave: the input half of step t+1 (W_ih x, 10 k-steps, independent of the
    // recurrence) is issued right after the recurrent half of step t (W_hh h, 5 k-steps), so the matrix pipe works on it
    // while the VALU runs step t's gate non-linearities -- in program order (input half, recurrent half, gates) the
    // pipe idled through the gates and the wave through the MFMAs.  For that the NEXT chunk must already be parked when
    // a chunk's last step runs: chunk ck+1 is parked at the start of chunk ck (its loads were requested a chunk ago).
    auto input_half = [&](const float *xrow, f32x4 (&a)[MT]) {        // a = bias + W_ih x, x = 16 frames of one bin
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = f32x4{bias[mt][0], bias[mt][1], bias[mt][2], bias[mt][3]};
#pragma unroll
        for (int s = 0; s < KI; ++s) {
            const float xv = xrow[(4 * s + q) * 16 + i];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = mfma16(wi[mt][s], xv, a[mt]);
        }
    };
    request(0);
    park(xs[dir][0]);
    if (nchunk > 1) request(1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // this wave's LDS writes precede its reads below
    __builtin_amdgcn_wave_barrier();
    f32x4 accn[MT];
    input_half(xs[dir][0], accn);
    for (int ck = 0; ck < nchunk; ++ck) {
        const float *xb = xs[dir][ck & 1], *xnext = xs[dir][(ck + 1) & 1];
        if (ck + 1 < nchunk) {
            park(xs[dir][(ck + 1) & 1]);                  // the buffer last read by chunk ck - 1
            if (ck + 2 < nchunk) request(ck + 2);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const int f = bin_of(ck, b);
            if (f < 0 || f >= p.F) break;
            // next step's input operands: the next bin of this chunk, or bin 0 of the parked next chunk (after the very last
            // step this reads stale rows of the other buffer; the result is never used)
            const float *xrow = b + 1 < NB ? xb + (b + 1) * IN * 16 : xnext;
            float xv[KI];
#pragma unroll
            for (int s = 0; s < KI; ++s) xv[s] = xrow[(4 * s + q) * 16 + i];
            f32x4 acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = accn[mt];
#pragma unroll
            for (int s = 0; s < MT; ++s)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16(wh[mt][s], h[s], acc[mt]);
            __builtin_amdgcn_sched_barrier(0);
            // The matrix pipe takes 32 cycles per MFMA, during which the wave can issue three to four other instructions.  Left
            // to itself the scheduler emits the next input half as two runs of MFMAs and the gate arithmetic as ~50-instruction
            // stretches with the pipe idle, so the order is pinned here: PIECES slices per hidden-unit quad, each = a few
            // input-half MFMAs of step t+1 + one slice of step t's gate arithmetic, fenced by sched_barriers.
            constexpr int NIN = MT * KI, PIECES = 5, PER = (NIN + MT * PIECES - 1) / (MT * PIECES);
            auto in_mfma = [&](int n) {                         // n-th MFMA of a = bias + W_ih x  (k-step n / MT, row tile n % MT)
                if (n >= NIN) return;
                const int s2 = n / MT, m2 = n % MT;
                if (s2 == 0) accn[m2] = f32x4{bias[m2][0], bias[m2][1], bias[m2][2], bias[m2][3]};
                accn[m2] = mfma16(wi[m2][s2], xv[s2], accn[m2]);
            };
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                int n = mt * PIECES * PER;
#pragma unroll
                for (int u = 0; u < PER; ++u) in_mfma(n++);
                const float ig = gate_sigmoid(acc[mt][0]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PER; ++u) in_mfma(n++);
                const float fg = gate_sigmoid(acc[mt][1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PER; ++u) in_mfma(n++);
                const float gg = gate_tanh(acc[mt][2]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PER; ++u) in_mfma(n++);
                const float og = gate_sigmoid(acc[mt][3]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PER; ++u) in_mfma(n++);
                c[mt] = fg * c[mt] + ig * gg;
                h[mt] = og * gate_tanh(c[mt]);
                p.out.ptr[ft_idx(tile, p.out.c_total, p.out.c_off + dir * H + 4 * mt + q, p.F, f) + i] = h[mt];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------
// lstm_f on split products (csrc/split_scheme.h), CepsUnit geometry (IN = 40, hidden 20): ONE kernel, instantiated for bf16 x 3 and
// fp16 x 2; `if constexpr` on the scheme marks the only parts that differ -- where weight plane 2 lives, the product block, the join of
// its accumulators and the range epilogue.  Described for bf16 x 3 first.  Same decomposition as lstm_f_kernel<40>:
// one wave per direction, gate rows ordered so that the cell update is lane-local, x streamed through the wave's private LDS chunks.
// The step's matrix product is ONE GEMM over the concatenated operand [h (20) ; x (40) ; 1 (bias)] = 61 of the 64 k-slots of two
// 32-k chunks: 5 row tiles x 2 chunks x 6 = 60 v_mfma_f32_16x16x32_bf16 (1020 matrix cycles) instead of 75 v_mfma_f32_16x16x4_f32
// (2400), and the gate arithmetic hides beside the bf16 matrix pipe instead of adding to it.
//   k-slot map (same for the weights' A fragments and the operand's B fragment; lane 16 g + i supplies slots e = 0..7 of group g):
//     chunk 0: e < 5 -> h of unit 4 e + g (the lane's OWN cell outputs: the new h is the next step's operand without any
//              cross-lane traffic, as in the f32 kernel);  e = 5..7 -> x channel 3 g + e - 5
//     chunk 1: x channel 12 + 8 g + e (< 40), channel 40 = the constant 1.0 whose "weight" is b_ih + b_hh, beyond: zero
// Weights are split by each lane at kernel start from the torch layouts (80 loads + splits; the workgroups are persistent over tiles).
// fp16 x 2: both planes of the weights in registers (80 VGPRs, no LDS plane), three v_mfma_f32_16x16x32_f16 per (row tile, chunk) = 30 per
// step instead of 60 bf16, 3 VALU per split value instead of 5.5.  h lies in (-1, 1); the LayerNorm'd inputs and the weights feed the
// range check (vadx_dfsmn_lstm_f's range_flag).
// Both instances sit at 256 VGPRs with a little scratch (as inlined functions of a policy struct the four parts cost fp16 x 2 more of it).
// ---------------------------------------------------------------------------------------------
// eight float32 values (the k-slots of one lane's chunk) -> the planes of its A / B fragment (two bodies: over split4's arrays the callers' code reorders)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&p)[3], float &) {
    u32x2 a0, a1, a2, b0, b1, b2;
    split3x4(f32x4{v[0], v[1], v[2], v[3]}, a0, a1, a2);
    split3x4(f32x4{v[4], v[5], v[6], v[7]}, b0, b1, b2);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    p[0] = __builtin_bit_cast(bf16x8, u32x4{a0[0], a0[1], b0[0], b0[1]});
    p[1] = __builtin_bit_cast(bf16x8, u32x4{a1[0], a1[1], b1[0], b1[1]});
    p[2] = __builtin_bit_cast(bf16x8, u32x4{a2[0], a2[1], b2[0], b2[1]});
}
__device__ __forceinline__ void split8(const float (&v)[8], f16x8 (&p)[2], float &amax) {
    u32x2 a0, a1, b0, b1;
    vadx::split2x4(f32x4{v[0], v[1], v[2], v[3]}, a0, a1, amax);
    vadx::split2x4(f32x4{v[4], v[5], v[6], v[7]}, b0, b1, amax);
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    p[0] = __builtin_bit_cast(f16x8, u32x4{a0[0], a0[1], b0[0], b0[1]});
    p[1] = __builtin_bit_cast(f16x8, u32x4{a1[0], a1[1], b1[0], b1[1]});
}

template <class SC>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void lstm_f_split_kernel(LstmFArgs p, int tiles, unsigned *__restrict__ range_flag) {
    constexpr int IN = 40, H = 20, MT = 5, NB = 2;
    constexpr int CH_FLOATS = NB * IN * 16, NLD = NB * IN / 16;
    constexpr bool W2_IN_LDS = SC::NP == 3;
    __shared__ __attribute__((aligned(16))) float xs[2][2][CH_FLOATS];      // [direction][buffer]
    __shared__ bf16x8 w2s[2][MT][2][64];              // bf16 x 3: plane 2 of the weights (used by one product in six): 20 KB, read back per step
                                                      // (fp16 x 2 never names it, so that instance has no such LDS)
    const int lane = threadIdx.x & 63, dir = threadIdx.x >> 6, q = lane >> 4, i = lane & 15;
    const int grow = (i & 3) * H + (i >> 2);          // A-fragment row i <-> gate (i&3), unit-in-quad (i>>2)
    typename SC::frag wa[MT][2][2];                   // [row tile][chunk][plane 0, 1]: 80 VGPRs, resident for every tile of this workgroup
    float amax = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = grow + 4 * mt;
        float v0[8], v1[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v0[e] = e < 5 ? p.w_hh[dir][(size_t)row * H + 4 * e + q] : p.w_ih[dir][(size_t)row * IN + 3 * q + e - 5];
            const int ch = 12 + 8 * q + e;
            v1[e] = ch < IN ? p.w_ih[dir][(size_t)row * IN + ch] : (ch == IN ? p.b_ih[dir][row] + p.b_hh[dir][row] : 0.f);
        }
        if constexpr (W2_IN_LDS) {
            typename SC::frag t[3];
            split8(v0, t, amax);
            wa[mt][0][0] = t[0]; wa[mt][0][1] = t[1]; w2s[dir][mt][0][lane] = t[2];
            split8(v1, t, amax);
            wa[mt][1][0] = t[0]; wa[mt][1][1] = t[1]; w2s[dir][mt][1][lane] = t[2];
        } else {
            split8(v0, wa[mt][0], amax);
            split8(v1, wa[mt][1], amax);
        }
    }
    if constexpr (W2_IN_LDS) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // the LDS plane is written and read by the same wave only
        __builtin_amdgcn_wave_barrier();
    }
    const int tq = lane & 3;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    float h[MT], c[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { h[mt] = 0.f; c[mt] = 0.f; }
    f32x4 ln_mean, ln_inv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ln_mean[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2];
        ln_inv[r] = p.ln.stats[((size_t)tile * 16 + 4 * tq + r) * 2 + 1];
    }
    const int nchunk = (p.F + NB - 1) / NB;
    auto bin_of = [&](int ck, int b) { const int st = ck * NB + b; return dir ? p.F - 1 - st : st; };
    f32x4 pre[NLD];
    float lw[NLD], lb[NLD];
    auto request = [&](int ck) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int row = (lane >> 2) + 16 * r, b = row / IN, ch = row - b * IN, f = bin_of(ck, b);
            const int fcl = f < 0 ? 0 : (f >= p.F ? p.F - 1 : f);        // unconditional (clamped) loads; bins past the end are never used
            pre[r] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + ch, p.F, fcl) + 4 * tq);
            lw[r] = p.ln.w[ch * p.F + fcl]; lb[r] = p.ln.b[ch * p.F + fcl];
        }
    };
    auto park = [&](float *dst) {
#pragma unroll
        for (int r = 0; r < NLD; ++r)
            *reinterpret_cast<f32x4 *>(dst + ((lane >> 2) + 16 * r) * 16 + 4 * tq) = (pre[r] - ln_mean) * ln_inv * lw[r] + lb[r];
    };
    __builtin_amdgcn_wave_barrier();                  // the previous tile's last reads of xs precede this tile's first park
    request(0);
    park(xs[dir][0]);
    if (nchunk > 1) request(1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int ck = 0; ck < nchunk; ++ck) {
        const float *xb = xs[dir][ck & 1];
        if (ck + 1 < nchunk) {
            park(xs[dir][(ck + 1) & 1]);                  // the buffer last read by chunk ck - 1
            if (ck + 2 < nchunk) request(ck + 2);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const int f = bin_of(ck, b);
            if (f < 0 || f >= p.F) break;
            const float *xrow = xb + b * IN * 16 + i;
            float v0[8], v1[8];
#pragma unroll
            for (int e = 0; e < 5; ++e) v0[e] = h[e];
#pragma unroll
            for (int e = 5; e < 8; ++e) v0[e] = xrow[(3 * q + e - 5) * 16];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ch = 12 + 8 * q + e;               // (q is per-lane: clamp the read, select afterwards)
                const float xv = xrow[(ch < IN ? ch : IN - 1) * 16];
                v1[e] = ch < IN ? xv : (ch == IN ? 1.0f : 0.f);
            }
            typename SC::frag b0[SC::NP], b1[SC::NP];
            split8(v0, b0, amax);
            split8(v1, b1, amax);
            f32x4 acc[MT];                                   // bf16 x 3: every product; fp16 x 2: the leading ones
            [[maybe_unused]] f32x4 mid[MT];                  // fp16 x 2: the cross terms
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (SC::NP == 2) mid[mt] = acc[mt];
            }
            if constexpr (SC::NP == 3) {
                // ONE accumulator per row tile, small products first (at 256 VGPRs the separate accumulator of the small products spilled
                // into the chunk code; measured on its own -- tools/bf16x3_probe.sh "s6" -- the single accumulator is still closer to the float64
                // product than the f32 MFMA chain: 1.4e-7 against 2.5e-7 of sum |w x|).  Row tiles innermost: consecutive MFMAs are independent.
#define LF_TERM(CH, BF, AP, BP) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_bf16(wa[mt][CH][AP], BF[BP], acc[mt]);
#define LF_TERM2(CH, BF) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_bf16(w2s[dir][mt][CH][lane], BF[0], acc[mt]);
                LF_TERM2(0, b0) LF_TERM(0, b0, 1, 1) LF_TERM(0, b0, 0, 2) LF_TERM2(1, b1) LF_TERM(1, b1, 1, 1) LF_TERM(1, b1, 0, 2)
                LF_TERM(0, b0, 1, 0) LF_TERM(0, b0, 0, 1) LF_TERM(1, b1, 1, 0) LF_TERM(1, b1, 0, 1) LF_TERM(0, b0, 0, 0) LF_TERM(1, b1, 0, 0)
#undef LF_TERM
#undef LF_TERM2
            } else {
                // three products per (row tile, chunk): the two cross terms into `mid`, the leading one into `acc`; row tiles innermost so that
                // consecutive MFMAs are independent
#define LF_TERM(ACC, CH, BF, AP, BP) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) ACC[mt] = vadx::mfma_f16(wa[mt][CH][AP], BF[BP], ACC[mt]);
                LF_TERM(mid, 0, b0, 1, 0) LF_TERM(mid, 1, b1, 1, 0) LF_TERM(mid, 0, b0, 0, 1) LF_TERM(mid, 1, b1, 0, 1)
                LF_TERM(acc, 0, b0, 0, 0) LF_TERM(acc, 1, b1, 0, 0)
#undef LF_TERM
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 a = acc[mt];
                if constexpr (SC::NP == 2) a = vadx::join2(acc[mt], mid[mt]);
                const float ig = gate_sigmoid(a[0]), fg = gate_sigmoid(a[1]), gg = gate_tanh(a[2]), og = gate_sigmoid(a[3]);
                c[mt] = fg * c[mt] + ig * gg;
                h[mt] = og * gate_tanh(c[mt]);
                p.out.ptr[ft_idx(tile, p.out.c_total, p.out.c_off + dir * H + 4 * mt + q, p.F, f) + i] = h[mt];
            }
        }
    }
    }
    if constexpr (SC::RANGE_CHECK) vadx::range_flag_raise(range_flag, amax);
}


// ---------------------------------------------------------------------------------------------
// alpha_scale (DFSMN_VAD.forward :326-335): x4 = [mix_re, mix_im, |alpha| * far_re, |alpha| * far_im] with
//   alpha[f][t] = linear2_j( linear1( [pow_far, pow_mix][t-9+j] ) ),  pow = re^2 + im^2, zero history.
// in: FT [4 ch] (mix re, mix im, far re, far im) of NT tiles per chunk; one thread per (tile, f, t16).
// ---------------------------------------------------------------------------------------------
// pow_far != nullptr: the near-end-only model (DFSMN/only_near_end_audio/Export_DFSMN_VAD.py:309-331), whose far-end
// power is a constant [160][frames][10] baked at export (channels 2, 3 of `in` then hold the constant far spectrum).
__global__ void alpha_scale_kernel(const float *__restrict__ in, float *__restrict__ out, int nt, long long total,
                                   const float *__restrict__ w1, const float *__restrict__ b1,
                                   const float *__restrict__ w2, const float *__restrict__ b2,
                                   const float *__restrict__ pow_far, int frames) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int t16 = (int)(e & 15), f = (int)((e >> 4) % 160);
    const int tile = (int)(e / (160 * 16)), chunk = tile / nt, tl = tile - chunk * nt;
    const int t = tl * 16 + t16;
    float alpha = b2[0];
    // the ten history taps' four operands are requested first, unconditionally (time index clamped; taps before the chunk's first
    // frame are zeroed afterwards): loads under `if (tt >= 0)` were ten serialised round trips
    float mr[10], mi[10], fr[10], fi[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const int tt = t - 9 + j, tc = tt < 0 ? 0 : tt;
        const size_t base = ft_idx(chunk * nt + (tc >> 4), 4, 0, 160, f) + (tc & 15);
        mr[j] = in[base]; mi[j] = in[base + 160 * 16]; fr[j] = in[base + 2 * 160 * 16]; fi[j] = in[base + 3 * 160 * 16];
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const int tt = t - 9 + j;
        float pf = 0.f, pm = 0.f;
        if (tt >= 0) {
            pm = mr[j] * mr[j] + mi[j] * mi[j];
            pf = fr[j] * fr[j] + fi[j] * fi[j];
        }
        if (pow_far) pf = pow_far[((size_t)f * frames + (t < frames ? t : frames - 1)) * 10 + j];
        const float a1 = w1[0] * pf + w1[1] * pm + b1[0];
        alpha = fmaf(w2[j], a1, alpha);
    }
    const float sc = fabsf(alpha);
    const size_t o = ft_idx(tile, 4, 0, 160, f) + t16;
    out[o] = in[o];
    out[o + 160 * 16] = in[o + 160 * 16];
    out[o + 2 * 160 * 16] = in[o + 2 * 160 * 16] * sc;
    out[o + 3 * 160 * 16] = in[o + 3 * 160 * 16] * sc;
}

// ---------------------------------------------------------------------------------------------
// ft_repack: move an FT tensor between frame strides.  A 101-frame window on tiles of its own occupies 7 tiles = 112 columns; packed at a
// stride of 104 frames (windows start on alternate halves of a tile) the per-frame kernels -- everything but the two time-axis LSTMs --
// process 6.5 tiles per window: 7 % less work.  Only the 4-channel network input and the 2-channel output are repacked (a fiftieth of
// the traffic of one block); every per-frame op is independent per column, so the padding frames 101..103 of a window never reach a
// valid frame.  Columns beyond `frames` in the source are copied as they are (zeros where the writer zero-filled).
// ---------------------------------------------------------------------------------------------
__global__ void ft_repack_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int F, int frames, int src_stride,
                                 int dst_stride, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // (chunk, c, f, t) with t < min stride, 4 frames per thread
    if (e >= total) return;
    const int cp = min(src_stride, dst_stride) / 4;
    const int t4 = (int)(e % cp) * 4;
    long long r = e / cp;
    const int f = (int)(r % F); r /= F;
    const int c = (int)(r % C);
    const int chunk = (int)(r / C);
    const int gs = chunk * src_stride + t4, gd = chunk * dst_stride + t4;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(src + ft_idx(gs >> 4, C, c, F, f) + (gs & 15));
    *reinterpret_cast<f32x4 *>(dst + ft_idx(gd >> 4, C, c, F, f) + (gd & 15)) = v;
    (void)frames;
}

// ---------------------------------------------------------------------------------------------
// lstm_t: LSTM ALONG TIME (CH_LSTM_T :252-267), one sequence per bin, batch = 16 bins of one chunk.
//   Two layers (hidden 40, the bottleneck `ch_lstm`, lstm_t2_kernel): of a wave pair, one runs layer 0 and the other layer 1
//   one step behind, h0 handed over through double-buffered LDS (one barrier per step).  One layer (out_ch_lstm): lstm_t_kernel.
//   The output Linear is applied per step from the register-resident h; MODE 0 multiplies it with a
//   second tensor (d5 input = e5 * lstm_out, NET.forward :236), MODE 1 stores it (out_ch_lstm).
// ---------------------------------------------------------------------------------------------
struct LstmTArgs {
    View in;
    LN ln;                                                   // LayerNorm on the layer-0 input (NET.ln before ch_lstm)
    const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2];      // per layer
    const float *wl, *bl;                                    // Linear [OUTP][HID] (rows zero padded), [OUTP]
    View mul;                                                // MODE 0
    ViewW out;
    int F, T, nt, out_ch;
    int tp;                                                  // frames between the starts of two chunks in the FT tensor: nt * 16 (each chunk
                                                             // on its own tiles) or a packed stride (vadx_dfsmn_ft_repack), a multiple of 4
    int nunits;                                              // lstm_t2_kernel: chunks * (F / 16) bin groups
};

// acc[mt] += W(mt, s) * b[s] over KS k-steps with the A fragments in LDS (w = this lane's base: fragment (mt, s) at w[(mt * KS + s) * 64]).
// One k-step's MT fragments are in flight while the previous step's MFMAs issue; the fences keep the scheduler from hoisting
// every read of the GEMM to its top (100 registers for a 10 x 10 layer: spills at three waves per SIMD).
template <int MT, int KS>
__device__ __forceinline__ void gemm_lds_frag(f32x4 (&acc)[MT], const float *w, const float (&b)[KS]) {
    float wc[MT], wn[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) wc[mt] = w[(mt * KS) * 64];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) wn[mt] = w[(mt * KS + s + 1) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16(wc[mt], b[s], acc[mt]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) wc[mt] = wn[mt];
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Two-layer bottleneck LSTM (loads / stores issued per step, requested one step ahead) with every weight in LDS.  Its predecessor
// kept a layer's weights in its wave's registers (452 VGPRs + AGPRs): one wave per SIMD, and a lone wave pays 15.1 ns per MFMA,
// 2.6 ns per VALU instruction and 7 ns per transcendental where co-resident waves pay 13.7 / 0.93 / 6 (tools/mfma_valu_overlap.sh)
// -- it sat at 0.38 of the pipe, 32.6 ms per 3060 windows; this form takes 26.4 ms (outputs equal to 7e-7).  The weights are the
// same for every bin group, so ONE copy per CU lives in LDS as per-lane A fragments, [row tile][k-step][lane] (W_ih0 12.8 KB,
// W_hh0 / W_ih1 / W_hh1 25.6 KB each, the output Linear 5 KB: 95 KB; a lane's fragment is one conflict-free ds_read, and LDS
// reads cost next to nothing beside MFMAs), and a workgroup runs NTILE bin groups at once: 2 NTILE waves of 228 registers --
// NTILE = 4: two per SIMD (six waves of <= 168 registers spill) -- sharing the matrix pipe, one barrier per step.
// (The same scheme for the ONE-layer out_ch_lstm -- 40 input channels gathered 4 B at a time per step, 125 registers, four waves
// per SIMD -- ran three times slower than lstm_t_kernel's loader wave, 37 vs 12.4 ms per 3060 windows: that LSTM is bound by its
// memory path, not by the pipe.)
template <int IN, int HID, int OUT_MT, int MODE, int NTILE>
__global__ __launch_bounds__(128 * NTILE) void lstm_t2_kernel(LstmTArgs p) {
    constexpr int MT = HID / 4, KI0 = IN / 4;
    constexpr int OFF_WI0 = 0, OFF_WH0 = OFF_WI0 + MT * KI0 * 64, OFF_WI1 = OFF_WH0 + MT * MT * 64, OFF_WH1 = OFF_WI1 + MT * MT * 64,
                  OFF_WL = OFF_WH1 + MT * MT * 64, OFF_BIAS = OFF_WL + OUT_MT * MT * 64, OFF_HS = OFF_BIAS + 2 * MT * 16,
                  LDS_FLOATS = OFF_HS + NTILE * 2 * HID * 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
    // (waves w and w + NTILE share a SIMD: one of each layer there -- with slot = wave >> 1, layer = wave & 1 two SIMDs carried two layer-1
    //  waves, 220 MFMAs each, and two SIMDs two layer-0 waves of 150)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = wave % NTILE, layer = wave / NTILE, q = lane >> 4, i = lane & 15;
    const int groups = p.F / 16;
    // ---- one copy of the weights per workgroup: fragment (mt, s) of matrix W[4 HID][K], lane (q, i) <- W[grow(i) + 4 mt][4 s + q]
    auto stage_w = [&](float *dst, const float *W, int K, int nmt, bool gate_rows) {
        const int ks = K / 4;
        for (int e = tid; e < nmt * ks * 64; e += blockDim.x) {
            const int l = e & 63, s2 = (e >> 6) % ks, mt = (e >> 6) / ks, lq = l >> 4, li = l & 15;
            const int row = gate_rows ? ((li & 3) * HID + (li >> 2) + 4 * mt) : (mt * 16 + li);
            dst[e] = W[(size_t)row * K + 4 * s2 + lq];
        }
    };
    stage_w(lds + OFF_WI0, p.w_ih[0], IN, MT, true);
    stage_w(lds + OFF_WH0, p.w_hh[0], HID, MT, true);
    stage_w(lds + OFF_WI1, p.w_ih[1], HID, MT, true);
    stage_w(lds + OFF_WH1, p.w_hh[1], HID, MT, true);
    stage_w(lds + OFF_WL, p.wl, HID, OUT_MT, false);
    for (int e = tid; e < 2 * MT * 16; e += blockDim.x) {                 // bias rows: [layer][mt][q][gate r]
        const int l2 = e / (MT * 16), r = e & 3, qq = (e >> 2) & 3, mt = (e >> 4) % MT;
        lds[OFF_BIAS + e] = p.b_ih[l2][r * HID + 4 * mt + qq] + p.b_hh[l2][r * HID + 4 * mt + qq];
    }
    __syncthreads();
    const int unit = blockIdx.x * NTILE + slot;                           // this wave pair's (chunk, bin group)
    const int total = p.nunits;
    const bool live = unit < total;
    const int uc = live ? unit : total - 1, chunk = uc / groups, f0 = (uc - chunk * groups) * 16;
    float *hs = lds + OFF_HS + slot * 2 * HID * 16;                       // [2][HID][16]: layer 0's h, double buffered
    const float *wi = lds + (layer == 0 ? OFF_WI0 : OFF_WI1) + lane, *wh = lds + (layer == 0 ? OFF_WH0 : OFF_WH1) + lane;
    const float *wl = lds + OFF_WL + lane;
    const f32x4 *biasq = reinterpret_cast<const f32x4 *>(lds + OFF_BIAS + layer * MT * 16) + q;
    float h[MT], c[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { h[mt] = 0.f; c[mt] = 0.f; }
    // every per-step global value is requested ONE STEP AHEAD, unconditionally (time index clamped)
    float lnw[KI0], lnb[KI0], xn[KI0], mean_n = 0.f, inv_n = 1.f, muln[OUT_MT][4], blr[OUT_MT][4];
#pragma unroll
    for (int s = 0; s < KI0; ++s) {
        lnw[s] = p.ln.stats ? p.ln.w[(4 * s + q) * p.F + f0 + i] : 1.f;
        lnb[s] = p.ln.stats ? p.ln.b[(4 * s + q) * p.F + f0 + i] : 0.f;
        xn[s] = 0.f;
    }
#pragma unroll
    for (int om = 0; om < OUT_MT; ++om)
#pragma unroll
        for (int r = 0; r < 4; ++r) { muln[om][r] = 1.f; blr[om][r] = (om * 16 + 4 * q + r) < p.out_ch ? p.bl[om * 16 + 4 * q + r] : 0.f; }
    auto prefetch = [&](int t) {
        const int tc = t < 0 ? 0 : (t >= p.T ? p.T - 1 : t), gfr = chunk * p.tp + tc, tile = gfr >> 4, t16 = gfr & 15;
        if (layer == 0) {
#pragma unroll
            for (int s = 0; s < KI0; ++s) xn[s] = p.in.ptr[ft_idx(tile, p.in.c_total, p.in.c_off + 4 * s + q, p.F, f0 + i) + t16];
            if (p.ln.stats) { mean_n = p.ln.stats[((size_t)tile * 16 + t16) * 2]; inv_n = p.ln.stats[((size_t)tile * 16 + t16) * 2 + 1]; }
        } else if (MODE == 0) {
#pragma unroll
            for (int om = 0; om < OUT_MT; ++om)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = om * 16 + 4 * q + r, oc = o < p.out_ch ? o : p.out_ch - 1;
                    muln[om][r] = p.mul.ptr[ft_idx(tile, p.mul.c_total, p.mul.c_off + oc, p.F, f0 + i) + t16];
                }
        }
    };
    prefetch(0);
    for (int it = 0; it < p.T + 1; ++it) {
        const int t = it - layer;                            // this wave's time step
        if (t >= 0 && t < p.T) {
            const int gfr = chunk * p.tp + t, tile = gfr >> 4, t16 = gfr & 15;
            f32x4 acc[MT];
            float mulc[OUT_MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = biasq[mt * 4];
            if (layer == 0) {
                float x[KI0];
#pragma unroll
                for (int s = 0; s < KI0; ++s) x[s] = p.ln.stats ? (xn[s] - mean_n) * inv_n * lnw[s] + lnb[s] : xn[s];
                prefetch(t + 1);
                gemm_lds_frag<MT, KI0>(acc, wi, x);
            } else {
                float x[MT];
#pragma unroll
                for (int s = 0; s < MT; ++s) x[s] = hs[(t & 1) * HID * 16 + (4 * s + q) * 16 + i];
#pragma unroll
                for (int om = 0; om < OUT_MT; ++om)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mulc[om][r] = muln[om][r];
                prefetch(t + 1);
                gemm_lds_frag<MT, MT>(acc, wi, x);
            }
            gemm_lds_frag<MT, MT>(acc, wh, h);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float ig = gate_sigmoid(acc[mt][0]), fg = gate_sigmoid(acc[mt][1]), gg = gate_tanh(acc[mt][2]), og = gate_sigmoid(acc[mt][3]);
                c[mt] = fg * c[mt] + ig * gg;
                h[mt] = og * gate_tanh(c[mt]);
                if (layer == 0) hs[(t & 1) * HID * 16 + (4 * mt + q) * 16 + i] = h[mt];
            }
            if (layer == 1) {
                f32x4 yy[OUT_MT];
#pragma unroll
                for (int om = 0; om < OUT_MT; ++om) yy[om] = f32x4{0.f, 0.f, 0.f, 0.f};
                gemm_lds_frag<OUT_MT, MT>(yy, wl, h);
#pragma unroll
                for (int om = 0; om < OUT_MT; ++om) {
                    const f32x4 y = yy[om];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = om * 16 + 4 * q + r;
                        if (o < p.out_ch && live) {
                            float v = y[r] + blr[om][r];
                            p.out.ptr[ft_idx(tile, p.out.c_total, p.out.c_off + o, p.F, f0 + i) + t16] = MODE == 0 ? v * mulc[om][r] : v;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// The two-layer time LSTM on fp16 x 2 split products (csrc/split2.h).  Same decomposition as lstm_t2_kernel (a wave pair per 16-bin
// group, layer 1 one step behind layer 0, one barrier per step, every weight in LDS as per-lane A fragments), but a layer's step is ONE
// GEMM over the concatenated operand [h ; x] with 32-k chunks: layer 0 [h0 (40) ; x (20)] = 2 chunks, layer 1 [h1 (40) ; h0 (40)] = 3,
// i.e. 60 / 90 v_mfma_f32_16x16x32_f16 per step (960 / 1440 matrix cycles) instead of 150 / 200 v_mfma_f32_16x16x4_f32 (4800 / 6400); the
// weights are 110 KB of fragments instead of 95 (bf16 x 3 needed 162 KB and did not fit: see the launch site).
//   k-slot maps (same for the A fragments and the B operand; lane 16 g + n supplies slots e = 0..7 of group g for bin n):
//     "own" chunk: slot (g, e) = the layer's h of unit 4 e + g -- the lane's OWN cell outputs of row tiles 0..7 (D rows 4 q + r of
//                  row tile mt are the four gates of unit 4 mt + q: the new h is the next step's operand without cross-lane traffic);
//     layer 0 chunk 1: e = 0, 1 -> own units 32 + g, 36 + g (row tiles 8, 9); e = 2..6 -> x channel 5 g + e - 2; e = 7 -> zero;
//     layer 1 chunk 1: h0 of unit 4 e + g = layer 0's own chunk, which that wave leaves in LDS ALREADY SPLIT (two 16-byte stores);
//     layer 1 chunk 2: e = 0, 1 -> own units of row tiles 8, 9; e = 2, 3 -> h0 of units 32 + g, 36 + g (layer 0's 4-byte "head"); rest zero.
//   The output Linear takes layer 1's NEW own chunk and chunk 2 (its weights are zero on the h0 / empty slots).  Biases are the
//   accumulators' initial value (exact float32 adds, as in the f32 kernel).  h lies in (-1, 1); x and the weights feed the range check.
// ---------------------------------------------------------------------------------------------
template <int NPAIR>
__device__ __forceinline__ void gemm_h2_lds(f32x4 *hi, f32x4 *mid, const unsigned char *w, int frag_stride2, const f16x8 (&b)[2]) {
    // NPAIR pairs of row tiles against one chunk's operand b; fragment pair of row tile mt at w + mt * frag_stride2 (+ 1024 for plane 1).
    // A pair's four fragments are requested while the previous pair's six MFMAs issue; the two tiles of a pair alternate so that no
    // MFMA waits on the one before it.
    f16x8 cur[2][2], nxt[2][2];
    auto load = [&](int pr, f16x8 (&a)[2][2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) a[u][pl] = *reinterpret_cast<const f16x8 *>(w + (size_t)(2 * pr + u) * frag_stride2 + pl * 1024);
    };
    load(0, cur);
#pragma unroll
    for (int pr = 0; pr < NPAIR; ++pr) {
        if (pr + 1 < NPAIR) load(pr + 1, nxt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; ++u) mid[2 * pr + u] = vadx::mfma_f16(cur[u][1], b[0], mid[2 * pr + u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) mid[2 * pr + u] = vadx::mfma_f16(cur[u][0], b[1], mid[2 * pr + u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) hi[2 * pr + u] = vadx::mfma_f16(cur[u][0], b[0], hi[2 * pr + u]);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) cur[u][pl] = nxt[u][pl];
        __builtin_amdgcn_sched_barrier(0);
    }
}


template <int OUT_MT, int MODE, int NTILE>
__global__ __launch_bounds__(128 * NTILE) void lstm_t2h_kernel(LstmTArgs p, unsigned *__restrict__ range_flag) {
    constexpr int IN = 20, HID = 40, MT = 10, FR = 1024;
    constexpr int OFF_W0 = 0, OFF_W1 = OFF_W0 + MT * 2 * 2 * FR, OFF_WL = OFF_W1 + MT * 3 * 2 * FR, OFF_BIAS = OFF_WL + OUT_MT * 2 * 2 * FR,
                  OFF_HS = OFF_BIAS + 2 * MT * 16 * 4, HS_BUF = 2 * FR + 2 * 256, LDS_BYTES = OFF_HS + NTILE * 2 * HS_BUF;
    static_assert(LDS_BYTES <= 160 * 1024 && OFF_HS % 16 == 0, "LDS budget");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, slot = wave % NTILE, layer = wave / NTILE, q = lane >> 4, i = lane & 15;      // one wave of each layer per SIMD
    const int groups = p.F / 16;
    float amax = 0.f;
    // ---- one copy of the weights per workgroup, split by the threads that stage them: fragment slot (tile, chunk, lane 16 g + r, e)
    {
        auto put = [&](int off, int frag, int l, int e, float wv) {
            unsigned short h0, h1;
            vadx::split2x1(wv, h0, h1, amax);
            *reinterpret_cast<unsigned short *>(smem + off + (size_t)frag * 2 * FR + l * 16 + e * 2) = h0;
            *reinterpret_cast<unsigned short *>(smem + off + (size_t)frag * 2 * FR + FR + l * 16 + e * 2) = h1;
        };
        for (int s2 = tid; s2 < MT * 2 * 512; s2 += blockDim.x) {           // layer 0: [h0 own | h0 tiles 8, 9 ; x ; 0]
            const int e = s2 & 7, l = (s2 >> 3) & 63, frag = s2 >> 9, ch = frag & 1, mt = frag >> 1, g = l >> 4, r = l & 15;
            const int row = (r & 3) * HID + (r >> 2) + 4 * mt;
            float wv = 0.f;
            if (ch == 0) wv = p.w_hh[0][(size_t)row * HID + 4 * e + g];
            else if (e < 2) wv = p.w_hh[0][(size_t)row * HID + 4 * (8 + e) + g];
            else if (e < 7) wv = p.w_ih[0][(size_t)row * IN + 5 * g + e - 2];
            put(OFF_W0, frag, l, e, wv);
        }
        for (int s2 = tid; s2 < MT * 3 * 512; s2 += blockDim.x) {           // layer 1: [h1 own | h0 own | h1 tiles 8, 9 ; h0 tiles 8, 9 ; 0]
            const int e = s2 & 7, l = (s2 >> 3) & 63, frag = s2 >> 9, ch = frag % 3, mt = frag / 3, g = l >> 4, r = l & 15;
            const int row = (r & 3) * HID + (r >> 2) + 4 * mt;
            float wv = 0.f;
            if (ch == 0) wv = p.w_hh[1][(size_t)row * HID + 4 * e + g];
            else if (ch == 1) wv = p.w_ih[1][(size_t)row * HID + 4 * e + g];
            else if (e < 2) wv = p.w_hh[1][(size_t)row * HID + 4 * (8 + e) + g];
            else if (e < 4) wv = p.w_ih[1][(size_t)row * HID + 4 * (8 + e - 2) + g];
            put(OFF_W1, frag, l, e, wv);
        }
        for (int s2 = tid; s2 < OUT_MT * 2 * 512; s2 += blockDim.x) {       // output Linear: [h1 own | h1 tiles 8, 9 ; 0]
            const int e = s2 & 7, l = (s2 >> 3) & 63, frag = s2 >> 9, ch = frag & 1, om = frag >> 1, g = l >> 4, r = l & 15;
            // D row 4 qq + rr of row tile om is output 5 qq + rr (om = 0) / 5 qq + 4 (om = 1, rr = 0): five outputs per lane quarter
            const int qq = r >> 2, rr = r & 3, row = om == 0 ? 5 * qq + rr : (rr == 0 ? 5 * qq + 4 : -1);
            float wv = 0.f;
            if (row >= 0 && row < p.out_ch) {
                if (ch == 0) wv = p.wl[(size_t)row * HID + 4 * e + g];
                else if (e < 2) wv = p.wl[(size_t)row * HID + 4 * (8 + e) + g];
            }
            put(OFF_WL, frag, l, e, wv);
        }
        float *bias = reinterpret_cast<float *>(smem + OFF_BIAS);
        for (int e = tid; e < 2 * MT * 16; e += blockDim.x) {               // bias rows: [layer][mt][q][gate r]
            const int l2 = e / (MT * 16), r = e & 3, qq = (e >> 2) & 3, mt = (e >> 4) % MT;
            bias[e] = p.b_ih[l2][r * HID + 4 * mt + qq] + p.b_hh[l2][r * HID + 4 * mt + qq];
        }
        for (int e = tid; e < NTILE * 2 * HS_BUF / 4; e += blockDim.x) reinterpret_cast<unsigned *>(smem + OFF_HS)[e] = 0u;
    }
    __syncthreads();
    const int unit = blockIdx.x * NTILE + slot;                           // this wave pair's (chunk, bin group)
    const int total = p.nunits;
    const bool live = unit < total;
    const int uc = live ? unit : total - 1, chunk = uc / groups, f0 = (uc - chunk * groups) * 16;
    unsigned char *hs = smem + OFF_HS + slot * 2 * HS_BUF;                // [2 buffers][plane 0 | plane 1 (1 KB each) | head 0 | head 1 (256 B each)]
    const unsigned char *wbase = smem + (layer == 0 ? OFF_W0 : OFF_W1) + lane * 16;
    constexpr int NCH0 = 2, NCH1 = 3;
    const f32x4 *biasq = reinterpret_cast<const f32x4 *>(smem + OFF_BIAS + layer * MT * 16 * 4) + q;
    float h[MT], c[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { h[mt] = 0.f; c[mt] = 0.f; }
    f16x8 bown[2] = {f16x8{0, 0, 0, 0, 0, 0, 0, 0}, f16x8{0, 0, 0, 0, 0, 0, 0, 0}};      // own chunk of the next step (h = 0)
    unsigned head_own[2] = {0u, 0u};                                                      // own units of row tiles 8, 9: two fp16 per plane
    // Memory path: in the FT layout the 16 frames of a (channel, bin) row are contiguous, so a lane moves FOUR time steps per request:
    // layer 0 loads the x rows of steps 4 k .. 4 k + 3 as one float4 per channel a group ahead (+ the LayerNorm statistics of the four
    // frames), layer 1 loads `mul` the same way at the start of a group and stores its outputs as one float4 per channel at the group's
    // end.  (As per-step 4-byte accesses -- the f32 kernel's way -- the loads and the stores each took 40 % of this kernel: what-ifs
    // 24 -> 14 ms per 3840 windows without either.)  tp and the group starts are multiples of 4: a group never straddles a tile.
    static_assert(OUT_MT == 2, "the 20 outputs sit as rows 5 q + j: j < 4 in row tile 0, j = 4 in row 4 q of row tile 1");
    constexpr int NO = 5;
    float lnw[5], lnb[5], blr[NO];
    // (a wave is layer 0 or layer 1 for its whole life: the two roles' group registers share storage -- ioa = x of this group / mul,
    //  iob = x of the next group / the outputs)
    f32x4 ioa[5], iob[5], st_m = {0.f, 0.f, 0.f, 0.f}, st_i = {1.f, 1.f, 1.f, 1.f}, st_mn = st_m, st_in = st_i;
    f32x4 (&xg)[5] = ioa, (&xg_n)[5] = iob, (&mg)[5] = ioa, (&og)[5] = iob;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        lnw[s] = p.ln.stats ? p.ln.w[(5 * q + s) * p.F + f0 + i] : 1.f;
        lnb[s] = p.ln.stats ? p.ln.b[(5 * q + s) * p.F + f0 + i] : 0.f;
        ioa[s] = layer == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{1.f, 1.f, 1.f, 1.f}; iob[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < NO; ++j) blr[j] = p.bl[5 * q + j];
    auto group_pos = [&](int t0, int &tile, int &t16) {          // t0 = first step of a group (clamped into the clip)
        const int tc = t0 >= p.T ? ((p.T - 1) & ~3) : t0, gfr = chunk * p.tp + tc;
        tile = gfr >> 4; t16 = gfr & 15;
    };
    auto load_x_group = [&](int t0) {                            // layer 0: the next group's inputs
        int tile, t16;
        group_pos(t0, tile, t16);
#pragma unroll
        for (int s = 0; s < 5; ++s) xg_n[s] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + 5 * q + s, p.F, f0 + i) + t16);
        if (p.ln.stats) {
            const float *sp = p.ln.stats + ((size_t)tile * 16 + t16) * 2;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(sp), b2 = *reinterpret_cast<const f32x4 *>(sp + 4);
            st_mn = f32x4{a[0], a[2], b2[0], b2[2]};
            st_in = f32x4{a[1], a[3], b2[1], b2[3]};
        }
    };
    auto load_mul_group = [&](int t0) {                          // layer 1, MODE 0: this group's multipliers (first used at the step's end)
        int tile, t16;
        group_pos(t0, tile, t16);
#pragma unroll
        for (int j = 0; j < NO; ++j) mg[j] = *reinterpret_cast<const f32x4 *>(p.mul.ptr + ft_idx(tile, p.mul.c_total, p.mul.c_off + 5 * q + j, p.F, f0 + i) + t16);
    };
    auto pick = [](const f32x4 &v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])); };
    if (layer == 0) load_x_group(0);
    for (int it = 0; it < p.T + 1; ++it) {
        const int t = it - layer;                            // this wave's time step
        if (t >= 0 && t < p.T) {
            const int j4 = t & 3;
            unsigned char *hbuf = hs + (t & 1) * HS_BUF;
            f16x8 bop[2][2];                                 // the operand chunks besides the own one (layer 0: one, layer 1: two)
            if (layer == 0) {
                if (j4 == 0) {
#pragma unroll
                    for (int s = 0; s < 5; ++s) xg[s] = xg_n[s];
                    st_m = st_mn; st_i = st_in;
                    load_x_group(t + 4);
                }
                float v1[8];
                v1[0] = 0.f; v1[1] = 0.f; v1[7] = 0.f;
                const float mean_c = pick(st_m, j4), inv_c = pick(st_i, j4);
#pragma unroll
                for (int s = 0; s < 5; ++s) { const float xv = pick(xg[s], j4); v1[2 + s] = p.ln.stats ? (xv - mean_c) * inv_c * lnw[s] + lnb[s] : xv; }
                split8(v1, bop[0], amax);
                {   // slots 0, 1 of chunk 1 = the own units of row tiles 8, 9 (split at the end of the previous step)
                    typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
                    u32x4_ w0 = __builtin_bit_cast(u32x4_, bop[0][0]), w1 = __builtin_bit_cast(u32x4_, bop[0][1]);
                    w0[0] = head_own[0]; w1[0] = head_own[1];
                    bop[0][0] = __builtin_bit_cast(f16x8, w0); bop[0][1] = __builtin_bit_cast(f16x8, w1);
                }
                bop[1][0] = bop[0][0]; bop[1][1] = bop[0][1];
            } else {
                if (MODE == 0 && j4 == 0) load_mul_group(t);
                bop[0][0] = *reinterpret_cast<const f16x8 *>(hbuf + lane * 16);
                bop[0][1] = *reinterpret_cast<const f16x8 *>(hbuf + FR + lane * 16);
                typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
                const unsigned hd0 = *reinterpret_cast<const unsigned *>(hbuf + 2 * FR + lane * 4), hd1 = *reinterpret_cast<const unsigned *>(hbuf + 2 * FR + 256 + lane * 4);
                bop[1][0] = __builtin_bit_cast(f16x8, u32x4_{head_own[0], hd0, 0u, 0u});
                bop[1][1] = __builtin_bit_cast(f16x8, u32x4_{head_own[1], hd1, 0u, 0u});
            }
            // row tiles in two passes (0..5, 6..9): 48 accumulator registers instead of 80 -- the operands are fragments in registers, the
            // cell update of the first pass touches nothing the second pass reads
            auto pass = [&](auto t0_c, auto np_c) {
                constexpr int T0 = decltype(t0_c)::value, NPR = decltype(np_c)::value;
                f32x4 hi[2 * NPR], mid[2 * NPR];
#pragma unroll
                for (int u = 0; u < 2 * NPR; ++u) { hi[u] = biasq[(T0 + u) * 4]; mid[u] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                if (layer == 0) {
                    gemm_h2_lds<NPR>(hi, mid, wbase + T0 * NCH0 * 2 * FR, NCH0 * 2 * FR, bown);
                    gemm_h2_lds<NPR>(hi, mid, wbase + T0 * NCH0 * 2 * FR + 2 * FR, NCH0 * 2 * FR, bop[0]);
                } else {
                    gemm_h2_lds<NPR>(hi, mid, wbase + T0 * NCH1 * 2 * FR, NCH1 * 2 * FR, bown);
                    gemm_h2_lds<NPR>(hi, mid, wbase + T0 * NCH1 * 2 * FR + 2 * FR, NCH1 * 2 * FR, bop[0]);
                    gemm_h2_lds<NPR>(hi, mid, wbase + T0 * NCH1 * 2 * FR + 4 * FR, NCH1 * 2 * FR, bop[1]);
                }
#pragma unroll
                for (int u = 0; u < 2 * NPR; ++u) {
                    const int mt = T0 + u;
                    const f32x4 a = vadx::join2(hi[u], mid[u]);
                    const float ig = gate_sigmoid(a[0]), fg = gate_sigmoid(a[1]);
                    const float gg = gate_tanh(a[2]), og2 = gate_sigmoid(a[3]);
                    c[mt] = fg * c[mt] + ig * gg;
                    h[mt] = og2 * gate_tanh(c[mt]);
                }
            };
            pass(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
            pass(std::integral_constant<int, 6>{}, std::integral_constant<int, 2>{});
            {   // the new h as the next step's operand: own chunk (row tiles 0..7) and the head (row tiles 8, 9)
                float v0[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v0[e] = h[e];
                split8(v0, bown, amax);
                unsigned short a0, a1, c0, c1;
                vadx::split2x1(h[8], a0, a1, amax);
                vadx::split2x1(h[9], c0, c1, amax);
                head_own[0] = (unsigned)a0 | ((unsigned)c0 << 16);
                head_own[1] = (unsigned)a1 | ((unsigned)c1 << 16);
            }
            if (layer == 0) {
                *reinterpret_cast<f16x8 *>(hbuf + lane * 16) = bown[0];
                *reinterpret_cast<f16x8 *>(hbuf + FR + lane * 16) = bown[1];
                *reinterpret_cast<unsigned *>(hbuf + 2 * FR + lane * 4) = head_own[0];
                *reinterpret_cast<unsigned *>(hbuf + 2 * FR + 256 + lane * 4) = head_own[1];
            } else {
                f32x4 yh[OUT_MT], ym[OUT_MT];
#pragma unroll
                for (int om = 0; om < OUT_MT; ++om) { yh[om] = f32x4{0.f, 0.f, 0.f, 0.f}; ym[om] = yh[om]; }
                typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
                const f16x8 bt[2] = {__builtin_bit_cast(f16x8, u32x4_{head_own[0], 0u, 0u, 0u}), __builtin_bit_cast(f16x8, u32x4_{head_own[1], 0u, 0u, 0u})};
                const unsigned char *wl = smem + OFF_WL + lane * 16;
                gemm_h2_lds<OUT_MT / 2>(yh, ym, wl, 2 * 2 * FR, bown);
                gemm_h2_lds<OUT_MT / 2>(yh, ym, wl + 2 * FR, 2 * 2 * FR, bt);
                const f32x4 y0 = vadx::join2(yh[0], ym[0]), y1 = vadx::join2(yh[1], ym[1]);
#pragma unroll
                for (int j = 0; j < NO; ++j) {
                    float v = (j < 4 ? y0[j < 4 ? j : 0] : y1[0]) + blr[j];
                    if (MODE == 0) v *= pick(mg[j], j4);
#pragma unroll
                    for (int k = 0; k < 4; ++k) og[j][k] = (j4 == k) ? v : og[j][k];
                }
                if ((j4 == 3 || t == p.T - 1) && live) {        // the group's outputs leave together
                    int tile, t16;
                    group_pos(t - j4, tile, t16);
#pragma unroll
                    for (int j = 0; j < NO; ++j) {
                        float *dst = p.out.ptr + ft_idx(tile, p.out.c_total, p.out.c_off + 5 * q + j, p.F, f0 + i) + t16;
                        if (j4 == 3) *reinterpret_cast<f32x4 *>(dst) = og[j];
                        else
#pragma unroll
                            for (int k = 0; k < 3; ++k) if (k <= j4) dst[k] = og[j][k];
                    }
                }
            }
        }
        __syncthreads();
    }
    vadx::range_flag_raise(range_flag, amax);
}

// Memory path.  In the FT layout one time step of a 16-bin group is 16 B out of each of IN*16 different 64-B rows, so
// per-step loads / stores (one cache line per lane, issued when needed) left the recurrence waiting on HBM every
// step.  A dedicated LOADER wave (the last wave of the workgroup; it holds no weights) streams CHUNKS of TS steps:
// it requests chunk k+1's rows as 16-B loads while the compute waves run chunk k, applies the LayerNorm, and parks
// them transposed in LDS as Xs[ch][t][bin] (channel pitch = 16 mod 32 floats: the MFMA B operand reads are conflict
// free); the last layer's outputs go to Ys[o][t][bin] and the loader writes chunk k-1 back as 16-B stores (times the
// `mul` tensor in MODE 0).  One workgroup barrier per step orders everything (it already paced the two layers).
template <int IN, int HID, int LAYERS, int OUT_MT, int MODE, int TS, int OUT_CH = OUT_MT * 16>
__global__ __launch_bounds__(64 * (LAYERS + 1)) void lstm_t_kernel(LstmTArgs p) {
    constexpr int MT = HID / 4, KI0 = IN / 4, CS = TS * 16 + 16, NQ = TS / 4;
    constexpr int NLD = IN * NQ / 4;                         // float4 loads per loader lane per chunk
    constexpr int OUTC = OUT_CH;                             // rows of the output staging block: the real channels (the MFMA tiles' padding rows are not stored)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Xs = lds;                                         // [2][IN][CS]
    float *Ys = Xs + 2 * IN * CS;                            // [2][OUTC][CS]
    float *hs = Ys + 2 * OUTC * CS;                          // [2][HID*16]
    const int lane = threadIdx.x & 63, layer = threadIdx.x >> 6, q = lane >> 4, i = lane & 15;
    const int groups = p.F / 16, chunk = blockIdx.x / groups, f0 = (blockIdx.x - chunk * groups) * 16;
    const int NI = p.T + LAYERS - 1, nck = (p.T + TS - 1) / TS;

    if (layer == LAYERS) {
        // ------------------------------------------------------------------ loader / storer wave
        const int sub = lane >> 4, quad = sub % NQ, chs = sub / NQ;      // lane -> (bin i, time quad, channel sub-offset)
        f32x4 pre[NLD];
        auto request = [&](int ck) {
            const int t0 = chunk * p.tp + ck * TS, tile = t0 >> 4, tb = (t0 & 15) + 4 * quad;
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int ch = j * (4 / NQ) + chs;
                pre[j] = *reinterpret_cast<const f32x4 *>(p.in.ptr + ft_idx(tile, p.in.c_total, p.in.c_off + ch, p.F, f0 + i) + tb);
            }
        };
        auto park = [&](int ck) {
            const int t0 = chunk * p.tp + ck * TS, tile = t0 >> 4, tb = (t0 & 15) + 4 * quad;
            f32x4 mean = {0.f, 0.f, 0.f, 0.f}, inv = {1.f, 1.f, 1.f, 1.f};
            if (p.ln.stats)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    mean[r] = p.ln.stats[((size_t)tile * 16 + tb + r) * 2];
                    inv[r] = p.ln.stats[((size_t)tile * 16 + tb + r) * 2 + 1];
                }
            float *dst = Xs + (ck & 1) * IN * CS;
#pragma unroll
            for (int j = 0; j < NLD; ++j) {
                const int ch = j * (4 / NQ) + chs;
                f32x4 v = pre[j];
                if (p.ln.stats) v = (v - mean) * inv * p.ln.w[ch * p.F + f0 + i] + p.ln.b[ch * p.F + f0 + i];
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[ch * CS + (4 * quad + r) * 16 + i] = v[r];
            }
        };
        auto flush = [&](int ck) {
            const int t0 = chunk * p.tp + ck * TS, tile = t0 >> 4, tb = (t0 & 15) + 4 * quad;
            const float *src = Ys + (ck & 1) * OUTC * CS;
            for (int o = chs; o < p.out_ch; o += 4 / NQ) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = src[o * CS + (4 * quad + r) * 16 + i];
                if (MODE == 0) v *= *reinterpret_cast<const f32x4 *>(p.mul.ptr + ft_idx(tile, p.mul.c_total, p.mul.c_off + o, p.F, f0 + i) + tb);
                *reinterpret_cast<f32x4 *>(p.out.ptr + ft_idx(tile, p.out.c_total, p.out.c_off + o, p.F, f0 + i) + tb) = v;
            }
        };
        request(0);
        park(0);
        int flushed = 0;                                     // chunks [0, flushed) are written back
        __syncthreads();
        for (int it = 0; it < NI; ++it) {
            const int k = it / TS, j = it - k * TS;
            if (j == 0 && k + 1 < nck) request(k + 1);       // Xs[(k+1)&1] was last read in chunk k-1
            if (j == 1 && k >= 1) { flush(k - 1); flushed = k; }     // every layer left chunk k-1 before this iteration
            if (j == TS - 1 && k + 1 < nck) park(k + 1);
            __syncthreads();
        }
        for (int ck = flushed; ck < nck; ++ck) flush(ck);
        return;
    }

    // ---------------------------------------------------------------------- compute waves (one per layer)
    const int grow = (i & 3) * HID + (i >> 2);
    constexpr int KI = (LAYERS == 2) ? (KI0 > MT ? KI0 : MT) : KI0;       // register array bound
    const int ki = layer == 0 ? KI0 : MT, in_dim = layer == 0 ? IN : HID;
    float wi[MT][KI], wh[MT][MT], bias[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = grow + 4 * mt;
#pragma unroll
        for (int s = 0; s < KI; ++s) wi[mt][s] = s < ki ? p.w_ih[layer][(size_t)row * in_dim + 4 * s + q] : 0.f;
#pragma unroll
        for (int s = 0; s < MT; ++s) wh[mt][s] = p.w_hh[layer][(size_t)row * HID + 4 * s + q];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[mt][r] = p.b_ih[layer][r * HID + 4 * mt + q] + p.b_hh[layer][r * HID + 4 * mt + q];
    }
    float wl[OUT_MT][MT], blr[OUT_MT][4];
#pragma unroll
    for (int om = 0; om < OUT_MT; ++om) {
#pragma unroll
        for (int s = 0; s < MT; ++s) wl[om][s] = p.wl[(size_t)(om * 16 + i) * HID + 4 * s + q];
#pragma unroll
        for (int r = 0; r < 4; ++r) blr[om][r] = (om * 16 + 4 * q + r) < p.out_ch ? p.bl[om * 16 + 4 * q + r] : 0.f;
    }
    float h[MT], c[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { h[mt] = 0.f; c[mt] = 0.f; }
    const bool last = layer == LAYERS - 1;
    __syncthreads();                                         // chunk 0 is parked
    for (int it = 0; it < NI; ++it) {
        const int t = it - layer;                            // this wave's time step
        if (t >= 0 && t < p.T) {
            const int ck = t / TS, tl = t - ck * TS;
            const float *xb = Xs + (ck & 1) * IN * CS + tl * 16 + i;
            float x[KI];
#pragma unroll
            for (int s = 0; s < KI; ++s) {
                x[s] = 0.f;
                if (s < ki) x[s] = layer == 0 ? xb[(4 * s + q) * CS] : hs[(t & 1) * HID * 16 + (4 * s + q) * 16 + i];
            }
            f32x4 acc[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{bias[mt][0], bias[mt][1], bias[mt][2], bias[mt][3]};
#pragma unroll
            for (int s = 0; s < KI; ++s)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16(wi[mt][s], x[s], acc[mt]);
#pragma unroll
            for (int s = 0; s < MT; ++s)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma16(wh[mt][s], h[s], acc[mt]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float ig = gate_sigmoid(acc[mt][0]), fg = gate_sigmoid(acc[mt][1]), gg = gate_tanh(acc[mt][2]), og = gate_sigmoid(acc[mt][3]);
                c[mt] = fg * c[mt] + ig * gg;
                h[mt] = og * gate_tanh(c[mt]);
                if (!last) hs[(t & 1) * HID * 16 + (4 * mt + q) * 16 + i] = h[mt];
            }
            if (last) {
                float *yb = Ys + (ck & 1) * OUTC * CS + tl * 16 + i;
#pragma unroll
                for (int om = 0; om < OUT_MT; ++om) {
                    f32x4 y = {blr[om][0], blr[om][1], blr[om][2], blr[om][3]};
#pragma unroll
                    for (int s = 0; s < MT; ++s) y = mfma16(wl[om][s], h[s], y);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (om * 16 + 4 * q + r < OUTC) yb[(om * 16 + 4 * q + r) * CS] = y[r];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// ISTFT of the ICCRN output (NET.istft :220-224): conv_transpose1d(Y[320][T], basis[320][319], stride 160)
// = per-frame GEMM Z[t][j] = sum_ch Y[ch][t] * basis[ch][j]  followed by overlap-add, crop of 159
// samples each side and the precomputed window_sum_inv scaling.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void istft_gemm_kernel(const float *__restrict__ Y, const float *__restrict__ basisT,
                                                         float *__restrict__ Z, int nt, int T) {
    // Y: FT [2 ch][160]; basisT: [320 j][320 ch] (row j = 319 is zero); Z: [chunk][T][320]
    __shared__ float Bs[320 * 16];
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, i = lane & 15;
    const int chunk = tile / nt, tl = tile - chunk * nt;
    for (int e = tid; e < 320 * 16; e += 256) Bs[e] = Y[(size_t)tile * 320 * 16 + e];      // [ch][16] contiguous in FT
    __syncthreads();
    for (int mt = wave; mt < 20; mt += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float *arow = basisT + (size_t)(mt * 16 + i) * 320 + q;
#pragma unroll 8
        for (int s = 0; s < 80; ++s) acc = mfma16(arow[4 * s], Bs[(4 * s + q) * 16 + i], acc);
        const int t = tl * 16 + i;
        if (t < T) {
            float *z = Z + ((size_t)chunk * T + t) * 320 + mt * 16 + 4 * q;
            *reinterpret_cast<f32x4 *>(z) = acc;
        }
    }
}

__global__ void istft_ola_kernel(const float *__restrict__ Z, const float *__restrict__ wsum_inv, float *__restrict__ out,
                                 int T, int L, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int chunk = (int)(e / L), n = (int)(e - (long long)chunk * L) + 159;         // position in the uncropped signal
    const int t1 = n / 160, j1 = n - t1 * 160;
    float v = 0.f;
    if (t1 < T) v = Z[((size_t)chunk * T + t1) * 320 + j1];
    if (t1 >= 1 && j1 + 160 < 319) v += Z[((size_t)chunk * T + t1 - 1) * 320 + j1 + 160];
    out[e] = v * wsum_inv[n];
}

// ---------------------------------------------------------------------------------------------
// look-ahead vote of the DFSMN driver on float scores (Inference_DFSMN_VAD_ONNX.py:231-273), one clip/thread
// ---------------------------------------------------------------------------------------------
struct Vote {
    int Tn, lb, slide;
    double speaking, silence_score, inv_lb;
    // A float32 score against the Python-float constant: NumPy 2 (NEP 50) compares in float32, i.e. against the constant rounded to
    // float32 -- a score of exactly float32(0.7) IS >= 0.7 there (tests/golden/hostloop_thresholds.npz, produced by the
    // reference loop under NumPy 2.2).  The vote ratio (int * float) against the constant stays a float64 comparison.
    float hi, lo;
    __device__ Vote(int Tn_, int lb_, double speaking_, double silence_score_)
        : Tn(Tn_), lb(lb_), slide(Tn_ - lb_), speaking(speaking_), silence_score(silence_score_), inv_lb(1.0 / (double)lb_),
          hi((float)speaking_), lo((float)silence_score_) {}

    // one window (:231-258): `slide` voted flags from its scores sc[0, Tn); returns the vote's `silence` after it
    __device__ int window(const float *__restrict__ sc, int silence, unsigned char *__restrict__ fl) const {
        for (int i2 = 0; i2 < slide; ++i2) {
            if (silence) {
                if (sc[i2] >= hi) {
                    int act = 1;
                    for (int j = 1; j < lb; ++j) act += (sc[i2 + j] >= hi) ? 1 : 0;
                    silence = !((double)act * inv_lb >= speaking);
                } else silence = 1;
            } else {
                if (sc[i2] <= lo) {
                    int act = 1;
                    for (int j = 1; j < lb; ++j) act += (sc[i2 + j] <= lo) ? 1 : 0;
                    silence = !((double)act * inv_lb <= silence_score);
                } else silence = 0;
            }
            fl[i2] = (unsigned char)silence;
        }
        return silence;
    }

    // the plain rule over the last window's last lb scores (:262-273): lb flags
    __device__ void tail(const float *__restrict__ sc, int silence, unsigned char *__restrict__ fl) const {
        for (int i2 = slide; i2 < Tn; ++i2) {
            if (silence) silence = !(sc[i2] >= hi);
            else silence = (sc[i2] <= lo) ? 1 : 0;
            fl[i2 - slide] = (unsigned char)silence;
        }
    }
};

__global__ void dfsmn_vote_kernel(const float *__restrict__ vad, int B, int W, int Tn, int lb, double speaking,
                                  double silence_score, unsigned char *__restrict__ flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const Vote v(Tn, lb, speaking, silence_score);
    int silence = 1;
    unsigned char *fl = flags + (size_t)b * (W * v.slide + lb);
    const float *sc = nullptr;
    for (int k = 0; k < W; ++k) {
        sc = vad + ((size_t)b * W + k) * Tn;
        silence = v.window(sc, silence, fl + k * v.slide);
    }
    v.tail(sc, silence, fl + W * v.slide);
}

// The same vote over a RAGGED batch: clip b owns the score rows win_first[b] .. win_first[b+1]-1 and row b of flags (filled with 255 by the
// caller of the kernel).  A table entry that does not describe rows inside `vad` leaves the thread without a store.
__global__ void dfsmn_vote_ragged_kernel(const float *__restrict__ vad, int B, int n_windows, int max_windows, const int *__restrict__ win_first,
                                         int Tn, int lb, double speaking, double silence_score, unsigned char *__restrict__ flags,
                                         long long flag_stride) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int first = win_first[b], last = win_first[b + 1];
    if (first < 0 || last > n_windows || last <= first || last - first > max_windows) return;
    const int W = last - first;
    const Vote v(Tn, lb, speaking, silence_score);
    int silence = 1;
    unsigned char *fl = flags + (size_t)b * flag_stride;
    const float *sc = nullptr;
    for (int k = 0; k < W; ++k) {
        sc = vad + ((size_t)first + k) * Tn;
        silence = v.window(sc, silence, fl + (size_t)k * v.slide);
    }
    v.tail(sc, silence, fl + (size_t)W * v.slide);
}

// ---- live near + far streams ------------------------------------------------------------------------------------------------------------
// The record of S streams with `ch` channels (include/vadx.h states the contract): header u32 [S][4] | carry int16 [ch][S][C],
// C = (look_backward + 1) * 320 = the samples two consecutive windows share.  Header words: 0 silence (the vote's), 1 primed (the stream
// has a carry), 2-3 windows done (u64).  The window kernel owns word 1 and the carry, the vote kernel the other words; zero bytes =
// un-primed = the reset state (silence takes its initial value, true, when an un-primed stream starts).
constexpr int SHDR_WORDS = 4, SH_SIL = 0, SH_PRIMED = 1, SH_DONE = 2, SFRAME = 320;
__host__ __device__ static size_t srec_carry(int S) { return (size_t)S * SHDR_WORDS * 4; }
static size_t srec_bytes(int S, int C, int ch) { return srec_carry(S) + (size_t)ch * S * C * sizeof(int16_t); }

// slot of stream s this tick: -1 = no audio (also for an entry outside [-1, n_slots))
__device__ __forceinline__ int stream_slot(const int *__restrict__ slot, int s, int n_slots) {
    const int a = slot ? slot[s] : s;
    return a >= 0 && a < n_slots ? a : -1;
}

struct StreamWinArgs {
    const int16_t *samples[2]; long long row_stride;   // per channel [S][row_stride]: each stream's new samples from column 0
    int S, n_slots, k, L, C, ch;                       // streams, slots, windows per tick, window length, carry length, channels
    const int *slot; const unsigned char *reset;       // optional [S]
    const unsigned char *sin; unsigned char *sout;     // records
    int16_t *wbuf[2];                                  // per channel [n_slots * k][L]
};

// Window assembly (the slicing of Inference_DFSMN_VAD_ONNX.py:221-229, 259-260 for a stream that arrives in pieces): a stream's timeline of
// this tick is its carry followed by its new samples (no carry before the first tick); window j = timeline[j * stride, j * stride + L), the
// new carry = the timeline's last C samples.  One workgroup per (channel, stream, window) plus one per (channel, stream) for the carry; one
// int16 per access (L and the stride are odd).  A sample past row_stride reads as zero.  An inactive stream keeps its carry and owns no row.
__global__ __launch_bounds__(256) void dfsmn_stream_windows_kernel(StreamWinArgs a) {
    const int per = a.k + 1, c = blockIdx.x / (a.S * per), r = blockIdx.x - c * (a.S * per), s = r / per, j = r - s * per, tid = threadIdx.x;
    const unsigned *hin = reinterpret_cast<const unsigned *>(a.sin) + (size_t)s * SHDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(a.sout) + (size_t)s * SHDR_WORDS;
    const size_t coff = srec_carry(a.S) + ((size_t)c * a.S + s) * a.C * sizeof(int16_t);
    const int16_t *cin = reinterpret_cast<const int16_t *>(a.sin + coff);
    int16_t *cout = reinterpret_cast<int16_t *>(a.sout + coff);
    const int slot = stream_slot(a.slot, s, a.n_slots);
    if (slot < 0) {
        if (j == a.k) {
            for (int i = tid; i < a.C; i += 256) cout[i] = cin[i];
            if (c == 0 && tid == 0) hout[SH_PRIMED] = hin[SH_PRIMED];
        }
        return;
    }
    const bool primed = hin[SH_PRIMED] != 0 && !(a.reset && a.reset[s]);
    const int16_t *smp = a.samples[c] + (long long)s * a.row_stride;
    const int stride = a.L - a.C;
    auto timeline = [&](long long i) -> int16_t {
        if (primed) {
            if (i < a.C) return cin[i];
            i -= a.C;
        }
        return i < a.row_stride ? smp[i] : (int16_t)0;
    };
    if (j < a.k) {
        int16_t *win = a.wbuf[c] + ((size_t)slot * a.k + j) * a.L;
        for (int i = tid; i < a.L; i += 256) win[i] = timeline((long long)j * stride + i);
    } else {
        for (int i = tid; i < a.C; i += 256) cout[i] = timeline((long long)a.k * stride + i);      // the timeline holds k * stride + C samples
        if (c == 0 && tid == 0) hout[SH_PRIMED] = 1u;
    }
}

struct StreamVoteArgs {
    const float *vad;                                  // [n_slots * k][Tn]
    int S, n_slots, k, Tn, lb;
    double speaking, silence_score;
    const int *slot; const unsigned char *reset;       // optional [S]
    const unsigned char *sin; unsigned char *sout;     // records
    unsigned char *flags, *tail;                       // [S][k * (Tn - lb)], [S][lb]
};

// One tick of the vote, one stream per thread: `silence` comes from state_in (true for an un-primed or reset stream), the tick's windows are
// voted as dfsmn_vote_kernel votes a clip's, the tail is what the plain rule would append if the stream ended here -- it starts from a copy
// of `silence`, the carried value is the one the next tick continues from.
__global__ void dfsmn_stream_vote_kernel(StreamVoteArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const Vote v(a.Tn, a.lb, a.speaking, a.silence_score);
    const unsigned *hin = reinterpret_cast<const unsigned *>(a.sin) + (size_t)s * SHDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(a.sout) + (size_t)s * SHDR_WORDS;
    unsigned char *fl = a.flags + (size_t)s * a.k * v.slide, *tl = a.tail + (size_t)s * a.lb;
    const int slot = stream_slot(a.slot, s, a.n_slots);
    if (slot < 0) {                        // no audio this tick: the record passes through bit for bit, a reset request is ignored
        hout[SH_SIL] = hin[SH_SIL]; hout[SH_DONE] = hin[SH_DONE]; hout[SH_DONE + 1] = hin[SH_DONE + 1];
        for (int i = 0; i < a.k * v.slide; ++i) fl[i] = 255;
        for (int i = 0; i < a.lb; ++i) tl[i] = 255;
        return;
    }
    const bool fresh = hin[SH_PRIMED] == 0 || (a.reset && a.reset[s]);
    int silence = fresh ? 1 : (int)hin[SH_SIL];
    const float *sc = nullptr;
    for (int k = 0; k < a.k; ++k) {
        sc = a.vad + ((size_t)slot * a.k + k) * a.Tn;
        silence = v.window(sc, silence, fl + (size_t)k * v.slide);
    }
    v.tail(sc, silence, tl);
    const unsigned long long done = (fresh ? 0ull : ((unsigned long long)hin[SH_DONE + 1] << 32 | hin[SH_DONE])) + (unsigned long long)a.k;
    hout[SH_SIL] = (unsigned)silence;
    hout[SH_DONE] = (unsigned)done; hout[SH_DONE + 1] = (unsigned)(done >> 32);
}


// ---------------------------------------------------------------------------------------------
// mask-net head (DFSMN_VAD.forward :349-353 + UniDeepFsmn.compute1, uni_deep_fsmn.py:311-329):
//   x = relu(linear1((feat + shift) * scale)); N x [ p = project(relu(linear(x))); x += conv1(0^19 ++ p) + p ];
//   vad = sigmoid(linear3(x)).   One workgroup per chunk, T <= 64 frames, activations k-major in LDS.
// ---------------------------------------------------------------------------------------------
constexpr int MK_LD = 68, MKP_LD = 84, MKP_CUR = 20;
constexpr int MK_A = 256 * MK_LD, MK_B = 128 * MK_LD, MK_P = 128 * MKP_LD;
constexpr int MK_LDS_FLOATS = MK_A + MK_B + MK_P;

struct MaskArgs {
    const float *feat;            // [chunks][T][240]
    const float *shift, *scale;   // [240]
    const float *w1, *b1;         // [Hp][240], [Hp]
    const float *wl[8], *bl[8], *wp[8], *wc[8];   // per layer: linear [H2p][Hp], bias, project [Hp][H2p], conv1 [H][lorder]
    const float *w3, *b3;         // [H], [1]
    float *vad;                   // [chunks][T]
    int T, H, Hp, H2p, layers, lorder;
};

__global__ __launch_bounds__(512, 2) void mask_net_kernel(MaskArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *bufA = lds, *bufB = lds + MK_A, *bufP = bufB + MK_B;
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const float *feat = p.feat + (size_t)chunk * p.T * 240;
    for (int e = tid; e < 64 * 240; e += 512) {
        const int t = e / 240, k = e - t * 240;
        bufA[k * MK_LD + t] = t < p.T ? (feat[(size_t)t * 240 + k] + p.shift[k]) * p.scale[k] : 0.f;
    }
    for (int e = tid; e < 128 * MKP_LD; e += 512) bufP[e] = 0.f;          // zero FIR history (stateless per chunk)
    __syncthreads();
    LayerArgs a{p.w1, 240, p.Hp / 16, 1, 15, 0, 0, p.b1, 1, bufA, MK_LD, 0, bufB, MK_LD, 0, nullptr, nullptr};
    layer<4, false>(a);
    __syncthreads();
    for (int l = 0; l < p.layers; ++l) {
        LayerArgs b{p.wl[l], p.Hp, p.H2p / 16, 1, p.Hp / 16, 0, 0, p.bl[l], 1, bufB, MK_LD, 0, bufA, MK_LD, 0, nullptr, nullptr};
        layer<4, false>(b);
        __syncthreads();
        LayerArgs c{p.wp[l], p.H2p, p.Hp / 16, 1, p.H2p / 16, 0, 0, nullptr, 0, bufA, MK_LD, 0, bufP, MKP_LD, MKP_CUR, nullptr, nullptr};
        layer<4, false>(c);
        __syncthreads();
        for (int e = tid; e < p.H * 64; e += 512) {       // depthwise causal FIR (zero left pad) + skip + residual
            const int ch = e >> 6, t = e & 63;
            const float *seq = bufP + ch * MKP_LD + MKP_CUR - (p.lorder - 1) + t;      // seq[k] = p[t - (lorder-1) + k]
            const float *wk = p.wc[l] + ch * p.lorder;
            float sfir = 0.f;
            for (int k = 0; k < p.lorder; ++k) sfir = fmaf(wk[k], seq[k], sfir);
            bufB[ch * MK_LD + t] += sfir + bufP[ch * MKP_LD + MKP_CUR + t];
        }
        __syncthreads();
    }
    if (tid < 64 && tid < p.T) {
        float sres = p.b3[0];
        for (int ch = 0; ch < p.H; ++ch) sres = fmaf(p.w3[ch], bufB[ch * MK_LD + tid], sres);
        p.vad[(size_t)chunk * p.T + tid] = sigmoidf_(sres);
    }
}

}  // namespace dfsmn
}  // namespace vadx

using namespace vadx::dfsmn;

static View mkview(const vadx_ft_view *v) { return View{v ? v->ptr : nullptr, v ? v->c_total : 0, v ? v->c_off : 0, v ? v->c : 0}; }
static ViewW mkvieww(const vadx_ft_view *v) { return ViewW{v ? const_cast<float *>(v->ptr) : nullptr, v ? v->c_total : 0, v ? v->c_off : 0, v ? v->c : 0}; }
static LN mkln(const vadx_ft_ln *l) { return LN{l ? l->stats : nullptr, l ? l->w : nullptr, l ? l->b : nullptr}; }

extern "C" int vadx_dfsmn_frame_stats(const vadx_ft_view *a, const vadx_ft_view *b, int F, int tiles, float *stats, void *stream) {
    VADX_REQUIRE(a && a->ptr && stats && F > 0 && tiles > 0, "vadx_dfsmn_frame_stats: bad argument");
    hipLaunchKernelGGL(frame_stats_kernel, dim3(tiles), dim3(256), 0, static_cast<hipStream_t>(stream), mkview(a), mkview(b), F, stats);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_stats_merge(const float *part_a, const float *part_b, int tiles, float *stats, void *stream) {
    VADX_REQUIRE(part_a && stats && tiles > 0, "vadx_dfsmn_stats_merge: bad argument");
    hipLaunchKernelGGL(stats_merge_kernel, dim3((unsigned)((tiles * 16 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       part_a, part_b, tiles, stats);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

template <int CO, int CIN, int KF, int MODE>
static int launch_pw(PwArgs p, int tiles, void *stream) {
    // a workgroup walks all chunks of its tile (weights stay in VGPRs), two workgroups per tile when there are few tiles
    using S = PwShape<CO, CIN, KF, MODE>;
    p.fc = S::FC;
    p.nchunk = (p.F + S::FC - 1) / S::FC;
    constexpr size_t lds = (size_t)S::LDS_FLOATS * sizeof(float);
    static_assert(S::LDS_FLOATS >= 144, "shape too small for the fused statistics' reduction scratch");
    VADX_DYN_LDS((pw_conv_kernel<CO, CIN, KF, MODE>), 64 * 1024);
    const unsigned split = tiles < 4096 ? 2 : 1;
    hipLaunchKernelGGL((pw_conv_kernel<CO, CIN, KF, MODE>), dim3((unsigned)tiles, split), dim3(256), lds,
                       static_cast<hipStream_t>(stream), p);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_pw_conv(int mode, const vadx_ft_view *a, const vadx_ft_view *b, const vadx_ft_ln *ln,
                                  const float *w, const float *bias, const float *w2, const float *bias2,
                                  const vadx_ft_view *add, const vadx_ft_view *out0, const vadx_ft_view *out1,
                                  int F, int co, int kf, int act, int tiles, float *part0, float *part1, void *stream) {
    VADX_REQUIRE(a && a->ptr && w && bias && out0 && out0->ptr && F > 0 && tiles > 0 && co > 0, "vadx_dfsmn_pw_conv: bad argument");
    PwArgs p;
    p.a = mkview(a); p.b = mkview(b); p.ln = mkln(ln); p.W = w; p.bias = bias; p.W2 = w2; p.bias2 = bias2;
    p.add = mkview(add); p.out0 = mkvieww(out0); p.out1 = mkvieww(out1); p.F = F; p.co = co; p.act = act;
    p.part0 = part0; p.part1 = mode == 1 ? part1 : nullptr;
    VADX_REQUIRE(mode == 0 ? !(ln && ln->stats) : (ln && ln->stats && ln->w && ln->b),
                 "vadx_dfsmn_pw_conv: mode %d %s a LayerNorm", mode, mode == 0 ? "takes no" : "needs");
    const int cin = p.a.c + p.b.c;
    VADX_REQUIRE((int64_t)tiles * 16 * 2 < INT32_MAX && (int64_t)(p.a.c_total + p.b.c_total + co) * F * 16 < INT32_MAX,
                 "vadx_dfsmn_pw_conv: tensor too large for the kernel's 32-bit in-tile offsets");
#define PW_CASE(cov, cinv, kfv, md) if (co == cov && cin == cinv && kf == kfv && mode == md) return launch_pw<cov, cinv, kfv, md>(p, tiles, stream)
    PW_CASE(20, 20, 1, 1);     // CFB front, 20 -> 20
    PW_CASE(20, 40, 1, 1);     // CFB front, 40 -> 20
    PW_CASE(20, 20, 3, 2);     // CFB back: conv (3,1) 20 -> 20 + ceps
    PW_CASE(20, 24, 1, 0);     // in_conv 24 -> 20
    PW_CASE(20, 40, 1, 0);     // in_ch_lstm linear 40 -> 20
    PW_CASE(40, 40, 1, 0);     // ceps linear 40 -> 40
    PW_CASE(2, 60, 1, 0);      // out_conv 60 -> 2
#undef PW_CASE
    vadx::set_error("vadx_dfsmn_pw_conv: unsupported shape (co=%d cin=%d kf=%d mode=%d)", co, cin, kf, mode);
    return VADX_EINVAL;
}

extern "C" int vadx_dfsmn_dft_f(int inverse, const vadx_ft_view *in, const vadx_ft_view *lo, const vadx_ft_ln *ln,
                                const float *tbl, const vadx_ft_view *out, int C, int tiles, float *part, void *stream) {
    VADX_REQUIRE(in && in->ptr && tbl && out && out->ptr && C > 0 && tiles > 0, "vadx_dfsmn_dft_f: bad argument");
    VADX_REQUIRE(inverse ? (lo && lo->ptr) : (ln && ln->stats), "vadx_dfsmn_dft_f: missing lo / ln");
    DftArgs p;
    p.in = mkview(in); p.lo = mkview(lo); p.ln = mkln(ln); p.tbl = tbl; p.out = mkvieww(out); p.C = C; p.part = inverse ? nullptr : part; p.tiles = tiles;
    const unsigned grid = (unsigned)(tiles < 512 ? tiles : 512);      // two persistent workgroups per CU, table in VGPRs
    if (inverse) hipLaunchKernelGGL(dft_f_kernel<true>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    else hipLaunchKernelGGL(dft_f_kernel<false>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_lstm_f(const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2],
                                 const float *const w_hh[2], const float *const b_ih[2], const float *const b_hh[2],
                                 const vadx_ft_view *out, int F, int tiles, void *stream, int arithmetic, void *range_flag) {
    VADX_REQUIRE(in && in->ptr && out && out->ptr && w_ih && w_hh && b_ih && b_hh && F > 0 && tiles > 0, "vadx_dfsmn_lstm_f: bad argument");
    VADX_REQUIRE(arithmetic == VADX_ARITH_AUTO || arithmetic == VADX_ARITH_F32 || arithmetic == VADX_ARITH_BF16X3 ||
                 (arithmetic == VADX_ARITH_F16X2 && range_flag),
                 "vadx_dfsmn_lstm_f: arithmetic=%d (F32, BF16X3, or F16X2 with two device words for the range flag)", arithmetic);
    VADX_REQUIRE(in->c == 40 ? (ln && ln->stats && ln->w && ln->b) : !(ln && ln->stats),
                 "vadx_dfsmn_lstm_f: the 40-channel (CepsUnit) LSTM takes a LayerNorm, the 4-channel one does not");
    LstmFArgs p;
    p.in = mkview(in); p.ln = mkln(ln); p.out = mkvieww(out); p.F = F;
    for (int d = 0; d < 2; ++d) { p.w_ih[d] = w_ih[d]; p.w_hh[d] = w_hh[d]; p.b_ih[d] = b_ih[d]; p.b_hh[d] = b_hh[d]; }
    if (in->c == 4) hipLaunchKernelGGL(lstm_f_kernel<4>, dim3(tiles), dim3(128), 0, static_cast<hipStream_t>(stream), p);
    else if (in->c == 40 && arithmetic == VADX_ARITH_F16X2)
        hipLaunchKernelGGL(lstm_f_split_kernel<vadx::SchemeH2>, dim3(tiles < 1024 ? tiles : 1024), dim3(128), 0, static_cast<hipStream_t>(stream), p, tiles,
                           static_cast<unsigned *>(range_flag));
    else if (in->c == 40 && arithmetic != VADX_ARITH_F32)      // split products: persistent workgroups (each lane splits its weights once), four per CU
        hipLaunchKernelGGL(lstm_f_split_kernel<vadx::SchemeB3>, dim3(tiles < 1024 ? tiles : 1024), dim3(128), 0, static_cast<hipStream_t>(stream), p, tiles,
                           static_cast<unsigned *>(nullptr));
    else if (in->c == 40) hipLaunchKernelGGL(lstm_f_kernel<40>, dim3(tiles), dim3(128), 0, static_cast<hipStream_t>(stream), p);
    else { vadx::set_error("vadx_dfsmn_lstm_f: input channels must be 4 or 40"); return VADX_EINVAL; }
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}


extern "C" int vadx_dfsmn_alpha_scale(const float *in, float *out, int chunks, int nt, const float *w1, const float *b1,
                                      const float *w2, const float *b2, const float *pow_far, int frames, void *stream) {
    VADX_REQUIRE(in && out && w1 && b1 && w2 && b2 && chunks > 0 && nt > 0, "vadx_dfsmn_alpha_scale: bad argument");
    VADX_REQUIRE(!pow_far || (frames > 0 && frames <= nt * 16), "vadx_dfsmn_alpha_scale: frames out of range for the constant far power");
    const long long total = (long long)chunks * nt * 160 * 16;
    hipLaunchKernelGGL(alpha_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       in, out, nt, total, w1, b1, w2, b2, pow_far, frames);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_lstm_t(int which, const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2], const float *const w_hh[2],
                                 const float *const b_ih[2], const float *const b_hh[2], const float *wl, const float *bl,
                                 const vadx_ft_view *mul, const vadx_ft_view *out, int F, int frames, int chunks, void *stream) {
    return vadx_dfsmn_lstm_t_ex(which, in, ln, w_ih, w_hh, b_ih, b_hh, wl, bl, mul, out, F, frames, chunks, ((frames + 15) / 16) * 16, stream,
                                VADX_ARITH_F32, nullptr);
}

extern "C" int vadx_dfsmn_lstm_t_ex(int which, const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2], const float *const w_hh[2],
                                    const float *const b_ih[2], const float *const b_hh[2], const float *wl, const float *bl,
                                    const vadx_ft_view *mul, const vadx_ft_view *out, int F, int frames, int chunks, int frame_stride, void *stream,
                                    int arithmetic, void *range_flag) {
    VADX_REQUIRE(in && in->ptr && out && out->ptr && w_ih && w_hh && b_ih && b_hh && wl && bl, "vadx_dfsmn_lstm_t: bad argument");
    VADX_REQUIRE(arithmetic == VADX_ARITH_AUTO || arithmetic == VADX_ARITH_F32 || (arithmetic == VADX_ARITH_F16X2 && range_flag),
                 "vadx_dfsmn_lstm_t: arithmetic must be AUTO / F32, or F16X2 with two device words for the range flag");
    VADX_REQUIRE(F % 16 == 0 && frames > 0 && chunks > 0, "vadx_dfsmn_lstm_t: F must be a multiple of 16");
    VADX_REQUIRE(frame_stride % 4 == 0 && frame_stride >= ((frames + 3) / 4) * 4, "vadx_dfsmn_lstm_t: frame_stride must be a multiple of 4 covering the frames rounded up to 4");
    LstmTArgs p;
    p.tp = frame_stride;
    p.in = mkview(in); p.ln = mkln(ln); p.mul = mkview(mul); p.out = mkvieww(out); p.F = F; p.T = frames; p.nt = (frames + 15) / 16;
    p.wl = wl; p.bl = bl;
    for (int l = 0; l < 2; ++l) { p.w_ih[l] = w_ih[l]; p.w_hh[l] = w_hh[l]; p.b_ih[l] = b_ih[l]; p.b_hh[l] = b_hh[l]; }
    const unsigned grid = (unsigned)(chunks * (F / 16));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // 40 (not 48) staged output rows and no inter-layer buffer for the one-layer net: 51.2 KB, three workgroups per CU instead of two.
    // (Dropping the output staging block altogether -- the compute wave storing its 4-B outputs itself, 25.6 KB, four workgroups
    // per CU -- was measured: lstm_t launches 365 -> 516 ms per pass; forty scattered store instructions per step cost far more
    // than the fourth workgroup brings.)
    auto lds_bytes = [](int in, int outc, int hid, int ts, int layers) { return (size_t)(2 * in * (ts * 16 + 16) + 2 * outc * (ts * 16 + 16) + (layers > 1 ? 2 * hid * 16 : 0)) * sizeof(float); };
    VADX_DYN_LDS((lstm_t_kernel<40, 20, 1, 3, 1, 4, 40>), 64 * 1024);
    if (which == 0) {            // bottleneck ch_lstm: in 20, hidden 40, 2 layers, Linear 40->20, multiplied with `mul`
        VADX_REQUIRE(in->c == 20 && mul && mul->ptr, "vadx_dfsmn_lstm_t(0): in must have 20 channels and mul is required");
        p.out_ch = 20;
        constexpr int NTILE = 4;
        constexpr size_t lds2 = (size_t)(10 * 5 * 64 + 3 * 10 * 10 * 64 + 2 * 10 * 64 + 2 * 10 * 16 + NTILE * 2 * 40 * 16) * sizeof(float);
        p.nunits = (int)grid;
        // (a split-product form of this kernel -- one GEMM per layer and step over [h ; x ; 1], planes 0 / 1 of the weights as LDS fragments,
        // plane 2 of each layer's first two chunks in its waves' registers -- was built and measured: 27.6 ms per 3060 windows against
        // 26.4 with a dependent chain per row tile, 33.8 with the products tile-interleaved (184 B of scratch per lane in the step): 162 KB
        // of split weights do not fit beside the h exchange in LDS, and 80 resident registers leave the step no room.  Removed.)
        // fp16 x 2 (lstm_t2h_kernel): half of bf16 x 3's products and 110 KB of fragments -- it fits, and the step is no longer bound by
        // the matrix pipe.
        if (arithmetic == VADX_ARITH_F16X2) {
            constexpr size_t ldsh = (size_t)(10 * 2 * 2 + 10 * 3 * 2 + 2 * 2 * 2) * 1024 + 2 * 10 * 16 * 4 + NTILE * 2 * (2 * 1024 + 2 * 256);
            VADX_DYN_LDS((lstm_t2h_kernel<2, 0, NTILE>), ldsh);
            hipLaunchKernelGGL((lstm_t2h_kernel<2, 0, NTILE>), dim3((grid + NTILE - 1) / NTILE), dim3(128 * NTILE), ldsh, st, p,
                               static_cast<unsigned *>(range_flag));
        } else {
            VADX_DYN_LDS((lstm_t2_kernel<20, 40, 2, 0, NTILE>), lds2);
            hipLaunchKernelGGL((lstm_t2_kernel<20, 40, 2, 0, NTILE>), dim3((grid + NTILE - 1) / NTILE), dim3(128 * NTILE), lds2, st, p);
        }
    } else {                     // out_ch_lstm: in 40, hidden 20, 1 layer, Linear 20->40
        VADX_REQUIRE(in->c == 40, "vadx_dfsmn_lstm_t(1): in must have 40 channels");
        p.out_ch = 40;
        // (an fp16 x 2 form of this net -- a wave per 16-bin group, eight independent waves per workgroup sharing 29 KB of fragments, no
        // barrier in the step loop, four time steps per memory request -- was built and measured: 14 ms per 3840 windows, the same as this
        // kernel.  What-ifs on it: without transcendentals 0, without the loads - 3.4 ms, without the STORES - 7.4, without both - 10: the
        // 40-channel output leaves as 16-byte quarters of 64-byte rows whose other quarters follow 4, 8 and 12 steps later; whole rows
        // need 16 steps of staging = 40 KB per wave.  Removed; this kernel runs float32 MFMAs for every arithmetic.)
        hipLaunchKernelGGL((lstm_t_kernel<40, 20, 1, 3, 1, 4, 40>), dim3(grid), dim3(128), lds_bytes(40, 40, 20, 4, 1), st, p);
    }
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_ft_repack(const float *src, float *dst, int channels, int F, int frames, int chunks, int src_stride, int dst_stride,
                                    void *stream) {
    VADX_REQUIRE(src && dst && channels > 0 && F > 0 && frames > 0 && chunks > 0, "vadx_dfsmn_ft_repack: bad argument");
    VADX_REQUIRE(src_stride % 4 == 0 && dst_stride % 4 == 0 && src_stride >= frames && dst_stride >= frames,
                 "vadx_dfsmn_ft_repack: strides must be multiples of 4 that cover the frames");
    const int cp = (src_stride < dst_stride ? src_stride : dst_stride) / 4;
    const long long total = (long long)chunks * channels * F * cp;
    hipLaunchKernelGGL(ft_repack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst, channels, F,
                       frames, src_stride, dst_stride, total);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_istft(const float *y_ft, const float *basis_t, const float *wsum_inv, float *z_ws, float *out,
                                int chunks, int frames, void *stream) {
    VADX_REQUIRE(y_ft && basis_t && wsum_inv && z_ws && out && chunks > 0 && frames > 0, "vadx_dfsmn_istft: bad argument");
    const int nt = (frames + 15) / 16, L = (frames - 1) * 160 + 319 - 318;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(istft_gemm_kernel, dim3((unsigned)(chunks * nt)), dim3(256), 0, st, y_ft, basis_t, z_ws, nt, frames);
    VADX_HIP_TRY(hipGetLastError());
    const long long total = (long long)chunks * L;
    hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z_ws, wsum_inv, out, frames, L, total);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_vote(const float *vad, int batch, int windows, int frames, int look_backward, double speaking_score,
                               double silence_score, uint8_t *flags, void *stream) {
    VADX_REQUIRE(vad && flags && batch > 0 && windows > 0 && look_backward >= 1 && look_backward < frames, "vadx_dfsmn_vote: bad argument");
    hipLaunchKernelGGL(dfsmn_vote_kernel, dim3((batch + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), vad, batch,
                       windows, frames, look_backward, speaking_score, silence_score, flags);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_vote_ragged(const float *vad, int batch, int n_windows, int max_windows, const int32_t *win_first, int frames,
                                      int look_backward, double speaking_score, double silence_score, uint8_t *flags, int64_t flag_stride,
                                      void *stream) {
    VADX_REQUIRE(vad && win_first && flags, "vadx_dfsmn_vote_ragged: NULL argument (vad, win_first, flags)");
    VADX_REQUIRE(batch >= 1 && n_windows >= 1 && max_windows >= 1 && frames >= 1,
                 "vadx_dfsmn_vote_ragged: batch=%d n_windows=%d max_windows=%d frames=%d must be positive", batch, n_windows, max_windows, frames);
    VADX_REQUIRE(look_backward >= 1 && look_backward < frames, "vadx_dfsmn_vote_ragged: look_backward=%d outside [1, %d)", look_backward, frames);
    const int64_t need = (int64_t)max_windows * (frames - look_backward) + look_backward;
    VADX_REQUIRE(flag_stride >= need, "vadx_dfsmn_vote_ragged: flag_stride=%lld is below max_windows * (frames - look_backward) + look_backward = %lld",
                 (long long)flag_stride, (long long)need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    VADX_HIP_TRY(hipMemsetAsync(flags, 255, (size_t)batch * (size_t)flag_stride, st));
    hipLaunchKernelGGL(dfsmn_vote_ragged_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, vad, batch, n_windows, max_windows, win_first, frames,
                       look_backward, speaking_score, silence_score, flags, (long long)flag_stride);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

// carry length of a stream record, or 0 when the arguments describe no window grid
static int stream_carry(int window_len, int look_backward) {
    if (window_len < 1 || look_backward < 1 || look_backward >= (1 << 20)) return 0;
    const long long C = (long long)(look_backward + 1) * SFRAME;
    return C < window_len ? (int)C : 0;
}

extern "C" size_t vadx_dfsmn_stream_state_bytes(int streams, int window_len, int look_backward, int channels) {
    const int C = stream_carry(window_len, look_backward);
    return streams > 0 && C > 0 && (channels == 1 || channels == 2) ? srec_bytes(streams, C, channels) : 0;
}

extern "C" int vadx_dfsmn_stream_windows(const int16_t *near, const int16_t *far, int64_t row_stride, int streams, int n_slots, int windows,
                                         int window_len, int look_backward, const int32_t *slot, const uint8_t *reset, const void *state_in,
                                         void *state_out, int16_t *near_buf, int16_t *far_buf, void *stream) {
    VADX_REQUIRE(near && state_in && state_out && near_buf, "vadx_dfsmn_stream_windows: NULL argument (near, state_in, state_out, near_buf)");
    VADX_REQUIRE((far == nullptr) == (far_buf == nullptr), "vadx_dfsmn_stream_windows: far and far_buf must both be given or both be NULL");
    const int ch = far ? 2 : 1;
    VADX_REQUIRE(streams >= 1 && n_slots >= 1 && windows >= 1 && (long long)ch * streams * ((long long)windows + 1) < (1ll << 31),
                 "vadx_dfsmn_stream_windows: streams=%d n_slots=%d windows=%d must be positive", streams, n_slots, windows);
    const int C = stream_carry(window_len, look_backward);
    VADX_REQUIRE(C > 0, "vadx_dfsmn_stream_windows: window_len=%d look_backward=%d: look_backward must be at least 1 and leave a stride "
                        "(window_len - (look_backward + 1) * 320 > 0)", window_len, look_backward);
    VADX_REQUIRE(row_stride >= (int64_t)windows * (window_len - C), "vadx_dfsmn_stream_windows: row_stride=%lld must hold windows * stride = %lld samples",
                 (long long)row_stride, (long long)windows * (window_len - C));
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, srec_bytes(streams, C, ch)), "vadx_dfsmn_stream_windows: state_in and state_out overlap");
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0 &&
                 ((reinterpret_cast<uintptr_t>(near) | reinterpret_cast<uintptr_t>(far) | reinterpret_cast<uintptr_t>(near_buf) |
                   reinterpret_cast<uintptr_t>(far_buf)) & 1) == 0 && (reinterpret_cast<uintptr_t>(slot) & 3) == 0,
                 "vadx_dfsmn_stream_windows: the records must be 16-byte aligned, slot 4-byte, the sample and window buffers 2-byte");
    StreamWinArgs a;
    a.samples[0] = near; a.samples[1] = far; a.row_stride = (long long)row_stride;
    a.S = streams; a.n_slots = n_slots; a.k = windows; a.L = window_len; a.C = C; a.ch = ch; a.slot = slot; a.reset = reset;
    a.sin = static_cast<const unsigned char *>(state_in); a.sout = static_cast<unsigned char *>(state_out);
    a.wbuf[0] = near_buf; a.wbuf[1] = far_buf;
    hipLaunchKernelGGL(dfsmn_stream_windows_kernel, dim3((unsigned)(ch * streams * (windows + 1))), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_dfsmn_stream_vote(const float *vad, int streams, int n_slots, int windows, int frames, int look_backward, int channels,
                                      double speaking_score, double silence_score, const int32_t *slot, const uint8_t *reset,
                                      const void *state_in, void *state_out, uint8_t *flags, uint8_t *tail, void *stream) {
    VADX_REQUIRE(vad && state_in && state_out && flags && tail, "vadx_dfsmn_stream_vote: NULL argument (vad, state_in, state_out, flags, tail)");
    VADX_REQUIRE(streams >= 1 && n_slots >= 1 && windows >= 1 && frames >= 1,
                 "vadx_dfsmn_stream_vote: streams=%d n_slots=%d windows=%d frames=%d must be positive", streams, n_slots, windows, frames);
    VADX_REQUIRE(look_backward >= 1 && look_backward < frames, "vadx_dfsmn_stream_vote: look_backward=%d outside [1, %d)", look_backward, frames);
    VADX_REQUIRE(channels == 1 || channels == 2, "vadx_dfsmn_stream_vote: channels=%d must be 1 or 2", channels);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, srec_bytes(streams, (look_backward + 1) * SFRAME, channels)),
                 "vadx_dfsmn_stream_vote: state_in and state_out overlap");
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0 && (reinterpret_cast<uintptr_t>(slot) & 3) == 0,
                 "vadx_dfsmn_stream_vote: the records must be 16-byte aligned, slot 4-byte");
    StreamVoteArgs a;
    a.vad = vad; a.S = streams; a.n_slots = n_slots; a.k = windows; a.Tn = frames; a.lb = look_backward;
    a.speaking = speaking_score; a.silence_score = silence_score; a.slot = slot; a.reset = reset;
    a.sin = static_cast<const unsigned char *>(state_in); a.sout = static_cast<unsigned char *>(state_out);
    a.flags = flags; a.tail = tail;
    hipLaunchKernelGGL(dfsmn_stream_vote_kernel, dim3((streams + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}


extern "C" int vadx_dfsmn_mask_net(const vadx_dfsmn_mask_weights *w, const float *feat, int chunks, int frames, float *vad,
                                   void *stream) {
    VADX_REQUIRE(w && feat && vad && chunks > 0, "vadx_dfsmn_mask_net: NULL argument");
    VADX_REQUIRE(frames > 0 && frames <= 64, "vadx_dfsmn_mask_net: frames must be in [1, 64] (got %d)", frames);
    VADX_REQUIRE(w->hidden > 0 && w->hidden <= 128, "vadx_dfsmn_mask_net: hidden must be in [1, 128] (got %d)", w->hidden);
    VADX_REQUIRE(w->fsmn_hidden > 0 && w->fsmn_hidden <= 256, "vadx_dfsmn_mask_net: fsmn_hidden must be in [1, 256] (got %d)", w->fsmn_hidden);
    VADX_REQUIRE(w->layers >= 0 && w->layers <= 8, "vadx_dfsmn_mask_net: layers must be in [0, 8] (got %d)", w->layers);
    VADX_REQUIRE(w->lorder >= 1 && w->lorder <= 20, "vadx_dfsmn_mask_net: lorder must be in [1, 20] (got %d)", w->lorder);
    MaskArgs p;
    p.feat = feat; p.shift = w->shift; p.scale = w->scale; p.w1 = w->linear1_w; p.b1 = w->linear1_b; p.w3 = w->linear3_w; p.b3 = w->linear3_b;
    p.vad = vad; p.T = frames; p.H = w->hidden; p.Hp = (w->hidden + 15) & ~15; p.H2p = (w->fsmn_hidden + 15) & ~15;
    p.layers = w->layers; p.lorder = w->lorder;
    for (int l = 0; l < w->layers; ++l) { p.wl[l] = w->fsmn_linear_w[l]; p.bl[l] = w->fsmn_linear_b[l]; p.wp[l] = w->fsmn_project_w[l]; p.wc[l] = w->fsmn_conv_w[l]; }
    VADX_DYN_LDS(mask_net_kernel, MK_LDS_FLOATS * sizeof(float));
    hipLaunchKernelGGL(mask_net_kernel, dim3(chunks), dim3(512), MK_LDS_FLOATS * sizeof(float), static_cast<hipStream_t>(stream), p);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
