// fsmn.hip -- FSMN-VAD (FunASR encoder, explicit 4-cache signature) for gfx950.
// Reference: FSMN/Export_FSMN_VAD.py:75-101 (wrapper), FSMN/modeling_modified/encoder.py:78-83,
// 108-110,139-144,208-217 (encoder), FSMN/Inference_FSMN_VAD_ONNX.py:156-234 (host loop).
//
// One workgroup (8 waves) owns one analysis window (chunk) of one clip at a time and keeps every
// activation of a 64-frame (then 48-frame) tile in LDS, k-major [feature][frame]:
//   LFR x5 + CMVN (applied on the MFMA operand) -> Affine 400->A -> Affine A->L, ReLU
//   -> 4 x [ Linear L->128 | 20-tap causal depthwise FIR over (19-frame cache ++ tile) + skip |
//            Affine 128->L, ReLU ] -> Affine L->A' -> Affine A'->O -> softmax[:,0]
// All dense layers are f32-MFMA GEMMs with weights streamed from L2 (gemm_rt); the FIR, softmax,
// energy gate and the look-ahead vote are VALU/LDS work.  In "clips" mode the workgroup walks the
// overlapping windows of its clip in order, carrying the four FIR caches (global scratch = the
// reference's cache_0..3 tensors) and the adaptive noise floor exactly like the reference loop.
#include "rebalance.h"
#include "common.h"
#include "layers.h"
#include "layers_split.h"
#include "pack.h"

#include <math.h>
#include <string.h>

namespace vadx {
namespace fsmn {

constexpr int THREADS = 512, NW = 8;
constexpr int PROJ = 128, LORDER = 20, HIST = LORDER - 1, NLAYER = 4, NMEL = 80, LFR_M = 5;
constexpr int A_LD = 68;                 // bufA / bufB row stride: 64 frames + 4 (% 8 == 4)
constexpr int P_LD = 84;                 // bufP row stride: 1 unused + 19 history + 64 frames
constexpr int P_CUR = 20;                // first "current frame" column of bufP (16-B aligned)
constexpr int BUFA_ROWS = 256, BUFB_ROWS = 144;
constexpr int BUFA = BUFA_ROWS * A_LD, BUFB = BUFB_ROWS * A_LD, BUFP = PROJ * P_LD;
// The small block behind the tile buffers (Small<AR> finds it), in floats: ps[128] a window's P(silence) | red[512] partial results of the
// softmax and the gate | sc[128] the gate's 0 / 1 per frame | cnt[256] the vote's look-ahead counts
constexpr int SMALL = 1024, SM_PS = 0, SM_RED = 128, SM_SC = 640, SM_CNT = 768;
constexpr int MAX_T = 128;               // frames per window of vadx_fsmn_run: ps and sc hold 128
// frames per window of the clips / ragged / stream loops.  The cap is historical: it dates from the first loop kernel, written for a 64- then a
// 48-frame tile, and no reason for it is on record; ps, sc and cnt would hold MAX_T, but the loops are validated up to 112 frames only.
constexpr int MAX_T_LOOP = 112;
constexpr int CACHE_FLOATS = NLAYER * PROJ * HIST;      // the four FIR caches of one clip or stream, [layer][128][19]
constexpr int LDS_FLOATS = BUFA + BUFB + BUFP + SMALL;

struct Dev {
    int A, L, A2, O, Ap, Lp, A2p, Op, T;
    float ratio;
    int off_in1, off_b1, off_mean, off_var, off_in2, off_b2;
    int off_lin[NLAYER], off_fir[NLAYER], off_aff[NLAYER], off_baff[NLAYER];
    int off_out1, off_bo1, off_out2, off_bo2, total;
    // split-product copies of the dense layers (layers_split.h): A fragments [n-tile][32-k chunk][np planes][QFRAG] of ONE arithmetic, the one
    // dims->arithmetic names (split_scheme.h: np = 3 for bf16 x 3, 2 for fp16 x 2, 0 = none: float32 MFMAs on the fragment-major matrices)
    int arith, np, off_flag;                        // off_flag: [sticky range flag, bits of the largest |x|, pad, pad] of the fp16 x 2 kernels
    int split_ok;                                   // 0: dims outside the split tile's LDS map (Ap, A2p <= 160, Lp, Op <= 256)
    int nch_A, nch_L, nch_A2;                       // 32-k chunks of an A- / L- / A2-wide input
    int q_in1, q_b1, q_mbar, q_in2, q_lin[NLAYER], q_aff[NLAYER], q_out1, q_out2;
};
constexpr int NCH_IN1 = 13;                         // 5 x 80 LFR features = 400 -> 13 chunks of 32 (k-groups 50, 51 read a row of zeros)

static int r16(int x) { return (x + 15) & ~15; }

static int derive(const vadx_fsmn_dims *c, Dev *d) {
    memset(d, 0, sizeof(*d));
    if (c->input_affine_dim <= 0 || c->linear_dim <= 0 || c->output_affine_dim <= 0 || c->output_dim <= 0 || c->frames <= 0) return -1;
    d->A = c->input_affine_dim; d->L = c->linear_dim; d->A2 = c->output_affine_dim; d->O = c->output_dim; d->T = c->frames;
    d->Ap = r16(d->A); d->Lp = r16(d->L); d->A2p = r16(d->A2); d->Op = r16(d->O);
    d->ratio = c->speech_2_noise_ratio;
    if (d->Ap > BUFB_ROWS || d->A2p > BUFB_ROWS || d->Lp > BUFA_ROWS || d->Op > BUFA_ROWS) return -1;
    int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 255) & ~255; return r; };      // every section on a 1 KiB boundary (a wave's fragment load = 1 KiB = 16 lines)
    d->off_in1 = take(d->Ap * 400); d->off_b1 = take(d->Ap); d->off_mean = take(400); d->off_var = take(400);
    d->off_in2 = take(d->Lp * d->Ap); d->off_b2 = take(d->Lp);
    for (int l = 0; l < NLAYER; ++l) {
        d->off_lin[l] = take(PROJ * d->Lp); d->off_fir[l] = take(PROJ * LORDER);
        d->off_aff[l] = take(d->Lp * PROJ); d->off_baff[l] = take(d->Lp);
    }
    d->off_out1 = take(d->A2p * d->Lp); d->off_bo1 = take(d->A2p);
    d->off_out2 = take(d->Op * d->A2p); d->off_bo2 = take(d->Op);
    d->nch_A = (d->Ap + 31) / 32; d->nch_L = (d->Lp + 31) / 32; d->nch_A2 = (d->A2p + 31) / 32;
    d->split_ok = d->Ap <= 160 && d->A2p <= 160 && d->Lp <= 256 && d->Op <= 256;
    // AUTO = bf16 x 3 where the split tile fits (float32's exponent range: safe for a caller that never reads the range flag -- the score
    // gate's uint8 output has no NaN to be poisoned with), float32 MFMAs otherwise; fp16 x 2 is an explicit request (VADX_ARITH_F16X2) by
    // callers that run the range protocol, as FsmnEngine does; an explicit split arithmetic on dims outside the tile is refused
    d->arith = vadx::arith_internal(c->arithmetic, d->split_ok ? vadx::VADX_AR_B3 : vadx::VADX_AR_F32);
    if (d->arith < 0 || (d->arith != vadx::VADX_AR_F32 && !d->split_ok)) return -1;
    d->np = vadx::planes_of(d->arith);
    const int np = d->np;
    d->q_in1 = take(d->Ap / 16 * NCH_IN1 * np * QFRAG); d->q_b1 = take(d->Ap); d->q_mbar = take(NMEL);
    d->q_in2 = take(d->Lp / 16 * d->nch_A * np * QFRAG);
    for (int l = 0; l < NLAYER; ++l) {
        d->q_lin[l] = take(PROJ / 16 * d->nch_L * np * QFRAG);
        d->q_aff[l] = take(d->Lp / 16 * (PROJ / 32) * np * QFRAG);
    }
    d->q_out1 = take(d->A2p / 16 * d->nch_L * np * QFRAG);
    d->q_out2 = take(d->Op / 16 * d->nch_A2 * np * QFRAG);
    d->off_flag = take(4);
    d->total = o;
    return 0;
}

// One tile of MTT*16 frames starting at frame f0 (nvalid of them inside the chunk).
//   lm     : this chunk's log-mel [T][80] (global)
//   cin/cout: FIR caches of this stream, [layer][128][19] (global); cout may alias cin
//   ps     : LDS, receives P(silence) for frames f0 .. f0+nvalid-1
template <int MTT>
__device__ __forceinline__ void tile(const Dev &d, const float *__restrict__ Pk, const float *__restrict__ lm,
                                     int f0, int nvalid, const float *const *cin, float *const *cout,
                                     float *bufA, float *bufB, float *bufP, float *ps, float *red) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));          // per tile: nothing derived from the thread index is hoisted out of the tile / window loops
    constexpr int NF = MTT * 16;

    // ---- stage log-mel with LFR edge replication: bufB[mel][c] = lm[clamp(f0 + c - 2, 0, T-1)][mel]
    {   // batches of four loads per thread in flight (the index is always clamped into the chunk)
        constexpr int NE = (NF + 4) * NMEL, NIT = (NE + THREADS - 1) / THREADS;
        for (int u0 = 0; u0 < NIT; u0 += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = min(tid + THREADS * (u0 + u), NE - 1), c = e / NMEL, mel = e - c * NMEL;
                int fr = f0 + c - 2;
                fr = fr < 0 ? 0 : (fr > d.T - 1 ? d.T - 1 : fr);
                // read-once stream: non-temporal, so that it does not push the weight set (1.67 MB, re-read by every tile) and the FIR
                // caches (rewritten by every tile) out of the 4 MB L2 of the XCD
                v[u] = __builtin_nontemporal_load((vadx::global_f32_ptr)(lm + (size_t)fr * NMEL + mel));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + THREADS * (u0 + u), c = e / NMEL, mel = e - c * NMEL;
                if (e < NE) bufB[mel * A_LD + c] = v[u];
            }
        }
    }
    __syncthreads();

    LayerArgs a;
    // in_linear1: K = 5 passes x 80 (LFR concat: frame offset j -> column offset j), CMVN on the operand
    a = LayerArgs{Pk + d.off_in1, 400, d.Ap / 16, LFR_M, NMEL / 16, NMEL, 1, Pk + d.off_b1, 0,
                  bufB, A_LD, 0, bufP, A_LD, 0, Pk + d.off_mean, Pk + d.off_var, bufA};      // bufA is idle: K-split scratch
    layer<MTT, true>(a);
    __syncthreads();
    // FIR caches: the five values a thread carries into bufP's history columns are requested one layer EARLY (layer 0's before in_linear2,
    // layer l + 1's before layer l's linear), so the round trip to the global cache hides behind a GEMM instead of opening every layer
    constexpr int NH = (PROJ * HIST + THREADS - 1) / THREADS;
    auto cache_fetch = [&](int l, float (&hv)[NH]) {
#pragma unroll
        for (int u = 0; u < NH; ++u) { const int e = tid + THREADS * u; hv[u] = ldg1(cin[l] + (e < PROJ * HIST ? e : PROJ * HIST - 1)); }
    };
    float hv[NH];
    cache_fetch(0, hv);
    // in_linear2 + ReLU
    a = LayerArgs{Pk + d.off_in2, d.Ap, d.Lp / 16, 1, d.Ap / 16, 0, 0, Pk + d.off_b2, 1,
                  bufP, A_LD, 0, bufA, A_LD, 0, nullptr, nullptr};
    layer<MTT, false>(a);
    __syncthreads();

    for (int l = 0; l < NLAYER; ++l) {
        // history columns 1..19 of bufP <- cache (previous tile / previous chunk)
        {
#pragma unroll
            for (int u = 0; u < NH; ++u) {
                const int e = tid + THREADS * u, ch = e / HIST, h = e - ch * HIST;
                if (e < PROJ * HIST) bufP[ch * P_LD + 1 + h] = hv[u];
            }
            cache_fetch(l + 1 < NLAYER ? l + 1 : l, hv);      // next layer's values (the last iteration's request is unused)
        }
        a = LayerArgs{Pk + d.off_lin[l], d.Lp, PROJ / 16, 1, d.Lp / 16, 0, 0, nullptr, 0,
                      bufA, A_LD, 0, bufP, P_LD, P_CUR, nullptr, nullptr};
        layer<MTT, false>(a);
        __syncthreads();
        {   // FIR + skip: thread = (channel, quarter of the tile's frames)
            const int ch = tid >> 2, fq = tid & 3;
            constexpr int FPT = NF / 4;
            const float *wf = Pk + d.off_fir[l] + ch * LORDER;
            float w[LORDER];
#pragma unroll
            for (int k = 0; k < LORDER; ++k) w[k] = ldg1(wf + k);
            const float *seq = bufP + ch * P_LD + 1 + fq * FPT;       // seq[s], s = t + k
            float win[FPT + HIST];
#pragma unroll
            for (int s = 0; s < FPT + HIST; ++s) win[s] = seq[s];
#pragma unroll
            for (int t = 0; t < FPT; ++t) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < LORDER; ++k) s = fmaf(w[k], win[t + k], s);
                bufB[ch * A_LD + fq * FPT + t] = win[t + HIST] + s;
            }
            // new cache = last 19 entries of (history ++ valid frames)
            for (int e = tid; e < PROJ * HIST; e += THREADS) {
                const int c2 = e / HIST, h = e - c2 * HIST;
                stg1(cout[l] + e, bufP[c2 * P_LD + 1 + nvalid + h]);
            }
        }
        __syncthreads();
        a = LayerArgs{Pk + d.off_aff[l], PROJ, d.Lp / 16, 1, PROJ / 16, 0, 0, Pk + d.off_baff[l], 1,
                      bufB, A_LD, 0, bufA, A_LD, 0, nullptr, nullptr};
        layer<MTT, false>(a);
        __syncthreads();
    }
    a = LayerArgs{Pk + d.off_out1, d.Lp, d.A2p / 16, 1, d.Lp / 16, 0, 0, Pk + d.off_bo1, 0,
                  bufA, A_LD, 0, bufB, A_LD, 0, nullptr, nullptr, bufP};                      // bufP is idle: K-split scratch
    layer<MTT, false>(a);
    __syncthreads();
    a = LayerArgs{Pk + d.off_out2, d.A2p, d.Op / 16, 1, d.A2p / 16, 0, 0, Pk + d.off_bo2, 0,
                  bufB, A_LD, 0, bufA, A_LD, 0, nullptr, nullptr};
    layer<MTT, false>(a);
    __syncthreads();

    // ---- softmax over the O logits of each frame, keep class 0: thread = (part 0..7, frame 0..63)
    {
        const int m = tid & 63, part = tid >> 6;
        float mx = -INFINITY;
        if (m < NF) for (int n = part; n < d.O; n += NW) mx = fmaxf(mx, bufA[n * A_LD + m]);
        red[part * 64 + m] = mx;
        __syncthreads();
        float gm = red[m];
#pragma unroll
        for (int p2 = 1; p2 < NW; ++p2) gm = fmaxf(gm, red[p2 * 64 + m]);
        __syncthreads();
        float sm = 0.f;
        if (m < NF) for (int n = part; n < d.O; n += NW) sm += expf(bufA[n * A_LD + m] - gm);
        red[part * 64 + m] = sm;
        __syncthreads();
        if (part == 0 && m < nvalid) {
            float tot = 0.f;
#pragma unroll
            for (int p2 = 0; p2 < NW; ++p2) tot += red[p2 * 64 + m];
            ps[f0 + m] = expf(bufA[m] - gm) / tot;
        }
        __syncthreads();
    }
}


// ---- the same tile on bf16 x 3 split products (layers_split.h) ---------------------------------------------------------------------
// Every dense layer runs as six v_mfma_f32_16x16x32_bf16 per K = 32 step on exactly split float32 operands (6/16 of the f32-MFMA matrix
// time, float32-class accuracy).  Activations that feed a GEMM live in LDS as three bf16 planes [k / 8][frame][8]; the two float32
// buffers that remain are the FIR's input P [128][history ++ frames] and the softmax's logits.
//   * CMVN: the reference's (x + mean) * var on the LFR features moves into the first layer, W1' = W1 var, b1' = b1 + W1' (mean - mbar),
//     evaluated in double on the host; the staged log-mel is pre-centred with mbar = the centre LFR position's means (one float32
//     add), so that the products keep the magnitude of centred features.  Re-association only.
//   * the FIR thread owns four consecutive channels x four frames, so its outputs leave as one 8-byte store per plane and frame.
// LDS map (bytes), 160 KB with the small block -- tensors of one phase never overlap (H = planes of an A-wide tensor padded to 160
// channels, HL = planes of an L-wide tensor [256][64], P = float32 [128][84], FO = FIR output planes [128][64]):
//   in1: LM @61440 -> H1 @0        in2: H1 @0 -> HL @61440 ("mid")
//   even layer: HL mid -> P @0 -> FO @110592 -> HL @0 ("low")         odd layer: HL low -> P @98304 -> FO @0 -> HL mid
//   out1: HL mid -> H2 @0          out2: H2 @0 -> logits f32 [256][68] @61440
constexpr int SQ_H = 0, SQ_LM = 61440, SQ_HLM = 61440, SQ_HLL = 0, SQ_PE = 0, SQ_PO = 98304, SQ_FOH = 110592, SQ_FOL = 0, SQ_LOG = 61440;
constexpr int SQ_ARENA = 159744, SQ_LDS_BYTES = SQ_ARENA + SMALL * 4;
static_assert(SQ_HLM + 256 * 64 * 6 <= SQ_ARENA && SQ_FOH + 128 * 64 * 6 <= SQ_ARENA && SQ_PO + BUFP * 4 <= SQ_FOH + 128 * 64 * 6 &&
              SQ_LOG + 256 * A_LD * 4 <= SQ_ARENA && SQ_LM + 11 * 80 * 16 * 3 <= SQ_ARENA && 160 * 64 * 6 <= SQ_HLM && SQ_LDS_BYTES <= 160 * 1024,
              "split tile LDS map");

// The small block of a workgroup's LDS (layout at SMALL): behind the float32 tile's three buffers, or behind the split tile's arena.
// AR: the arithmetic of the dense layers (split_scheme.h: 0 float32 MFMAs, 1 bf16 x 3, 2 fp16 x 2)
template <int AR>
struct Small {
    float *ps, *red, *sc, *cnt;
    __device__ __forceinline__ explicit Small(float *lds) {
        float *base = AR != vadx::VADX_AR_F32 ? reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(lds) + SQ_ARENA) : lds + BUFA + BUFB + BUFP;
        ps = base + SM_PS; red = base + SM_RED; sc = base + SM_SC; cnt = base + SM_CNT;
    }
};

template <typename SC, int MTT>
__device__ __forceinline__ void tile_split(const Dev &d, const float *__restrict__ Pk, const float *__restrict__ lm,
                                           int f0, int nvalid, const float *const *cin, float *const *cout,
                                           unsigned char *smem, float *ps, float *red, float &amax) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    constexpr int NP = SC::NP;
    constexpr int NF = MTT * 16, NCL = NF + 16;             // columns of a plane row: frames (log-mel: + LFR context)
    const int lane = tid & 63, i = lane & 15;
    auto grp_pl = [](int kgrps, int ncol) { return kgrps * ncol * 16; };      // bytes of one plane

    // A layer's last 32-k chunk reads four k-groups whatever the tensor's width: k-groups kg0 .. kg1 - 1 of the NP planes [kg1][NF][8] at
    // `base` lie beyond the padded width (Ap, Lp or A2p, multiples of 16 but not of 32), no layer writes them, and what they overlap in the
    // LDS map (float32 P and logits, other tensors' planes) read as fp16 / bf16 can be Inf or NaN -- the weights there are zero, the
    // operand must be finite.  Called by every thread before the layer that writes the tensor (the region is free then, and P / FO of the
    // next layers overwrite it again: once per tile would not do).  Nothing to do when the width is a multiple of 32.
    auto zero_rows = [&](unsigned char *base, int kg0, int kg1) {
        const int pl = grp_pl(kg1, NF), n = (kg1 - kg0) * NF;
        for (int e = tid; e < NP * n; e += THREADS) {
            const int p = e / n, r = e - p * n;
            *reinterpret_cast<f32x4 *>(base + p * pl + (kg0 * NF + r) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    // ---- zero rows: k-groups of the A-wide tensor beyond Ap, the log-mel's row 10
    {
        zero_rows(smem + SQ_H, d.Ap / 8, 4 * d.nch_A);
        for (int e = tid; e < NP * NCL; e += THREADS) {
            const int p = e / NCL, c = e - p * NCL;
            *reinterpret_cast<f32x4 *>(smem + SQ_LM + p * grp_pl(11, NCL) + (10 * NCL + c) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    // ---- stage log-mel with LFR edge replication, pre-centred, as planes: column c = frame clamp(f0 + c - 2), item = (column, 4 mels)
    {
        constexpr int NE = (NF + 4) * (NMEL / 4), NIT = (NE + THREADS - 1) / THREADS;
        f32x4 v[NIT];
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int e = min(tid + THREADS * u, NE - 1), c = e / (NMEL / 4), mg = e - c * (NMEL / 4);
            int fr = f0 + c - 2;
            fr = fr < 0 ? 0 : (fr > d.T - 1 ? d.T - 1 : fr);
            v[u] = __builtin_nontemporal_load((vadx::global_f32x4_ptr)(lm + (size_t)fr * NMEL + 4 * mg));
        }
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int e = tid + THREADS * u, c = e / (NMEL / 4), mg = e - c * (NMEL / 4);
            if (e < NE) {
                const f32x4 x = v[u] + ldg4(Pk + d.q_mbar + 4 * mg);
                u32x2 pp[NP];
                SC::split4(x, pp, amax);
                unsigned char *dp = smem + SQ_LM + ((mg >> 1) * NCL + c) * 16 + (mg & 1) * 8;
#pragma unroll
                for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x2 *>(dp + p * grp_pl(11, NCL)) = pp[p];
            }
        }
    }
    __syncthreads();

    auto plain = [&](int ncol) { return [=](int kgrp, int mt) { return (kgrp * ncol + mt * 16 + i) * 16; }; };
    QLayerArgs a;
    // in_linear1: K = 5 LFR positions x 80 mels = 50 k-groups; k-group G = (position j = G / 10, mel group G % 10) reads column + j
    a = QLayerArgs{Pk + d.q_in1, d.Ap / 16, NCH_IN1, Pk + d.q_b1, 0, smem + SQ_LM, grp_pl(11, NCL), smem + SQ_H, grp_pl(4 * d.nch_A, NF), NF, nullptr};
    qlayer<SC, MTT, true>(a, [=](int G, int mt) { const int j = G / 10, mg = G - 10 * j; return G < 50 ? (mg * NCL + mt * 16 + i + j) * 16 : (10 * NCL + mt * 16 + i) * 16; }, amax);
    __syncthreads();
    constexpr int NH = (PROJ * HIST + THREADS - 1) / THREADS;
    auto cache_fetch = [&](int l, float (&hv)[NH]) {
#pragma unroll
        for (int u = 0; u < NH; ++u) { const int e = tid + THREADS * u; hv[u] = ldg1(cin[l] + (e < PROJ * HIST ? e : PROJ * HIST - 1)); }
    };
    float hv[NH];
    cache_fetch(0, hv);
    // in_linear2 + ReLU
    zero_rows(smem + SQ_HLM, d.Lp / 8, 4 * d.nch_L);
    a = QLayerArgs{Pk + d.q_in2, d.Lp / 16, d.nch_A, Pk + d.off_b2, 1, smem + SQ_H, grp_pl(4 * d.nch_A, NF), smem + SQ_HLM, grp_pl(4 * d.nch_L, NF), NF, nullptr};
    qlayer<SC, MTT, true>(a, plain(NF), amax);
    __syncthreads();

    for (int l = 0; l < NLAYER; ++l) {
        const bool even = (l & 1) == 0;
        unsigned char *HLin = smem + (even ? SQ_HLM : SQ_HLL), *HLout = smem + (even ? SQ_HLL : SQ_HLM);
        float *bufP = reinterpret_cast<float *>(smem + (even ? SQ_PE : SQ_PO));
        unsigned char *FO = smem + (even ? SQ_FOH : SQ_FOL);
        {   // history columns 1..19 of P <- cache (previous tile / previous chunk)
#pragma unroll
            for (int u = 0; u < NH; ++u) {
                const int e = tid + THREADS * u, ch = e / HIST, h = e - ch * HIST;
                if (e < PROJ * HIST) bufP[ch * P_LD + 1 + h] = hv[u];
            }
            cache_fetch(l + 1 < NLAYER ? l + 1 : l, hv);
        }
        a = QLayerArgs{Pk + d.q_lin[l], PROJ / 16, d.nch_L, nullptr, 0, HLin, grp_pl(4 * d.nch_L, NF), reinterpret_cast<unsigned char *>(bufP), P_CUR, P_LD, nullptr};
        qlayer<SC, MTT, false>(a, plain(NF), amax);
        // the FIR taps of this thread's four channels (80 floats) are requested BEFORE the barrier: their L2 round trip hides behind the
        // wait for the slowest wave of the GEMM instead of opening the FIR (per channel: load, wait, 80 FMAs -- four times in a row)
        const int cg = tid >> 4, fg = tid & 15;
        f32x4 fw[4][LORDER / 4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k4 = 0; k4 < LORDER / 4; ++k4) fw[c][k4] = ldg4(Pk + d.off_fir[l] + (4 * cg + c) * LORDER + 4 * k4);
        __syncthreads();
        {   // FIR + skip: thread = (4 consecutive channels, 4 frames); the four channels of a frame leave as one 8-byte store per plane
            if (fg < NF / 4) {
                f32x4 o[4];                                               // o[t][c]
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int ch = 4 * cg + c;
                    float w[LORDER], v[24];
#pragma unroll
                    for (int k4 = 0; k4 < LORDER / 4; ++k4) {
                        const f32x4 w4 = fw[c][k4];
                        w[4 * k4] = w4[0]; w[4 * k4 + 1] = w4[1]; w[4 * k4 + 2] = w4[2]; w[4 * k4 + 3] = w4[3];
                    }
                    const float *row = bufP + ch * P_LD + 4 * fg;         // v[1 + s] = seq[s] of the f32 tile (column 1 + 4 fg + s)
#pragma unroll
                    for (int b4 = 0; b4 < 6; ++b4) {
                        const f32x4 x4 = *reinterpret_cast<const f32x4 *>(row + 4 * b4);
                        v[4 * b4] = x4[0]; v[4 * b4 + 1] = x4[1]; v[4 * b4 + 2] = x4[2]; v[4 * b4 + 3] = x4[3];
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        float s = 0.f;
#pragma unroll
                        for (int k = 0; k < LORDER; ++k) s = fmaf(w[k], v[1 + t + k], s);
                        o[t][c] = v[1 + t + HIST] + s;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    u32x2 pp[NP];
                    SC::split4(o[t], pp, amax);
                    unsigned char *dp = FO + ((cg >> 1) * NF + 4 * fg + t) * 16 + (cg & 1) * 8;
#pragma unroll
                    for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x2 *>(dp + p * grp_pl(PROJ / 8, NF)) = pp[p];
                }
            }
            for (int e = tid; e < PROJ * HIST; e += THREADS) {            // new cache = last 19 entries of (history ++ valid frames)
                const int c2 = e / HIST, h = e - c2 * HIST;
                stg1(cout[l] + e, bufP[c2 * P_LD + 1 + nvalid + h]);
            }
        }
        __syncthreads();
        zero_rows(HLout, d.Lp / 8, 4 * d.nch_L);
        a = QLayerArgs{Pk + d.q_aff[l], d.Lp / 16, PROJ / 32, Pk + d.off_baff[l], 1, FO, grp_pl(PROJ / 8, NF), HLout, grp_pl(4 * d.nch_L, NF), NF, nullptr};
        qlayer<SC, MTT, true>(a, plain(NF), amax);
        __syncthreads();
    }
    zero_rows(smem + SQ_H, d.A2p / 8, 4 * d.nch_A2);       // the A2-wide tensor (region 0 is free again)
    a = QLayerArgs{Pk + d.q_out1, d.A2p / 16, d.nch_L, Pk + d.off_bo1, 0, smem + SQ_HLM, grp_pl(4 * d.nch_L, NF), smem + SQ_H, grp_pl(4 * d.nch_A2, NF), NF, nullptr};
    qlayer<SC, MTT, true>(a, plain(NF), amax);
    __syncthreads();
    float *logits = reinterpret_cast<float *>(smem + SQ_LOG);
    a = QLayerArgs{Pk + d.q_out2, d.Op / 16, d.nch_A2, Pk + d.off_bo2, 0, smem + SQ_H, grp_pl(4 * d.nch_A2, NF), reinterpret_cast<unsigned char *>(logits), 0, A_LD, nullptr};
    qlayer<SC, MTT, false>(a, plain(NF), amax);
    __syncthreads();
    {   // softmax over the O logits of each frame, keep class 0 (as tile<>)
        const int m = tid & 63, part = tid >> 6;
        float mx = -INFINITY;
        if (m < NF) for (int n = part; n < d.O; n += NW) mx = fmaxf(mx, logits[n * A_LD + m]);
        red[part * 64 + m] = mx;
        __syncthreads();
        float gm = red[m];
#pragma unroll
        for (int p2 = 1; p2 < NW; ++p2) gm = fmaxf(gm, red[p2 * 64 + m]);
        __syncthreads();
        float sm = 0.f;
        if (m < NF) for (int n = part; n < d.O; n += NW) sm += expf(logits[n * A_LD + m] - gm);
        red[part * 64 + m] = sm;
        __syncthreads();
        if (part == 0 && m < nvalid) {
            float tot = 0.f;
#pragma unroll
            for (int p2 = 0; p2 < NW; ++p2) tot += red[p2 * 64 + m];
            ps[f0 + m] = expf(logits[m] - gm) / tot;
        }
        __syncthreads();
    }
}

// score gate of one chunk (FSMN/Export_FSMN_VAD.py:87-101): returns noisy_dB (NaN if no frame is "noise")
__device__ __forceinline__ float gate(const Dev &d, const float *ps, const float *__restrict__ db, float thr,
                                      float noise_db, unsigned char *__restrict__ score_out, float *__restrict__ psil_out,
                                      float *sc, float *red) {
    const int tid = threadIdx.x;
    float part_sum = 0.f, part_cnt = 0.f;
    if (tid < 128) {
        for (int t = tid; t < d.T; t += 128) {
            const float p = ps[t];
            float s;
            if (d.ratio > 1.0f) s = p + powf(p, d.ratio);
            else if (d.ratio < 1.0f) s = p + 1.0f;
            else s = p + p;
            const float e = db[t];
            const bool cond = (s <= thr) && (e >= noise_db);
            sc[t] = cond ? 1.f : 0.f;
            if (score_out) score_out[t] = cond ? 1 : 0;
            if (psil_out) psil_out[t] = p;
            if (!cond) { part_sum += e; part_cnt += 1.f; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { part_sum += __shfl_xor(part_sum, o); part_cnt += __shfl_xor(part_cnt, o); }
        if ((tid & 63) == 0) { red[(tid >> 6) * 2] = part_sum; red[(tid >> 6) * 2 + 1] = part_cnt; }
    }
    __syncthreads();
    const float tot = red[0] + red[2], cnt = red[1] + red[3];
    __syncthreads();
    return tot / cnt;                      // 0/0 -> NaN like torch's mean of an empty tensor
}

// One window: its tiles in order, P(silence) of its T frames into ps[0 .. T): Small<AR>::ps (T <= MAX_T), or global memory (a long window)
template <int AR>
__device__ __forceinline__ void run_chunk_to(const Dev &d, const float *Pk, const float *lm, const float *const *cin,
                                             float *const *cout, float *lds, float *ps, float &amax) {
    constexpr bool SPLIT = AR != vadx::VADX_AR_F32;
    typedef typename vadx::SchemeFor<AR>::type SC;
    float *bufA = lds, *bufB = lds + BUFA, *bufP = bufB + BUFB;
    const Small<AR> sm(lds);
    float *red = sm.red;
    unsigned char *smem = reinterpret_cast<unsigned char *>(lds);
    int f0 = 0;
    bool first = true;
    while (f0 < d.T) {
        const int left = d.T - f0;
        const float *const *ci = first ? cin : cout;         // later tiles continue from the updated cache
        if (SPLIT) {
            if (left > 48) tile_split<SC, 4>(d, Pk, lm, f0, left < 64 ? left : 64, ci, cout, smem, ps, red, amax), f0 += 64;
            else if (left > 32) tile_split<SC, 3>(d, Pk, lm, f0, left, ci, cout, smem, ps, red, amax), f0 += 48;
            else if (left > 16) tile_split<SC, 2>(d, Pk, lm, f0, left, ci, cout, smem, ps, red, amax), f0 += 32;
            else tile_split<SC, 1>(d, Pk, lm, f0, left, ci, cout, smem, ps, red, amax), f0 += 16;
        } else {
            if (left > 48) tile<4>(d, Pk, lm, f0, left < 64 ? left : 64, ci, cout, bufA, bufB, bufP, ps, red), f0 += 64;
            else if (left > 32) tile<3>(d, Pk, lm, f0, left, ci, cout, bufA, bufB, bufP, ps, red), f0 += 48;
            else if (left > 16) tile<2>(d, Pk, lm, f0, left, ci, cout, bufA, bufB, bufP, ps, red), f0 += 32;
            else tile<1>(d, Pk, lm, f0, left, ci, cout, bufA, bufB, bufP, ps, red), f0 += 16;
        }
        first = false;
    }
}

template <int AR>
__device__ __forceinline__ void run_chunk(const Dev &d, const float *Pk, const float *lm, const float *const *cin,
                                          float *const *cout, float *lds, float &amax) {
    run_chunk_to<AR>(d, Pk, lm, cin, cout, lds, Small<AR>(lds).ps, amax);
}

struct RunArgs {
    const float *logmel, *db;             // [B][T][80], [B][T]
    const float *cin[NLAYER]; float *cout[NLAYER];   // each [B][128][19]
    const float *thr, *noise_db;          // [B]
    unsigned char *score; float *noisy_db, *psil;    // [B][T], [B], [B][T] (psil optional)
};

// ORT-boundary equivalent: one chunk per stream, B independent streams.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_run_kernel(Dev d, const float *__restrict__ Pk, RunArgs r) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const float *cin[NLAYER]; float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) { cin[l] = r.cin[l] + (size_t)b * PROJ * HIST; cout[l] = r.cout[l] + (size_t)b * PROJ * HIST; }
    run_chunk<AR>(d, Pk, r.logmel + (size_t)b * d.T * NMEL, cin, cout, lds, amax);
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
    const Small<AR> sm(lds);
    const float noisy = gate(d, sm.ps, r.db + (size_t)b * d.T, r.thr[b], r.noise_db[b], r.score + (size_t)b * d.T,
                             r.psil ? r.psil + (size_t)b * d.T : nullptr, sm.sc, sm.red);
    if (threadIdx.x == 0) r.noisy_db[b] = noisy;
}

struct LoopArgs {
    int slide, lb;                        // slide_range, look_backward of the vote (>= 1)
    float thr, noise0, snr;               // one_minus_speech_threshold, initial noise floor (x0.1), SNR (x0.1)
    double speaking, silence_score;
};

struct ClipArgs {
    const float *logmel, *db;             // [B*W][T][80], [B*W][T]
    float *cache;                         // scratch [B][4][128][19]
    int W;                                // windows per clip
    LoopArgs lp;
    unsigned char *flags;                 // [B][W*slide + (T - slide)] silence flags
    float *noise_trace;                   // optional [B][W]
};

// One clip of the reference's while-loop (Inference_FSMN_VAD_ONNX.py:176-234) by one workgroup: W windows in order from zero caches (cbase,
// this clip's [4][128][19] scratch), the noise floor and the vote's `silence` carried from window to window, the plain rule on the tail of
// the last window.  logmel / db / noise_trace point at the clip's FIRST window, fl at its flags (W * slide + T - slide of them).
template <int AR>
__device__ __forceinline__ void clip_loop(const Dev &d, const float *__restrict__ Pk, const LoopArgs &c, const float *logmel, const float *db,
                                          float *cbase, int W, unsigned char *fl, float *noise_trace, float *lds, float &amax) {
    const int tid = threadIdx.x;
    const Small<AR> sm(lds);
    float *ps = sm.ps, *red = sm.red, *sc = sm.sc, *cnt = sm.cnt;
    for (int e = tid; e < CACHE_FLOATS; e += THREADS) cbase[e] = 0.f;
    __syncthreads();
    const float *cin[NLAYER]; float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) { cin[l] = cbase + l * PROJ * HIST; cout[l] = cbase + l * PROJ * HIST; }
    float noise = c.noise0;
    int silence = 1;                       // carried by thread 0
    for (int k = 0; k < W; ++k) {
        run_chunk<AR>(d, Pk, logmel + (size_t)k * d.T * NMEL, cin, cout, lds, amax);
        const float noisy = gate(d, ps, db + (size_t)k * d.T, c.thr, noise, nullptr, nullptr, sc, red);
        // look-ahead vote: cnt[i] = #{ j in [1,lb) : sc[i+j] != 0 }
        if (tid < c.slide) {
            float s = 0.f;
            for (int j = 1; j < c.lb; ++j) s += sc[tid + j];
            cnt[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            const double inv_lb = 1.0 / (double)c.lb;
            for (int i = 0; i < c.slide; ++i) {
                if (silence) {
                    if (sc[i] != 0.f) silence = !((1.0 + (double)cnt[i]) * inv_lb >= c.speaking);
                    else silence = 1;
                } else {
                    if (sc[i] != 1.f) silence = !((1.0 + (double)((c.lb - 1) - cnt[i])) * inv_lb <= c.silence_score);
                    else silence = 0;
                }
                fl[k * c.slide + i] = (unsigned char)silence;
            }
            if (k == W - 1)                // tail of the final chunk: plain rule (:223-234)
                for (int i = c.slide; i < d.T; ++i) {
                    silence = silence ? !(sc[i] != 0.f) : (sc[i] != 1.f);
                    fl[W * c.slide + (i - c.slide)] = (unsigned char)silence;
                }
        }
        if (noisy > 0.0f) noise = 0.5f * ((noise + noisy) + c.snr);
        if (noise_trace && tid == 0) noise_trace[k] = noise;
        __syncthreads();
    }
}

// Whole clips: the reference's while-loop (Inference_FSMN_VAD_ONNX.py:176-234), one workgroup per clip.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_clips_kernel(Dev d, const float *__restrict__ Pk, ClipArgs c) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const size_t w0 = (size_t)b * c.W;
    const int nflags = c.W * c.lp.slide + (d.T - c.lp.slide);
    clip_loop<AR>(d, Pk, c.lp, c.logmel + w0 * d.T * NMEL, c.db + w0 * d.T, c.cache + (size_t)b * CACHE_FLOATS, c.W,
                  c.flags + (size_t)b * nflags, c.noise_trace ? c.noise_trace + w0 : nullptr, lds, amax);
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

struct RaggedArgs {
    const float *logmel, *db;             // [n_windows][T][80], [n_windows][T]: the front-end over the gathered windows
    float *cache;                         // scratch [B][4][128][19]
    int batch, n_windows, max_windows;
    const int *win_first, *order;         // [B+1] prefix sum of the windows per clip; [B] launch order (optional)
    LoopArgs lp;
    unsigned char *flags; long long flag_stride;      // [B][flag_stride], 255-filled by the entry point before the launch
    float *noise_trace;                   // optional [n_windows]
};

// The same loop over a RAGGED batch: workgroup i serves clip order[i] (longest first, so that the long clips start first and the short ones
// fill in behind them), whose windows are win_first[b] .. win_first[b+1]-1 of the per-window buffers.  A table entry that does not describe
// windows inside the buffers returns before anything is read or written: the clip's row keeps the entry point's 255 fill.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_clips_ragged_kernel(Dev d, const float *__restrict__ Pk, RaggedArgs c) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = c.order ? c.order[blockIdx.x] : (int)blockIdx.x;
    if (b < 0 || b >= c.batch) return;
    const int first = c.win_first[b], last = c.win_first[b + 1];
    if (first < 0 || last <= first || last - first > c.max_windows || last > c.n_windows) return;
    clip_loop<AR>(d, Pk, c.lp, c.logmel + (size_t)first * d.T * NMEL, c.db + (size_t)first * d.T, c.cache + (size_t)b * CACHE_FLOATS,
                  last - first, c.flags + (size_t)b * c.flag_stride, c.noise_trace ? c.noise_trace + first : nullptr, lds, amax);
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

// ---- long windows: any T up to MAX_T_LONG frames (opt-in entry points; the kernels above are untouched) ---------------------------------
// What bounds T above is Small's ps / sc / cnt, a whole window's P(silence), gate bits and vote counts in LDS.  Here a window's ps and sc
// are rows of a global workspace (L2-resident: 8 bytes per frame), written and read back by the SAME workgroup around a barrier; the tile
// walk, the caches carried from tile to tile and the gate are the code above, given other pointers.  The vote needs no count per frame:
// one running count of the gate bits in [i, i + lb) moves along the window.
constexpr int MAX_T_LONG = VADX_FSMN_LONG_MAX_FRAMES;
constexpr int VOTE_CH = 256;             // frames per step of the vote: their gate bits are staged in `red`, their flags in `cnt`
static_assert(2 * VOTE_CH <= SM_SC - SM_RED && VOTE_CH <= (SMALL - SM_CNT) * 4 && NW <= SM_RED - SM_PS, "the long vote's staging in the small block");
static int long_row(int T) { return (T + 63) & ~63; }                   // floats of one ps or sc row
struct LongWs { float *base; int row; };                                 // [rows][2][row]: ps, sc

struct RunLongArgs { RunArgs r; LongWs ws; };

// fsmn_run_kernel for a window of any length: P(silence) goes straight to the caller's psil rows when they are asked for
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_run_long_kernel(Dev d, const float *__restrict__ Pk, RunLongArgs a) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const RunArgs &r = a.r;
    const float *cin[NLAYER]; float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) { cin[l] = r.cin[l] + (size_t)b * PROJ * HIST; cout[l] = r.cout[l] + (size_t)b * PROJ * HIST; }
    float *row = a.ws.base + (size_t)b * 2 * a.ws.row;
    float *ps = r.psil ? r.psil + (size_t)b * d.T : row;
    run_chunk_to<AR>(d, Pk, r.logmel + (size_t)b * d.T * NMEL, cin, cout, lds, ps, amax);
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
    __threadfence_block();                 // ps was written by other threads of this workgroup
    __syncthreads();
    const Small<AR> sm(lds);
    const float noisy = gate(d, ps, r.db + (size_t)b * d.T, r.thr[b], r.noise_db[b], r.score + (size_t)b * d.T, nullptr, row + a.ws.row, sm.red);
    if (threadIdx.x == 0) r.noisy_db[b] = noisy;
}

// clip_loop for windows of any length: ps and sc are this clip's workspace rows.  The vote's count of window frame i is
// #{ j in [1, lb) : sc[i+j] != 0 } = run - sc[i], run = the gate bits in [i, i + lb): exact small integers, the same value clip_loop sums.
// Thread 0 walks VOTE_CH frames at a time over bits staged in LDS (cur = sc[i], ent = sc[i + lb], the bit that enters the count).
template <int AR>
__device__ __forceinline__ void clip_loop_long(const Dev &d, const float *__restrict__ Pk, const LoopArgs &c, const float *logmel, const float *db,
                                               float *cbase, int W, unsigned char *fl, float *noise_trace, float *lds, float *ps, float *sc,
                                               float &amax) {
    const int tid = threadIdx.x;
    const Small<AR> sm(lds);
    float *red = sm.red, *cur = sm.red, *ent = sm.red + VOTE_CH, *wsum = sm.ps;
    unsigned char *out = reinterpret_cast<unsigned char *>(sm.cnt);
    for (int e = tid; e < CACHE_FLOATS; e += THREADS) cbase[e] = 0.f;
    __syncthreads();
    const float *cin[NLAYER]; float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) { cin[l] = cbase + l * PROJ * HIST; cout[l] = cbase + l * PROJ * HIST; }
    float noise = c.noise0;
    int silence = 1;                       // carried by thread 0
    for (int k = 0; k < W; ++k) {
        run_chunk_to<AR>(d, Pk, logmel + (size_t)k * d.T * NMEL, cin, cout, lds, ps, amax);
        __threadfence_block();             // ps, then sc: written by some threads of this workgroup, read by others
        __syncthreads();
        const float noisy = gate(d, ps, db + (size_t)k * d.T, c.thr, noise, nullptr, nullptr, sc, red);
        __threadfence_block();
        __syncthreads();
        {   // the count's first value: the gate bits of frames [0, lb)   (lb <= T - 1)
            float part = 0.f;
            for (int j = tid; j < c.lb; j += THREADS) part += sc[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
            if ((tid & 63) == 0) wsum[tid >> 6] = part;
        }
        float run = 0.f;                   // thread 0's
        const int nfl = k == W - 1 ? d.T : c.slide;          // the final window's tail follows the plain rule (:223-234)
        for (int i0 = 0; i0 < nfl; i0 += VOTE_CH) {
            const int n = min(VOTE_CH, nfl - i0);
            if (tid < n) {
                const int i = i0 + tid;
                cur[tid] = sc[i];
                ent[tid] = i + c.lb < d.T ? sc[i + c.lb] : 0.f;
            }
            __syncthreads();
            if (tid == 0) {
                if (i0 == 0)
                    for (int w = 0; w < NW; ++w) run += wsum[w];
                const double inv_lb = 1.0 / (double)c.lb;
                for (int u = 0; u < n; ++u) {
                    const float s = cur[u];
                    if (i0 + u < c.slide) {
                        const float cnt = run - s;
                        if (silence) {
                            if (s != 0.f) silence = !((1.0 + (double)cnt) * inv_lb >= c.speaking);
                            else silence = 1;
                        } else {
                            if (s != 1.f) silence = !((1.0 + (double)((c.lb - 1) - cnt)) * inv_lb <= c.silence_score);
                            else silence = 0;
                        }
                        run = cnt + ent[u];
                    } else {
                        silence = silence ? !(s != 0.f) : (s != 1.f);
                    }
                    out[u] = (unsigned char)silence;
                }
            }
            __syncthreads();
            if (tid < n) fl[(size_t)k * c.slide + i0 + tid] = out[tid];
        }
        if (noisy > 0.0f) noise = 0.5f * ((noise + noisy) + c.snr);
        if (noise_trace && tid == 0) noise_trace[k] = noise;
        __syncthreads();
    }
}

struct ClipLongArgs { RaggedArgs r; LongWs ws; };

// Whole clips of long windows, rectangular (win_first == NULL: max_windows windows for every clip) or ragged, one workgroup per clip.
// The table guard is fsmn_clips_ragged_kernel's.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_clips_long_kernel(Dev d, const float *__restrict__ Pk, ClipLongArgs a) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const RaggedArgs &c = a.r;
    const int b = c.order ? c.order[blockIdx.x] : (int)blockIdx.x;
    if (b < 0 || b >= c.batch) return;
    const int first = c.win_first ? c.win_first[b] : b * c.max_windows, last = c.win_first ? c.win_first[b + 1] : first + c.max_windows;
    if (first < 0 || last <= first || last - first > c.max_windows || last > c.n_windows) return;
    float *row = a.ws.base + (size_t)b * 2 * a.ws.row;
    clip_loop_long<AR>(d, Pk, c.lp, c.logmel + (size_t)first * d.T * NMEL, c.db + (size_t)first * d.T, c.cache + (size_t)b * CACHE_FLOATS,
                       last - first, c.flags + (size_t)b * c.flag_stride, c.noise_trace ? c.noise_trace + first : nullptr, lds, row,
                       row + a.ws.row, amax);
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

// ---- live streams: the same loop, k windows per call, everything it carries in a device record -----------------------------------------
// The record of S streams (include/vadx.h states the contract): caches f32 [S][4][128][19] | header u32 [S][8] | carry int16 [S][C],
// C = (look_backward + 1) * 160 = the samples two consecutive windows share.  Header words: 0 noise floor (f32 bits), 1 silence,
// 2 primed (the stream has a carry), 3 zero, 4-5 windows done (u64), 6-7 zero.  The window kernel owns words 2-3 and the carry, the
// stream kernel the caches and the other words; zero bytes = un-primed = the reset state (noise floor and silence take their initial
// values when an un-primed stream starts).
constexpr int HDR_WORDS = 8, H_NOISE = 0, H_SIL = 1, H_PRIMED = 2, H_DONE = 4;
static size_t rec_hdr(int S) { return (size_t)S * CACHE_FLOATS * sizeof(float); }
static size_t rec_carry(int S) { return rec_hdr(S) + (size_t)S * HDR_WORDS * 4; }
static size_t rec_bytes(int S, int C) { return rec_carry(S) + (size_t)S * C * sizeof(int16_t); }

struct WinArgs {
    const int16_t *samples; long long row_stride;   // [S][row_stride]: k * stride new samples (L + (k-1) * stride for an un-primed stream)
    int k, L, C;                                    // windows per tick, window length, carry length; stride = L - C
    const unsigned char *reset, *active;            // optional [S]
    const unsigned char *sin; unsigned char *sout;  // records
    size_t hdr, carry;                              // byte offsets of the header / carry sections
    int16_t *wbuf;                                  // [S * k][L]
};

// Window assembly (the slicing of Inference_FSMN_VAD_ONNX.py:162-167 for a stream that arrives in pieces): a stream's timeline of this tick
// is its carry followed by its new samples (no carry before the first tick); window j = timeline[j * stride, j * stride + L), the new carry
// = the timeline's last C samples.  One workgroup per (stream, window) plus one per stream for the carry; 16-byte runs throughout (C, stride
// and L are multiples of 8 samples).  An inactive stream keeps its carry and gets windows of zeros (the front-end runs over them; the
// stream kernel ignores the result).
__global__ __launch_bounds__(256) void fsmn_stream_windows_kernel(WinArgs a) {
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int s = blockIdx.x / (a.k + 1), j = blockIdx.x - s * (a.k + 1), tid = threadIdx.x;
    const unsigned *hin = reinterpret_cast<const unsigned *>(a.sin + a.hdr) + (size_t)s * HDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(a.sout + a.hdr) + (size_t)s * HDR_WORDS;
    const s16x8 *cin = reinterpret_cast<const s16x8 *>(a.sin + a.carry + (size_t)s * a.C * sizeof(int16_t));
    s16x8 *cout = reinterpret_cast<s16x8 *>(a.sout + a.carry + (size_t)s * a.C * sizeof(int16_t));
    s16x8 *win = reinterpret_cast<s16x8 *>(a.wbuf + ((size_t)s * a.k + (j < a.k ? j : 0)) * a.L);
    const int nc = a.C / 8, nl = a.L / 8, ns = (a.L - a.C) / 8;
    if (a.active && !a.active[s]) {
        if (j < a.k) {
            for (int v = tid; v < nl; v += 256) win[v] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        } else {
            for (int v = tid; v < nc; v += 256) cout[v] = cin[v];
            if (tid < 2) hout[H_PRIMED + tid] = hin[H_PRIMED + tid];
        }
        return;
    }
    const bool primed = hin[H_PRIMED] != 0 && !(a.reset && a.reset[s]);
    const s16x8 *smp = reinterpret_cast<const s16x8 *>(a.samples + (long long)s * a.row_stride);
    auto timeline = [&](int v) { return primed ? (v < nc ? cin[v] : smp[v - nc]) : smp[v]; };       // 8-sample run v
    if (j < a.k) {
        for (int v = tid; v < nl; v += 256) win[v] = timeline(j * ns + v);
    } else {
        for (int v = tid; v < nc; v += 256) cout[v] = timeline(a.k * ns + v);        // the timeline holds k * stride + C samples
        if (tid < 2) hout[H_PRIMED + tid] = tid == 0 ? 1u : 0u;
    }
}

struct StreamArgs {
    const float *logmel, *db;             // [S*k][T][80], [S*k][T]: the front-end over the window buffer
    const unsigned char *sin; unsigned char *sout; size_t hdr;
    const unsigned char *reset, *active;  // optional [S]
    int k, slide, lb, ntail;              // windows per tick, slide_range, look_backward of the vote (>= 1), tail flags (= look_backward)
    float thr, noise0, snr;
    double speaking, silence_score;
    unsigned char *flags, *tail;          // [S][k*slide], [S][ntail]
    float *noise_trace;                   // optional [S][k]
};

// One window of a live stream -- the loop body both stream kernels run, written once: the network over the window (run_chunk), the score
// gate, the look-ahead vote that continues `silence` and writes the window's `slide` flags to fl, the noise-floor update, the trace, and --
// on the stream's LAST window of this tick -- the tail: the plain rule on a COPY of silence (the carried value is the one the next tick's
// vote continues from).  noise and silence are the caller's carried values (silence is thread 0's); widx is the window's row in logmel /
// db / noise_trace.
template <int AR>
__device__ __forceinline__ void stream_window(const Dev &d, const float *__restrict__ Pk, const float *logmel, const float *db, size_t widx,
                                              const float *const *cin, float *const *cout, int slide, int lb, float thr, float snr,
                                              double speaking, double silence_score, unsigned char *fl, unsigned char *tl, bool last,
                                              float *noise_trace, float &noise, int &silence, float *lds, float &amax) {
    const int tid = threadIdx.x;
    const Small<AR> sm(lds);
    float *ps = sm.ps, *red = sm.red, *sc = sm.sc, *cnt = sm.cnt;
    run_chunk<AR>(d, Pk, logmel + widx * d.T * NMEL, cin, cout, lds, amax);
    const float noisy = gate(d, ps, db + widx * d.T, thr, noise, nullptr, nullptr, sc, red);
    // look-ahead vote: cnt[i] = #{ j in [1,lb) : sc[i+j] != 0 }
    if (tid < slide) {
        float v = 0.f;
        for (int j = 1; j < lb; ++j) v += sc[tid + j];
        cnt[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const double inv_lb = 1.0 / (double)lb;
        for (int i = 0; i < slide; ++i) {
            if (silence) {
                if (sc[i] != 0.f) silence = !((1.0 + (double)cnt[i]) * inv_lb >= speaking);
                else silence = 1;
            } else {
                if (sc[i] != 1.f) silence = !((1.0 + (double)((lb - 1) - cnt[i])) * inv_lb <= silence_score);
                else silence = 0;
            }
            fl[i] = (unsigned char)silence;
        }
        if (last) {                        // what the tail would read if the stream ended here: plain rule (:223-234)
            int st = silence;
            for (int i = slide; i < d.T; ++i) {
                st = st ? !(sc[i] != 0.f) : (sc[i] != 1.f);
                tl[i - slide] = (unsigned char)st;
            }
        }
    }
    if (noisy > 0.0f) noise = 0.5f * ((noise + noisy) + snr);
    if (noise_trace && tid == 0) noise_trace[widx] = noise;
    __syncthreads();
}

// fsmn_clips_kernel's window loop with its state (four caches, noise floor, silence) loaded from state_in and stored to state_out; one
// workgroup per stream.  state_in is only read: run_chunk reads the caches of a window's first tile from `cin` and everything later from
// `cout`, so window 0 points cin at state_in and nothing is copied.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_stream_kernel(Dev d, const float *__restrict__ Pk, StreamArgs c) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const float *cache_in = reinterpret_cast<const float *>(c.sin) + (size_t)s * CACHE_FLOATS;
    float *cache_out = reinterpret_cast<float *>(c.sout) + (size_t)s * CACHE_FLOATS;
    const unsigned *hin = reinterpret_cast<const unsigned *>(c.sin + c.hdr) + (size_t)s * HDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(c.sout + c.hdr) + (size_t)s * HDR_WORDS;
    unsigned char *fl = c.flags + (size_t)s * c.k * c.slide, *tl = c.tail + (size_t)s * c.ntail;
    if (c.active && !c.active[s]) {        // no audio this tick: the record passes through bit for bit, a reset request is ignored
        const unsigned *ci = reinterpret_cast<const unsigned *>(cache_in);
        unsigned *co = reinterpret_cast<unsigned *>(cache_out);
        for (int e = tid; e < CACHE_FLOATS; e += THREADS) co[e] = ci[e];
        if (tid < HDR_WORDS && (tid < H_PRIMED || tid >= H_DONE)) hout[tid] = hin[tid];
        for (int e = tid; e < c.k * c.slide; e += THREADS) fl[e] = 255;
        for (int e = tid; e < c.ntail; e += THREADS) tl[e] = 255;
        if (c.noise_trace) for (int e = tid; e < c.k; e += THREADS) c.noise_trace[(size_t)s * c.k + e] = __uint_as_float(0x7fc00000u);
        return;
    }
    const bool fresh = hin[H_PRIMED] == 0 || (c.reset && c.reset[s]);
    if (fresh) {                           // un-primed: zero caches (written to state_out, read back as window 0's input)
        for (int e = tid; e < CACHE_FLOATS; e += THREADS) cache_out[e] = 0.f;
        __syncthreads();
    }
    float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) cout[l] = cache_out + l * PROJ * HIST;
    float noise = fresh ? c.noise0 : __uint_as_float(hin[H_NOISE]);
    int silence = fresh ? 1 : (int)hin[H_SIL];                                    // carried by thread 0
    for (int k = 0; k < c.k; ++k) {
        const float *cin[NLAYER];
#pragma unroll
        for (int l = 0; l < NLAYER; ++l) cin[l] = (k == 0 && !fresh ? cache_in : cache_out) + l * PROJ * HIST;
        stream_window<AR>(d, Pk, c.logmel, c.db, (size_t)s * c.k + k, cin, cout, c.slide, c.lb, c.thr, c.snr, c.speaking, c.silence_score,
                          fl + k * c.slide, tl, k == c.k - 1, c.noise_trace, noise, silence, lds, amax);
    }
    if (tid == 0) {
        hout[H_NOISE] = __float_as_uint(noise);
        hout[H_SIL] = (unsigned)silence;
        const unsigned long long done = fresh ? 0ull : *reinterpret_cast<const unsigned long long *>(hin + H_DONE);
        *reinterpret_cast<unsigned long long *>(hout + H_DONE) = done + (unsigned long long)c.k;
        hout[H_DONE + 2] = 0u; hout[H_DONE + 3] = 0u;
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

// ---- ragged ticks: stream s advances by counts[s] windows, 0 <= counts[s] <= max_windows; the work is sum(counts) windows ------------------
// counts int32 [S] and win_first int32 [S + 1] (its prefix sum; n_windows = win_first[S]) describe the tick to both kernels; window j of
// stream s is row win_first[s] + j of window_buf and of everything the front-end makes of it.  A stream with count 0 owns no row.  The
// tables are the caller's: a stream whose entries do not describe rows inside the buffers counts as 0 and raises bit 1 of *status.
constexpr int STREAM_RAGGED_MAX_WINDOWS = 256;       // no kernel resource depends on a count (a loop bound, a row index): the cap of the Silero tick
constexpr unsigned STATUS_BAD_TABLE = 2u;

// counts[s] when the tables of stream s describe rows inside [0, n_windows), else -1
__device__ __forceinline__ int ragged_count(const int *counts, const int *win_first, int s, int n_windows, int max_windows) {
    const int n = counts[s], first = win_first[s], last = win_first[s + 1];
    return (n >= 0 && n <= max_windows && first >= 0 && last <= n_windows && last - first == n) ? n : -1;
}

struct WinRaggedArgs {
    const int16_t *samples; long long row_stride;   // [S][row_stride]: n_s * stride new samples (L + (n_s - 1) * stride without a carry)
    int S, n_windows, max_windows, L, C;
    const int *counts, *win_first, *win_stream;     // [S], [S + 1], [n_windows]: the stream of each window row
    const unsigned char *reset;                     // optional [S]
    const unsigned char *sin; unsigned char *sout;
    size_t hdr, carry;
    int16_t *wbuf;                                  // [n_windows][L]
    unsigned *status;
};

// fsmn_stream_windows_kernel's timeline rule with a count per stream: workgroup w < n_windows assembles window row w (stream win_stream[w],
// its window w - win_first[s]); workgroup n_windows + s writes stream s's new carry -- the last C samples of ITS timeline of n_s windows --
// or, for a stream without audio, copies the carry and the "has a carry" word bit for bit.  16-byte runs throughout.
__global__ __launch_bounds__(256) void fsmn_stream_windows_ragged_kernel(WinRaggedArgs a) {
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int w = blockIdx.x, tid = threadIdx.x;
    const bool is_win = w < a.n_windows;
    const int s = is_win ? a.win_stream[w] : w - a.n_windows;
    if (s < 0 || s >= a.S) return;                  // a window row nobody owns stays unwritten
    const int n = ragged_count(a.counts, a.win_first, s, a.n_windows, a.max_windows);
    const unsigned *hin = reinterpret_cast<const unsigned *>(a.sin + a.hdr) + (size_t)s * HDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(a.sout + a.hdr) + (size_t)s * HDR_WORDS;
    const s16x8 *cin = reinterpret_cast<const s16x8 *>(a.sin + a.carry + (size_t)s * a.C * sizeof(int16_t));
    s16x8 *cout = reinterpret_cast<s16x8 *>(a.sout + a.carry + (size_t)s * a.C * sizeof(int16_t));
    const int nc = a.C / 8, nl = a.L / 8, ns = (a.L - a.C) / 8;
    if (n <= 0) {
        if (!is_win) {
            for (int v = tid; v < nc; v += 256) cout[v] = cin[v];
            if (tid < 2) hout[H_PRIMED + tid] = hin[H_PRIMED + tid];
            if (n < 0 && tid == 0) atomicOr(a.status, STATUS_BAD_TABLE);
        }
        return;
    }
    const bool primed = hin[H_PRIMED] != 0 && !(a.reset && a.reset[s]);
    const s16x8 *smp = reinterpret_cast<const s16x8 *>(a.samples + (long long)s * a.row_stride);
    auto timeline = [&](int v) { return primed ? (v < nc ? cin[v] : smp[v - nc]) : smp[v]; };       // 8-sample run v
    if (is_win) {
        const int j = w - a.win_first[s];
        if (j < 0 || j >= n) return;                // the row table and win_first disagree: not this stream's row
        s16x8 *win = reinterpret_cast<s16x8 *>(a.wbuf + (size_t)w * a.L);
        for (int v = tid; v < nl; v += 256) win[v] = timeline(j * ns + v);
    } else {
        for (int v = tid; v < nc; v += 256) cout[v] = timeline(n * ns + v);          // the stream's timeline holds n * stride + C samples
        if (tid < 2) hout[H_PRIMED + tid] = tid == 0 ? 1u : 0u;
    }
}

struct StreamRaggedArgs {
    const float *logmel, *db;             // [n_windows][T][80], [n_windows][T]
    const unsigned char *sin; unsigned char *sout; size_t hdr;
    const unsigned char *reset;           // optional [S]
    const int *counts, *win_first, *order;          // [S], [S + 1], [S] launch order (optional)
    int S, n_windows, max_windows, slide, lb, ntail;
    float thr, noise0, snr;
    double speaking, silence_score;
    unsigned char *flags, *tail;          // [n_windows][slide], [S][ntail]
    float *noise_trace;                   // optional [n_windows]
    unsigned *status;
};

// fsmn_stream_kernel with a count per stream: workgroup i serves stream order[i] (most windows first, idle streams last) and runs
// stream_window n_s times over its own rows.  A stream without audio (count 0, or tables that lie) copies its caches and header bit for bit
// and reads 255 in its tail; it touches no flag or trace row.
template <int AR>
__global__ __launch_bounds__(THREADS, 2) void fsmn_stream_ragged_kernel(Dev d, const float *__restrict__ Pk, StreamRaggedArgs c) {
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int s = c.order ? c.order[blockIdx.x] : (int)blockIdx.x;
    if (s < 0 || s >= c.S) {
        if (tid == 0) atomicOr(c.status, STATUS_BAD_TABLE);
        return;
    }
    const int n = ragged_count(c.counts, c.win_first, s, c.n_windows, c.max_windows);
    const float *cache_in = reinterpret_cast<const float *>(c.sin) + (size_t)s * CACHE_FLOATS;
    float *cache_out = reinterpret_cast<float *>(c.sout) + (size_t)s * CACHE_FLOATS;
    const unsigned *hin = reinterpret_cast<const unsigned *>(c.sin + c.hdr) + (size_t)s * HDR_WORDS;
    unsigned *hout = reinterpret_cast<unsigned *>(c.sout + c.hdr) + (size_t)s * HDR_WORDS;
    unsigned char *tl = c.tail + (size_t)s * c.ntail;
    if (n <= 0) {
        const unsigned *ci = reinterpret_cast<const unsigned *>(cache_in);
        unsigned *co = reinterpret_cast<unsigned *>(cache_out);
        for (int e = tid; e < CACHE_FLOATS; e += THREADS) co[e] = ci[e];
        if (tid < HDR_WORDS && (tid < H_PRIMED || tid >= H_DONE)) hout[tid] = hin[tid];
        for (int e = tid; e < c.ntail; e += THREADS) tl[e] = 255;
        if (n < 0 && tid == 0) atomicOr(c.status, STATUS_BAD_TABLE);
        return;
    }
    const size_t first = (size_t)c.win_first[s];
    unsigned char *fl = c.flags + first * c.slide;
    const bool fresh = hin[H_PRIMED] == 0 || (c.reset && c.reset[s]);
    if (fresh) {
        for (int e = tid; e < CACHE_FLOATS; e += THREADS) cache_out[e] = 0.f;
        __syncthreads();
    }
    float *cout[NLAYER];
#pragma unroll
    for (int l = 0; l < NLAYER; ++l) cout[l] = cache_out + l * PROJ * HIST;
    float noise = fresh ? c.noise0 : __uint_as_float(hin[H_NOISE]);
    int silence = fresh ? 1 : (int)hin[H_SIL];                                    // carried by thread 0
    for (int k = 0; k < n; ++k) {
        const float *cin[NLAYER];
#pragma unroll
        for (int l = 0; l < NLAYER; ++l) cin[l] = (k == 0 && !fresh ? cache_in : cache_out) + l * PROJ * HIST;
        stream_window<AR>(d, Pk, c.logmel, c.db, first + k, cin, cout, c.slide, c.lb, c.thr, c.snr, c.speaking, c.silence_score,
                          fl + k * c.slide, tl, k == n - 1, c.noise_trace, noise, silence, lds, amax);
    }
    if (tid == 0) {
        hout[H_NOISE] = __float_as_uint(noise);
        hout[H_SIL] = (unsigned)silence;
        const unsigned long long done = fresh ? 0ull : *reinterpret_cast<const unsigned long long *>(hin + H_DONE);
        *reinterpret_cast<unsigned long long *>(hout + H_DONE) = done + (unsigned long long)n;
        hout[H_DONE + 2] = 0u; hout[H_DONE + 3] = 0u;
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

// frame energy in dB/10 of the prepped window (FSMN/Export_FSMN_VAD.py:93-97): one workgroup per window
__global__ void fsmn_energy_kernel(const int16_t *__restrict__ audio, long long row_stride, long long win_stride,
                                   int windows_per_clip, int window_len, int n_fft, int hop, int T,
                                   const float *__restrict__ means, float inv_ref, float *__restrict__ db) {
    const int widx = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int b = widx / windows_per_clip, w = widx - b * windows_per_clip;
    const int16_t *win = audio + (long long)b * row_stride + (long long)w * win_stride;
    const float mean = means[widx];
    const int nfr = (window_len - n_fft) / hop + 1;
    float *out = db + (size_t)widx * T;
    for (int f = wave; f < T; f += nw) {
        const int ff = f < nfr ? f : nfr - 1;          // last value repeated up to T frames
        float s = 0.f;
        // eight (sample, predecessor) pairs per lane are requested before any is used, unconditionally (clamped index, value selected
        // afterwards): the guarded predecessor load compiled to a branch plus a full wait -- one serialised round trip per sample.
        // Accumulation order per lane is unchanged (k ascending): the sums are bit-identical.
        for (int k0 = lane; k0 < n_fft; k0 += 64 * 8) {
            float xa[8], xb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = min(k0 + 64 * u, n_fft - 1), n = ff * hop + k;
                xa[u] = (float)win[n];
                xb[u] = (float)win[n > 0 ? n - 1 : 0];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = k0 + 64 * u, n = ff * hop + k;
                if (k < n_fft) {
                    const float a = __fsub_rn(xa[u], mean);
                    float y = a;
                    if (n > 0) y = __fsub_rn(a, __fmul_rn(0.97f, __fsub_rn(xb[u], mean)));
                    y = __fmul_rn(y, inv_ref);
                    s = fmaf(y, y, s);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) out[f] = log10f(s + 0.00002f);
    }
}

// Window mean AND frame energies in one pass over the PCM (round 6; replaces window_mean_kernel + fsmn_energy_kernel for the aligned case: the two
// read every window from memory once each, and the energy kernel visited every sample 3.2 times -- 512-sample frames at a hop of 160).
// One workgroup of 256 threads per window: a thread keeps its (up to) eight 16-byte runs of samples in registers, the workgroup sums them as
// integers (the mean, exactly as window_mean_kernel computes it), then every run contributes sum(y^2) of its eight prepped samples ONCE; four
// neighbouring lanes add up to a 32-sample granule, and a frame is sixteen consecutive granules (512 = 16 x 32, 160 = 5 x 32).
// Same formula as fsmn_energy_kernel, another summation order: the dB values agree to float32 rounding (1e-7 relative).
constexpr int ST_THREADS = 256, ST_MAXIT = 8, ST_MAXGRAN = (ST_THREADS * ST_MAXIT * 8) / 32;       // windows up to 16 384 samples
__global__ __launch_bounds__(ST_THREADS) void fsmn_stats_kernel(const int16_t *__restrict__ audio, long long row_stride, long long win_stride,
                                                                int windows_per_clip, int window_len, int T, float inv_ref,
                                                                float *__restrict__ means, float *__restrict__ db) {
    __shared__ float gran[ST_MAXGRAN];
    __shared__ long long wsum[ST_THREADS / 64];
    const int widx = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = widx / windows_per_clip, w = widx - b * windows_per_clip;
    const int16_t *win = audio + (long long)b * row_stride + (long long)w * win_stride;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const int nrun = window_len / 8;
    s16x8 x[ST_MAXIT];
    long long s = 0;
#pragma unroll
    for (int it = 0; it < ST_MAXIT; ++it) {
        const int r = it * ST_THREADS + tid;
        x[it] = *reinterpret_cast<const s16x8 *>(win + 8 * (r < nrun ? r : nrun - 1));
        if (r < nrun)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[it][e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    long long tot = 0;
#pragma unroll
    for (int k = 0; k < ST_THREADS / 64; ++k) tot += wsum[k];
    const float mean = (float)((double)tot / (double)window_len);
    if (tid == 0) means[widx] = mean;
#pragma unroll
    for (int it = 0; it < ST_MAXIT; ++it) {
        const int r = it * ST_THREADS + tid;
        // the sample in front of this run: the previous lane's last sample (the previous run), the first lane of a wave reads it from memory
        float prev = (float)__shfl_up((int)x[it][7], 1);
        if (lane == 0) prev = (float)win[r > 0 ? 8 * (r < nrun ? r : nrun - 1) - 1 : 0];
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = __fsub_rn((float)x[it][e], mean);
            float y = a;
            if (e > 0 || r > 0) y = __fsub_rn(a, __fmul_rn(0.97f, __fsub_rn(prev, mean)));
            y = __fmul_rn(y, inv_ref);
            acc = fmaf(y, y, acc);
            prev = (float)x[it][e];
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        if ((lane & 3) == 0 && r < nrun) gran[r >> 2] = acc;
    }
    __syncthreads();
    const int nfr = (window_len - 512) / 160 + 1;
    float *out = db + (size_t)widx * T;
    for (int f = tid; f < T; f += ST_THREADS) {
        const int ff = f < nfr ? f : nfr - 1;          // last value repeated up to T frames
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) e += gran[5 * ff + j];
        out[f] = log10f(e + 0.00002f);
    }
}

// Means and energies of LONG windows: above ST_MAXGRAN granules vadx_fsmn_window_stats falls back to one workgroup per window twice
// (window_mean_kernel: one wave; fsmn_energy_kernel: four waves, every sample 3.2 times), which leaves a single 10-minute window on one CU.
// Here the grid is (window, block): a sum kernel adds each block's samples into the window's 64-bit integer sum (integer atomics: exact,
// any order), then an energy kernel takes SL_FRAMES frames per workgroup.  The mean is window_mean_kernel's value bit for bit (exact sum,
// one rounding); a sample's y is fsmn_energy_kernel's expression; y^2 is summed per 32-sample granule by 32 lanes and a frame is sixteen
// granules, as in fsmn_stats_kernel.  Any alignment and any window_len >= 512: only granules inside a frame are formed.
constexpr int SL_THREADS = 256, SL_SUM = 16384, SL_FRAMES = 48, SL_GRAN = 5 * (SL_FRAMES - 1) + 16;
__global__ __launch_bounds__(SL_THREADS) void fsmn_long_sum_kernel(const int16_t *__restrict__ audio, long long row_stride, long long win_stride,
                                                                   int windows_per_clip, int window_len, unsigned long long *__restrict__ sums) {
    __shared__ long long wsum[SL_THREADS / 64];
    const int widx = blockIdx.x, tid = threadIdx.x;
    const int b = widx / windows_per_clip, w = widx - b * windows_per_clip;
    const int16_t *win = audio + (long long)b * row_stride + (long long)w * win_stride;
    const int n0 = blockIdx.y * SL_SUM, n1 = min(n0 + SL_SUM, window_len);
    long long s = 0;                       // 9.6 M samples x 32 767 does not fit 32 bits
    for (int n = n0 + tid; n < n1; n += SL_THREADS) s += win[n];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        long long tot = 0;
#pragma unroll
        for (int k = 0; k < SL_THREADS / 64; ++k) tot += wsum[k];
        atomicAdd(sums + widx, (unsigned long long)tot);      // two's complement: the wrapped sum of the blocks is the window's signed sum
    }
}

__global__ __launch_bounds__(SL_THREADS) void fsmn_long_energy_kernel(const int16_t *__restrict__ audio, long long row_stride, long long win_stride,
                                                                      int windows_per_clip, int window_len, int T, float inv_ref,
                                                                      const unsigned long long *__restrict__ sums, float *__restrict__ means,
                                                                      float *__restrict__ db) {
    __shared__ float gran[SL_GRAN];
    const int widx = blockIdx.x, tid = threadIdx.x, l = tid & 31, hw = tid >> 5;
    const int b = widx / windows_per_clip, w = widx - b * windows_per_clip;
    const int16_t *win = audio + (long long)b * row_stride + (long long)w * win_stride;
    const float mean = (float)((double)(long long)sums[widx] / (double)window_len);
    if (blockIdx.y == 0 && tid == 0) means[widx] = mean;
    const int nfr = (window_len - 512) / 160 + 1;
    const int f0 = blockIdx.y * SL_FRAMES, f1 = min(f0 + SL_FRAMES, T) - 1;          // this block's frames, f0 <= f1 < T
    const int ff0 = min(f0, nfr - 1), ff1 = min(f1, nfr - 1);                         // last value repeated up to T frames
    const int g0 = 5 * ff0, ng = 5 * (ff1 - ff0) + 16;                                // granules g0 .. g0 + ng - 1, ng <= SL_GRAN
    for (int gb = 0; gb < ng; gb += SL_THREADS / 32) {
        const int g = min(gb + hw, ng - 1), n = 32 * (g0 + g) + l;                   // n <= 160 (nfr - 1) + 511 < window_len
        const float xa = (float)win[n], xb = (float)win[n > 0 ? n - 1 : 0];
        const float a = __fsub_rn(xa, mean);
        float y = a;
        if (n > 0) y = __fsub_rn(a, __fmul_rn(0.97f, __fsub_rn(xb, mean)));
        y = __fmul_rn(y, inv_ref);
        float acc = __fmul_rn(y, y);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (l == 0 && gb + hw < ng) gran[g] = acc;
    }
    __syncthreads();
    float *out = db + (size_t)widx * T;
    for (int f = f0 + tid; f <= f1; f += SL_THREADS) {
        const int ff = min(f, nfr - 1);
        float e = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) e += gran[5 * (ff - ff0) + j];
        out[f] = log10f(e + 0.00002f);
    }
}

}  // namespace fsmn
}  // namespace vadx

using namespace vadx::fsmn;
using vadx::QFRAG;
namespace pack = vadx::pack;

extern "C" size_t vadx_fsmn_packed_floats(const vadx_fsmn_dims *dims) {
    Dev d;
    if (!dims || derive(dims, &d)) return 0;
    return (size_t)d.total;
}

extern "C" int vadx_fsmn_pack_host(const vadx_fsmn_dims *dims, const vadx_fsmn_weights_host *w_in, float *p) {
    Dev d;
    VADX_REQUIRE(dims && w_in && p, "vadx_fsmn_pack_host: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_pack_host: unsupported dims (affine <= 144, linear/output <= 256)");
    memset(p, 0, sizeof(float) * d.total);
    VADX_REQUIRE(w_in->in1_w && w_in->in1_b && w_in->in2_w && w_in->in2_b && w_in->out1_w && w_in->out1_b && w_in->out2_w && w_in->out2_b &&
                 w_in->cmvn_means && w_in->cmvn_vars, "vadx_fsmn_pack_host: NULL weight pointer");
    for (int l = 0; l < NLAYER; ++l)
        VADX_REQUIRE(w_in->lin_w[l] && w_in->fir_w[l] && w_in->aff_w[l] && w_in->aff_b[l], "vadx_fsmn_pack_host: NULL layer %d weight", l);
    // Exact power-of-two rebalancing of the affine chains (csrc/rebalance.h; ordinary checkpoints pass through untouched).  The projection p of
    // every FSMN block is visible outside the kernels (the FIR caches: cache_0..3 of the reference's session), so it stays at its true scale
    // and ends a segment: [in1, in2, lin_0], [aff_l, lin_(l+1)], [aff_3, out1, out2] (softmax after out2).  FIR + skip, ReLU and the
    // activation-free in1 -> in2 / out1 -> out2 pairs are positively homogeneous.
    std::vector<float> r_in1(w_in->in1_w, w_in->in1_w + (size_t)d.A * 400), r_in1b(w_in->in1_b, w_in->in1_b + d.A);
    std::vector<float> r_in2(w_in->in2_w, w_in->in2_w + (size_t)d.L * d.A), r_in2b(w_in->in2_b, w_in->in2_b + d.L);
    std::vector<float> r_out1(w_in->out1_w, w_in->out1_w + (size_t)d.A2 * d.L), r_out1b(w_in->out1_b, w_in->out1_b + d.A2);
    std::vector<float> r_out2(w_in->out2_w, w_in->out2_w + (size_t)d.O * d.A2), r_out2b(w_in->out2_b, w_in->out2_b + d.O);
    std::vector<float> r_lin[NLAYER], r_aff[NLAYER], r_affb[NLAYER];
    for (int l = 0; l < NLAYER; ++l) {
        r_lin[l].assign(w_in->lin_w[l], w_in->lin_w[l] + (size_t)PROJ * d.L);
        r_aff[l].assign(w_in->aff_w[l], w_in->aff_w[l] + (size_t)d.L * PROJ);
        r_affb[l].assign(w_in->aff_b[l], w_in->aff_b[l] + d.L);
    }
    int reb_min = 1000;
    vadx::rebalance_chain({{&r_in1, &r_in1b}, {&r_in2, &r_in2b}, {&r_lin[0], nullptr}}, &reb_min);
    for (int l = 0; l + 1 < NLAYER; ++l) vadx::rebalance_chain({{&r_aff[l], &r_affb[l]}, {&r_lin[l + 1], nullptr}}, &reb_min);
    vadx::rebalance_chain({{&r_aff[NLAYER - 1], &r_affb[NLAYER - 1]}, {&r_out1, &r_out1b}, {&r_out2, &r_out2b}}, &reb_min);
    vadx_fsmn_weights_host w_reb = *w_in;
    w_reb.in1_w = r_in1.data(); w_reb.in1_b = r_in1b.data(); w_reb.in2_w = r_in2.data(); w_reb.in2_b = r_in2b.data();
    w_reb.out1_w = r_out1.data(); w_reb.out1_b = r_out1b.data(); w_reb.out2_w = r_out2.data(); w_reb.out2_b = r_out2b.data();
    for (int l = 0; l < NLAYER; ++l) { w_reb.lin_w[l] = r_lin[l].data(); w_reb.aff_w[l] = r_aff[l].data(); w_reb.aff_b[l] = r_affb[l].data(); }
    const vadx_fsmn_weights_host *w = &w_reb;
    pack::rows_ld(p + d.off_in1, w->in1_w, d.A, 400, 400); memcpy(p + d.off_b1, w->in1_b, d.A * sizeof(float));
    memcpy(p + d.off_mean, w->cmvn_means, 400 * sizeof(float)); memcpy(p + d.off_var, w->cmvn_vars, 400 * sizeof(float));
    pack::rows_ld(p + d.off_in2, w->in2_w, d.L, d.A, d.Ap); memcpy(p + d.off_b2, w->in2_b, d.L * sizeof(float));
    for (int l = 0; l < NLAYER; ++l) {
        VADX_REQUIRE(w->lin_w[l] && w->fir_w[l] && w->aff_w[l] && w->aff_b[l], "vadx_fsmn_pack_host: NULL layer %d weight", l);
        pack::rows_ld(p + d.off_lin[l], w->lin_w[l], PROJ, d.L, d.Lp);
        memcpy(p + d.off_fir[l], w->fir_w[l], PROJ * LORDER * sizeof(float));
        pack::rows_ld(p + d.off_aff[l], w->aff_w[l], d.L, PROJ, PROJ); memcpy(p + d.off_baff[l], w->aff_b[l], d.L * sizeof(float));
    }
    pack::rows_ld(p + d.off_out1, w->out1_w, d.A2, d.L, d.Lp); memcpy(p + d.off_bo1, w->out1_b, d.A2 * sizeof(float));
    pack::rows_ld(p + d.off_out2, w->out2_w, d.O, d.A2, d.A2p); memcpy(p + d.off_bo2, w->out2_b, d.O * sizeof(float));
    // GEMM operands go fragment-major (common.h): one contiguous 1 KB run per wave-wide weight load
    vadx::frag_major_inplace(p + d.off_in1, d.Ap, 400);
    vadx::frag_major_inplace(p + d.off_in2, d.Lp, d.Ap);
    for (int l = 0; l < NLAYER; ++l) {
        vadx::frag_major_inplace(p + d.off_lin[l], PROJ, d.Lp);
        vadx::frag_major_inplace(p + d.off_aff[l], d.Lp, PROJ);
    }
    vadx::frag_major_inplace(p + d.off_out1, d.A2p, d.Lp);
    vadx::frag_major_inplace(p + d.off_out2, d.Op, d.A2p);
    // ---- split-product copies (layers_split.h): A fragments [n-tile][chunk][np planes][QFRAG] from the ORIGINAL row-major weights, in the
    // arithmetic dims->arithmetic names (none for float32 MFMAs)
    float wmax = 0.f;                                                  // largest |weight| handed to fp16 fragments
    // in_linear1 with the CMVN folded in (double): W1' = W1 var, b1' = b1 + sum_k W1' (mean_k - mbar_{k % 80}), mbar = the centre LFR position's means
    for (int m = 0; m < NMEL; ++m) p[d.q_mbar + m] = w->cmvn_means[2 * NMEL + m];
    pack::split(d.np, p + d.q_in1, d.Ap / 16, NCH_IN1, [&](int r, int k) {
        return (r < d.A && k < 400) ? (float)((double)w->in1_w[(size_t)r * 400 + k] * (double)w->cmvn_vars[k]) : 0.f; }, wmax);
    for (int r = 0; r < d.A; ++r) {
        double acc = (double)w->in1_b[r];
        for (int k = 0; k < 400; ++k)
            acc += (double)(float)((double)w->in1_w[(size_t)r * 400 + k] * (double)w->cmvn_vars[k]) * ((double)w->cmvn_means[k] - (double)p[d.q_mbar + k % NMEL]);
        p[d.q_b1 + r] = (float)acc;
    }
    pack::split(d.np, p + d.q_in2, d.Lp / 16, d.nch_A, pack::rowmajor(w->in2_w, d.L, d.A), wmax);
    for (int l = 0; l < NLAYER; ++l) {
        pack::split(d.np, p + d.q_lin[l], PROJ / 16, d.nch_L, pack::rowmajor(w->lin_w[l], PROJ, d.L), wmax);
        pack::split(d.np, p + d.q_aff[l], d.Lp / 16, PROJ / 32, pack::rowmajor(w->aff_w[l], d.L, PROJ), wmax);
    }
    pack::split(d.np, p + d.q_out1, d.A2p / 16, d.nch_L, pack::rowmajor(w->out1_w, d.A2, d.L), wmax);
    pack::split(d.np, p + d.q_out2, d.Op / 16, d.nch_A2, pack::rowmajor(w->out2_w, d.O, d.A2), wmax);
    VADX_REQUIRE(d.arith != vadx::VADX_AR_H2 || wmax <= vadx::H_MAX,
                 "vadx_fsmn_pack_host: a weight (|w| up to %g) is outside the fp16 range: pack with dims->arithmetic = VADX_ARITH_BF16X3", wmax);
    VADX_REQUIRE(d.arith != vadx::VADX_AR_H2 || reb_min >= vadx::REB_REFUSE,
                 "vadx_fsmn_pack_host: a weight tensor lies wholly below 2^%d (largest |w| < 2^%d after rebalancing), outside the fp16 range: pack with "
                 "dims->arithmetic = VADX_ARITH_BF16X3", vadx::REB_REFUSE, reb_min + 1);
    return VADX_OK;
}

// The fp16 x 2 kernels' sticky range flag (as vadx_silero_range_flag): [flag, largest |x|] of the launches since the last reset.
extern "C" int vadx_fsmn_range_flag(const vadx_fsmn_dims *dims, const float *packed, int reset, uint32_t *flag_host, float *amax_host, void *stream) {
    Dev d;
    VADX_REQUIRE(dims && packed && flag_host, "vadx_fsmn_range_flag: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_range_flag: unsupported dims");
    return vadx::range_flag_read(packed + d.off_flag, reset, flag_host, amax_host, stream);
}

// Launch KERNEL<AR> for the arithmetic `arith` (a Dev's) with that tile's dynamic LDS, on `grid` workgroups: the instantiation's dynamic-LDS
// limit is raised right here (every one of these kernels needs more than the 64 KiB default; once per device, VADX_DYN_LDS), so a kernel
// cannot be launched without it.  The kernel's arguments follow the stream.
#define FSMN_LAUNCH_AR(KERNEL, AR, BYTES, grid, stream, ...)                                                                         \
    do {                                                                                                                             \
        VADX_DYN_LDS(KERNEL<AR>, BYTES);                                                                                             \
        hipLaunchKernelGGL(KERNEL<AR>, dim3((unsigned)(grid)), dim3(THREADS), BYTES, static_cast<hipStream_t>(stream), __VA_ARGS__); \
    } while (0)
#define FSMN_LAUNCH(KERNEL, arith, grid, stream, ...)                                                                                \
    do {                                                                                                                             \
        if ((arith) == vadx::VADX_AR_H2) FSMN_LAUNCH_AR(KERNEL, vadx::VADX_AR_H2, SQ_LDS_BYTES, grid, stream, __VA_ARGS__);          \
        else if ((arith) == vadx::VADX_AR_B3) FSMN_LAUNCH_AR(KERNEL, vadx::VADX_AR_B3, SQ_LDS_BYTES, grid, stream, __VA_ARGS__);     \
        else FSMN_LAUNCH_AR(KERNEL, vadx::VADX_AR_F32, LDS_FLOATS * sizeof(float), grid, stream, __VA_ARGS__);                       \
        VADX_HIP_TRY(hipGetLastError());                                                                                             \
    } while (0)

extern "C" int vadx_fsmn_energy(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch,
                                int windows_per_clip, int window_len, int frames, const float *means, float *db,
                                void *stream) {
    VADX_REQUIRE(audio && means && db, "vadx_fsmn_energy: NULL argument");
    VADX_REQUIRE(batch > 0 && windows_per_clip > 0 && window_len >= 512 && frames > 0, "vadx_fsmn_energy: bad shape");
    const float inv_ref = (float)(1.0 / (sqrt((double)window_len) * 2e-5));
    hipLaunchKernelGGL(fsmn_energy_kernel, dim3((unsigned)(batch * windows_per_clip)), dim3(512), 0,
                       static_cast<hipStream_t>(stream), audio, (long long)row_stride, (long long)win_stride,
                       windows_per_clip, window_len, 512, 160, frames, means, inv_ref, db);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_fsmn_window_stats(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                                      int window_len, int frames, float *means, float *db, void *stream) {
    VADX_REQUIRE(audio && means && db, "vadx_fsmn_window_stats: NULL argument");
    VADX_REQUIRE(batch > 0 && windows_per_clip > 0 && window_len >= 512 && frames > 0, "vadx_fsmn_window_stats: bad shape");
    const float inv_ref = (float)(1.0 / (sqrt((double)window_len) * 2e-5));
    const long long nwin = (long long)batch * windows_per_clip;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the one-pass kernel reads 16-byte runs: every window must start on a 16-byte boundary and hold a whole number of 32-sample granules
    const bool aligned = (reinterpret_cast<uintptr_t>(audio) & 15) == 0 && (row_stride & 7) == 0 && (win_stride & 7) == 0 &&
                         window_len % 32 == 0 && window_len <= ST_THREADS * ST_MAXIT * 8;
    if (aligned) {
        hipLaunchKernelGGL(fsmn_stats_kernel, dim3((unsigned)nwin), dim3(ST_THREADS), 0, st, audio, (long long)row_stride, (long long)win_stride,
                           windows_per_clip, window_len, frames, inv_ref, means, db);
        VADX_HIP_TRY(hipGetLastError());
        return VADX_OK;
    }
    int rc = vadx_frontend_window_means(audio, row_stride, win_stride, batch, windows_per_clip, window_len, 1.0f, means, stream);
    if (rc != VADX_OK) return rc;
    return vadx_fsmn_energy(audio, row_stride, win_stride, batch, windows_per_clip, window_len, frames, means, db, stream);
}

extern "C" int vadx_fsmn_run(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                             const float *const cache_in[4], float *const cache_out[4], const float *thr,
                             const float *noise_db, int batch, uint8_t *score, float *noisy_db, float *psil,
                             void *stream) {
    Dev d;
    VADX_REQUIRE(dims && packed && logmel && db && cache_in && cache_out && thr && noise_db && score && noisy_db,
                 "vadx_fsmn_run: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_run: unsupported dims");
    VADX_REQUIRE(d.T <= MAX_T, "vadx_fsmn_run: frames=%d unsupported (at most %d per window: window_len <= %d)", d.T, MAX_T, MAX_T * 160 - 1);
    VADX_REQUIRE(batch > 0, "vadx_fsmn_run: batch must be positive");
    RunArgs r;
    r.logmel = logmel; r.db = db; r.thr = thr; r.noise_db = noise_db; r.score = score; r.noisy_db = noisy_db; r.psil = psil;
    for (int l = 0; l < NLAYER; ++l) {
        VADX_REQUIRE(cache_in[l] && cache_out[l], "vadx_fsmn_run: NULL cache %d", l);
        r.cin[l] = cache_in[l]; r.cout[l] = cache_out[l];
    }
    FSMN_LAUNCH(fsmn_run_kernel, d.arith, batch, stream, d, packed, r);
    return VADX_OK;
}

// The loop constants from the caller's struct, checked against the window first; `who` names the entry point in the message.  advancing: a
// stream's windows must advance, which takes look_backward < frames - 2 (a clip's only look_backward < frames).
static int loop_args(const char *who, const Dev &d, const vadx_fsmn_loop_params *lp, bool advancing, LoopArgs *a) {
    VADX_REQUIRE(lp->look_backward >= 0 && lp->look_backward < (advancing ? d.T - 2 : d.T) && d.T - lp->look_backward <= MAX_T && d.T <= MAX_T_LOOP,
                 "%s: look_backward=%d frames=%d unsupported%s", who, lp->look_backward, d.T,
                 advancing ? " (0 <= look_backward < frames - 2: the windows must advance)" : "");
    // the reference takes slide_range = score_len - look_backward BEFORE it bumps a zero look_backward to 1
    // (Inference_FSMN_VAD_ONNX.py:79-86): LOOK_BACKWARD = 0 means slide_range = T, a vote over one frame, an empty tail
    a->lb = lp->look_backward > 0 ? lp->look_backward : 1;
    a->slide = d.T - lp->look_backward; a->thr = lp->one_minus_speech_threshold; a->noise0 = lp->noise_db_init;
    a->snr = lp->snr_threshold; a->speaking = lp->speaking_score; a->silence_score = lp->silence_score;
    return VADX_OK;
}

extern "C" int vadx_fsmn_clips(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                               int batch, int windows_per_clip, const vadx_fsmn_loop_params *lp, float *cache_ws,
                               uint8_t *flags, float *noise_trace, void *stream) {
    Dev d;
    VADX_REQUIRE(dims && packed && logmel && db && lp && cache_ws && flags, "vadx_fsmn_clips: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_clips: unsupported dims");
    VADX_REQUIRE(batch > 0 && windows_per_clip > 0, "vadx_fsmn_clips: batch/windows must be positive");
    ClipArgs c;
    int rc = loop_args("vadx_fsmn_clips", d, lp, false, &c.lp);
    if (rc) return rc;
    c.logmel = logmel; c.db = db; c.cache = cache_ws; c.W = windows_per_clip;
    c.flags = flags; c.noise_trace = noise_trace;
    FSMN_LAUNCH(fsmn_clips_kernel, d.arith, batch, stream, d, packed, c);
    return VADX_OK;
}

extern "C" int vadx_fsmn_clips_ragged(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int batch,
                                      int n_windows, int max_windows, const int32_t *win_first, const int32_t *order,
                                      const vadx_fsmn_loop_params *lp, float *cache_ws, uint8_t *flags, int64_t flag_stride, float *noise_trace,
                                      void *stream) {
    Dev d;
    VADX_REQUIRE(dims && packed && logmel && db && win_first && lp && cache_ws && flags, "vadx_fsmn_clips_ragged: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_clips_ragged: unsupported dims");
    VADX_REQUIRE(batch >= 1 && n_windows >= 1 && max_windows >= 1, "vadx_fsmn_clips_ragged: batch=%d n_windows=%d max_windows=%d must be positive",
                 batch, n_windows, max_windows);
    RaggedArgs c;
    int rc = loop_args("vadx_fsmn_clips_ragged", d, lp, false, &c.lp);
    if (rc) return rc;
    const long long need = (long long)max_windows * c.lp.slide + lp->look_backward;
    VADX_REQUIRE(flag_stride >= need, "vadx_fsmn_clips_ragged: flag_stride=%lld holds fewer than max_windows * slide + look_backward = %lld flags",
                 (long long)flag_stride, need);
    // every row starts as "no flag"; a clip's workgroup then writes its W_b * slide + look_backward flags over the front of its row
    VADX_HIP_TRY(hipMemsetAsync(flags, 255, (size_t)batch * (size_t)flag_stride, static_cast<hipStream_t>(stream)));
    c.logmel = logmel; c.db = db; c.cache = cache_ws; c.batch = batch; c.n_windows = n_windows; c.max_windows = max_windows;
    c.win_first = win_first; c.order = order;
    c.flags = flags; c.flag_stride = (long long)flag_stride; c.noise_trace = noise_trace;
    FSMN_LAUNCH(fsmn_clips_ragged_kernel, d.arith, batch, stream, d, packed, c);
    return VADX_OK;
}

// ---- long windows (opt-in): every refusal names its argument and comes before any HIP call -----------------------------------------------
#define FSMN_NONNULL(who, p) VADX_REQUIRE((p) != nullptr, who ": NULL " #p)

extern "C" size_t vadx_fsmn_long_workspace_bytes(int rows, int frames) {
    if (rows < 1 || frames < 1 || frames > MAX_T_LONG) return 0;
    return (size_t)rows * 2 * long_row(frames) * sizeof(float);
}

extern "C" int vadx_fsmn_window_stats_long(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                                           int window_len, int frames, float *means, float *db, void *workspace, void *stream) {
    FSMN_NONNULL("vadx_fsmn_window_stats_long", audio); FSMN_NONNULL("vadx_fsmn_window_stats_long", means);
    FSMN_NONNULL("vadx_fsmn_window_stats_long", db); FSMN_NONNULL("vadx_fsmn_window_stats_long", workspace);
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "vadx_fsmn_window_stats_long: workspace must be 8-byte aligned");
    VADX_REQUIRE(batch > 0 && windows_per_clip > 0 && (long long)batch * windows_per_clip < (1ll << 31),
                 "vadx_fsmn_window_stats_long: batch=%d windows_per_clip=%d must be positive", batch, windows_per_clip);
    VADX_REQUIRE(window_len >= 512 && window_len <= (MAX_T_LONG - 1) * 160, "vadx_fsmn_window_stats_long: window_len=%d outside [512, %d]",
                 window_len, (MAX_T_LONG - 1) * 160);
    VADX_REQUIRE(frames >= 1 && frames <= MAX_T_LONG, "vadx_fsmn_window_stats_long: frames=%d outside [1, %d]", frames, MAX_T_LONG);
    VADX_REQUIRE(row_stride >= 0 && win_stride >= 0 && (windows_per_clip - 1) * win_stride + window_len <= row_stride,
                 "vadx_fsmn_window_stats_long: row_stride=%lld holds fewer than (windows_per_clip - 1) * win_stride + window_len = %lld samples",
                 (long long)row_stride, (long long)((windows_per_clip - 1) * win_stride + window_len));
    const float inv_ref = (float)(1.0 / (sqrt((double)window_len) * 2e-5));
    const unsigned nwin = (unsigned)(batch * windows_per_clip);
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long *sums = static_cast<unsigned long long *>(workspace);
    VADX_HIP_TRY(hipMemsetAsync(sums, 0, (size_t)nwin * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(fsmn_long_sum_kernel, dim3(nwin, (unsigned)((window_len + SL_SUM - 1) / SL_SUM)), dim3(SL_THREADS), 0, st, audio,
                       (long long)row_stride, (long long)win_stride, windows_per_clip, window_len, sums);
    VADX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fsmn_long_energy_kernel, dim3(nwin, (unsigned)((frames + SL_FRAMES - 1) / SL_FRAMES)), dim3(SL_THREADS), 0, st, audio,
                       (long long)row_stride, (long long)win_stride, windows_per_clip, window_len, frames, inv_ref, sums, means, db);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_fsmn_run_long(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                                  const float *const cache_in[4], float *const cache_out[4], const float *thr, const float *noise_db,
                                  int batch, uint8_t *score, float *noisy_db, float *psil, void *workspace, void *stream) {
    Dev d;
    FSMN_NONNULL("vadx_fsmn_run_long", dims); FSMN_NONNULL("vadx_fsmn_run_long", packed); FSMN_NONNULL("vadx_fsmn_run_long", logmel);
    FSMN_NONNULL("vadx_fsmn_run_long", db); FSMN_NONNULL("vadx_fsmn_run_long", cache_in); FSMN_NONNULL("vadx_fsmn_run_long", cache_out);
    FSMN_NONNULL("vadx_fsmn_run_long", thr); FSMN_NONNULL("vadx_fsmn_run_long", noise_db); FSMN_NONNULL("vadx_fsmn_run_long", score);
    FSMN_NONNULL("vadx_fsmn_run_long", noisy_db); FSMN_NONNULL("vadx_fsmn_run_long", workspace);
    VADX_REQUIRE(dims->frames >= 1 && dims->frames <= MAX_T_LONG, "vadx_fsmn_run_long: frames=%d outside [1, %d] (window_len <= %d)", dims->frames,
                 MAX_T_LONG, (MAX_T_LONG - 1) * 160);
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_run_long: unsupported dims");
    VADX_REQUIRE(batch > 0, "vadx_fsmn_run_long: batch=%d must be positive", batch);
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "vadx_fsmn_run_long: workspace must be 4-byte aligned");
    RunLongArgs a;
    RunArgs &r = a.r;
    r.logmel = logmel; r.db = db; r.thr = thr; r.noise_db = noise_db; r.score = score; r.noisy_db = noisy_db; r.psil = psil;
    for (int l = 0; l < NLAYER; ++l) {
        VADX_REQUIRE(cache_in[l] && cache_out[l], "vadx_fsmn_run_long: NULL cache_in / cache_out %d", l);
        r.cin[l] = cache_in[l]; r.cout[l] = cache_out[l];
    }
    a.ws.base = static_cast<float *>(workspace); a.ws.row = long_row(d.T);
    FSMN_LAUNCH(fsmn_run_long_kernel, d.arith, batch, stream, d, packed, a);
    return VADX_OK;
}

extern "C" int vadx_fsmn_clips_long(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int batch,
                                    int n_windows, int max_windows, const int32_t *win_first, const int32_t *order,
                                    const vadx_fsmn_loop_params *lp, float *cache_ws, uint8_t *flags, int64_t flag_stride, float *noise_trace,
                                    void *workspace, void *stream) {
    Dev d;
    FSMN_NONNULL("vadx_fsmn_clips_long", dims); FSMN_NONNULL("vadx_fsmn_clips_long", packed); FSMN_NONNULL("vadx_fsmn_clips_long", logmel);
    FSMN_NONNULL("vadx_fsmn_clips_long", db); FSMN_NONNULL("vadx_fsmn_clips_long", lp); FSMN_NONNULL("vadx_fsmn_clips_long", cache_ws);
    FSMN_NONNULL("vadx_fsmn_clips_long", flags); FSMN_NONNULL("vadx_fsmn_clips_long", workspace);
    VADX_REQUIRE(dims->frames >= 1 && dims->frames <= MAX_T_LONG, "vadx_fsmn_clips_long: frames=%d outside [1, %d] (window_len <= %d)", dims->frames,
                 MAX_T_LONG, (MAX_T_LONG - 1) * 160);
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_clips_long: unsupported dims");
    VADX_REQUIRE(batch >= 1 && n_windows >= 1 && max_windows >= 1, "vadx_fsmn_clips_long: batch=%d n_windows=%d max_windows=%d must be positive",
                 batch, n_windows, max_windows);
    // the counts fit each other: a rectangular batch is batch * max_windows windows; a ragged one gives every clip 1 .. max_windows
    VADX_REQUIRE(win_first ? n_windows >= batch && (long long)n_windows <= (long long)batch * max_windows
                           : (long long)n_windows == (long long)batch * max_windows,
                 "vadx_fsmn_clips_long: n_windows=%d does not fit batch=%d clips of %s max_windows=%d", n_windows, batch,
                 win_first ? "1 .." : "exactly", max_windows);
    // the windows of a grid must advance: (look_backward + 1) * 160 < window_len, as the stream path asks
    VADX_REQUIRE(lp->look_backward >= 0 && lp->look_backward < d.T - 1, "vadx_fsmn_clips_long: look_backward=%d outside [0, frames - 1 = %d)",
                 lp->look_backward, d.T - 1);
    ClipLongArgs a;
    RaggedArgs &c = a.r;
    c.lp.lb = lp->look_backward > 0 ? lp->look_backward : 1;       // as loop_args: slide_range is taken before a zero look_backward becomes 1
    c.lp.slide = d.T - lp->look_backward; c.lp.thr = lp->one_minus_speech_threshold; c.lp.noise0 = lp->noise_db_init;
    c.lp.snr = lp->snr_threshold; c.lp.speaking = lp->speaking_score; c.lp.silence_score = lp->silence_score;
    const long long need = (long long)max_windows * c.lp.slide + lp->look_backward;
    VADX_REQUIRE(flag_stride >= need, "vadx_fsmn_clips_long: flag_stride=%lld holds fewer than max_windows * slide + look_backward = %lld flags",
                 (long long)flag_stride, need);
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "vadx_fsmn_clips_long: workspace must be 4-byte aligned");
    // every row starts as "no flag", as in vadx_fsmn_clips_ragged
    VADX_HIP_TRY(hipMemsetAsync(flags, 255, (size_t)batch * (size_t)flag_stride, static_cast<hipStream_t>(stream)));
    c.logmel = logmel; c.db = db; c.cache = cache_ws; c.batch = batch; c.n_windows = n_windows; c.max_windows = max_windows;
    c.win_first = win_first; c.order = order;
    c.flags = flags; c.flag_stride = (long long)flag_stride; c.noise_trace = noise_trace;
    a.ws.base = static_cast<float *>(workspace); a.ws.row = long_row(d.T);
    FSMN_LAUNCH(fsmn_clips_long_kernel, d.arith, batch, stream, d, packed, a);
    return VADX_OK;
}

extern "C" size_t vadx_fsmn_stream_state_bytes(int streams, int look_backward) {
    return streams > 0 && look_backward >= 0 ? rec_bytes(streams, (look_backward + 1) * 160) : 0;
}

extern "C" int vadx_fsmn_stream_windows(const int16_t *samples, int64_t row_stride, int streams, int windows, int window_len,
                                        int look_backward, const uint8_t *reset, const uint8_t *active, const void *state_in,
                                        void *state_out, int16_t *window_buf, void *stream) {
    VADX_REQUIRE(samples && state_in && state_out && window_buf, "vadx_fsmn_stream_windows: NULL argument");
    VADX_REQUIRE(streams > 0 && windows >= 1 && (long long)streams * ((long long)windows + 1) < (1ll << 31),
                 "vadx_fsmn_stream_windows: streams=%d windows=%d", streams, windows);
    VADX_REQUIRE(window_len >= 512 && window_len % 8 == 0, "vadx_fsmn_stream_windows: window_len=%d must be a multiple of 8, at least 512", window_len);
    const int T = window_len / 160 + 1, C = (look_backward + 1) * 160, stride = window_len - C;
    VADX_REQUIRE(look_backward >= 0 && look_backward < T && stride > 0,
                 "vadx_fsmn_stream_windows: look_backward=%d outside [0, %d) or no stride left (window_len - (look_backward + 1) * 160 = %d)",
                 look_backward, T, stride);
    VADX_REQUIRE(row_stride >= (int64_t)windows * stride && row_stride % 8 == 0,
                 "vadx_fsmn_stream_windows: row_stride=%lld must be a multiple of 8 and hold windows * stride = %lld samples",
                 (long long)row_stride, (long long)windows * stride);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, rec_bytes(streams, C)), "vadx_fsmn_stream_windows: state_in and state_out overlap");
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out) |
                   reinterpret_cast<uintptr_t>(window_buf)) & 15) == 0,
                 "vadx_fsmn_stream_windows: samples, records and window_buf must be 16-byte aligned");
    WinArgs a;
    a.samples = samples; a.row_stride = (long long)row_stride; a.k = windows; a.L = window_len; a.C = C; a.reset = reset; a.active = active;
    a.sin = static_cast<const unsigned char *>(state_in); a.sout = static_cast<unsigned char *>(state_out);
    a.hdr = rec_hdr(streams); a.carry = rec_carry(streams); a.wbuf = window_buf;
    hipLaunchKernelGGL(fsmn_stream_windows_kernel, dim3((unsigned)(streams * (windows + 1))), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_fsmn_stream_run(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int streams,
                                    int windows, const vadx_fsmn_loop_params *lp, const uint8_t *reset, const uint8_t *active,
                                    const void *state_in, void *state_out, uint8_t *flags, uint8_t *tail, float *noise_trace, void *stream) {
    Dev d;
    VADX_REQUIRE(dims && packed && logmel && db && lp && state_in && state_out && flags, "vadx_fsmn_stream_run: NULL argument");
    VADX_REQUIRE(derive(dims, &d) == 0, "vadx_fsmn_stream_run: unsupported dims");
    VADX_REQUIRE(streams > 0 && windows >= 1, "vadx_fsmn_stream_run: streams=%d windows=%d", streams, windows);
    LoopArgs a;
    int rc = loop_args("vadx_fsmn_stream_run", d, lp, true, &a);
    if (rc) return rc;
    VADX_REQUIRE(tail || lp->look_backward == 0, "vadx_fsmn_stream_run: NULL tail with look_backward=%d", lp->look_backward);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, rec_bytes(streams, (lp->look_backward + 1) * 160)),
                 "vadx_fsmn_stream_run: state_in and state_out overlap");
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0,
                 "vadx_fsmn_stream_run: records must be 16-byte aligned");
    // the stream kernel keeps its flat argument struct: with a LoopArgs inside it the kernel compiles to other code, and the tick is 0.8 % slower
    StreamArgs c;
    c.logmel = logmel; c.db = db; c.sin = static_cast<const unsigned char *>(state_in); c.sout = static_cast<unsigned char *>(state_out);
    c.hdr = rec_hdr(streams); c.reset = reset; c.active = active; c.k = windows; c.ntail = lp->look_backward;
    c.lb = a.lb; c.slide = a.slide; c.thr = a.thr; c.noise0 = a.noise0; c.snr = a.snr; c.speaking = a.speaking; c.silence_score = a.silence_score;
    c.flags = flags; c.tail = tail; c.noise_trace = noise_trace;
    FSMN_LAUNCH(fsmn_stream_kernel, d.arith, streams, stream, d, packed, c);
    return VADX_OK;
}

// ---- ragged ticks: every refusal names its argument and comes before any HIP call ---------------------------------------------------------
extern "C" int vadx_fsmn_stream_ragged_max_windows(void) { return STREAM_RAGGED_MAX_WINDOWS; }

// what both ragged calls check alike: the sizes, the tables and the two records
static int ragged_tick_args(const char *who, int streams, int n_windows, int max_windows, int look_backward, const int32_t *counts,
                            const int32_t *win_first, const void *state_in, void *state_out, const uint32_t *status) {
    VADX_REQUIRE(counts != nullptr, "%s: NULL counts", who);
    VADX_REQUIRE(win_first != nullptr, "%s: NULL win_first", who);
    VADX_REQUIRE(state_in != nullptr, "%s: NULL state_in", who);
    VADX_REQUIRE(state_out != nullptr, "%s: NULL state_out", who);
    VADX_REQUIRE(status != nullptr, "%s: NULL status", who);
    VADX_REQUIRE(streams >= 1, "%s: streams=%d must be at least 1", who, streams);
    VADX_REQUIRE(n_windows >= 1, "%s: n_windows=%d must be at least 1 (a tick without audio is not launched)", who, n_windows);
    VADX_REQUIRE(max_windows >= 1 && max_windows <= STREAM_RAGGED_MAX_WINDOWS,
                 "%s: max_windows=%d outside [1, %d] (vadx_fsmn_stream_ragged_max_windows; longer catch-ups go through vadx_fsmn_stream_run)",
                 who, max_windows, STREAM_RAGGED_MAX_WINDOWS);
    VADX_REQUIRE((long long)streams + (long long)n_windows < (1ll << 31), "%s: streams=%d + n_windows=%d workgroups", who, streams, n_windows);
    VADX_REQUIRE(look_backward >= 0, "%s: look_backward=%d is negative", who, look_backward);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0,
                 "%s: state_in and state_out must be 16-byte aligned", who);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, rec_bytes(streams, (look_backward + 1) * 160)), "%s: state_in and state_out overlap", who);
    return VADX_OK;
}

extern "C" int vadx_fsmn_stream_windows_ragged(const int16_t *samples, int64_t row_stride, int streams, int n_windows, int max_windows,
                                               int window_len, int look_backward, const int32_t *counts, const int32_t *win_first,
                                               const int32_t *win_stream, const uint8_t *reset, const void *state_in, void *state_out,
                                               int16_t *window_buf, uint32_t *status, void *stream) {
    const char *who = "vadx_fsmn_stream_windows_ragged";
    VADX_REQUIRE(samples != nullptr, "%s: NULL samples", who);
    VADX_REQUIRE(win_stream != nullptr, "%s: NULL win_stream", who);
    VADX_REQUIRE(window_buf != nullptr, "%s: NULL window_buf", who);
    VADX_REQUIRE(window_len >= 512 && window_len % 8 == 0, "%s: window_len=%d must be a multiple of 8, at least 512", who, window_len);
    const int T = window_len / 160 + 1, C = (look_backward + 1) * 160, stride = window_len - C;
    VADX_REQUIRE(look_backward >= 0 && look_backward < T && stride > 0,
                 "%s: look_backward=%d outside [0, %d) or no stride left (window_len - (look_backward + 1) * 160 = %d)", who, look_backward, T, stride);
    int rc = ragged_tick_args(who, streams, n_windows, max_windows, look_backward, counts, win_first, state_in, state_out, status);
    if (rc) return rc;
    VADX_REQUIRE(row_stride >= (int64_t)max_windows * stride && row_stride % 8 == 0,
                 "%s: row_stride=%lld must be a multiple of 8 and hold max_windows * stride = %lld samples", who, (long long)row_stride,
                 (long long)max_windows * stride);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(samples) | reinterpret_cast<uintptr_t>(window_buf)) & 15) == 0,
                 "%s: samples and window_buf must be 16-byte aligned", who);
    WinRaggedArgs a;
    a.samples = samples; a.row_stride = (long long)row_stride; a.S = streams; a.n_windows = n_windows; a.max_windows = max_windows;
    a.L = window_len; a.C = C; a.counts = counts; a.win_first = win_first; a.win_stream = win_stream; a.reset = reset;
    a.sin = static_cast<const unsigned char *>(state_in); a.sout = static_cast<unsigned char *>(state_out);
    a.hdr = rec_hdr(streams); a.carry = rec_carry(streams); a.wbuf = window_buf; a.status = status;
    hipLaunchKernelGGL(fsmn_stream_windows_ragged_kernel, dim3((unsigned)(n_windows + streams)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_fsmn_stream_run_ragged(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int streams,
                                           int n_windows, int max_windows, const vadx_fsmn_loop_params *lp, const int32_t *counts,
                                           const int32_t *win_first, const int32_t *order, const uint8_t *reset, const void *state_in,
                                           void *state_out, uint8_t *flags, uint8_t *tail, float *noise_trace, uint32_t *status, void *stream) {
    const char *who = "vadx_fsmn_stream_run_ragged";
    Dev d;
    VADX_REQUIRE(dims != nullptr, "%s: NULL dims", who);
    VADX_REQUIRE(packed != nullptr, "%s: NULL packed", who);
    VADX_REQUIRE(logmel != nullptr, "%s: NULL logmel", who);
    VADX_REQUIRE(db != nullptr, "%s: NULL db", who);
    VADX_REQUIRE(lp != nullptr, "%s: NULL lp", who);
    VADX_REQUIRE(flags != nullptr, "%s: NULL flags", who);
    VADX_REQUIRE(derive(dims, &d) == 0, "%s: unsupported dims", who);
    LoopArgs a;
    int rc = loop_args(who, d, lp, true, &a);
    if (rc) return rc;
    rc = ragged_tick_args(who, streams, n_windows, max_windows, lp->look_backward, counts, win_first, state_in, state_out, status);
    if (rc) return rc;
    VADX_REQUIRE(tail || lp->look_backward == 0, "%s: NULL tail with look_backward=%d", who, lp->look_backward);
    StreamRaggedArgs c;
    c.logmel = logmel; c.db = db; c.sin = static_cast<const unsigned char *>(state_in); c.sout = static_cast<unsigned char *>(state_out);
    c.hdr = rec_hdr(streams); c.reset = reset; c.counts = counts; c.win_first = win_first; c.order = order;
    c.S = streams; c.n_windows = n_windows; c.max_windows = max_windows; c.ntail = lp->look_backward;
    c.lb = a.lb; c.slide = a.slide; c.thr = a.thr; c.noise0 = a.noise0; c.snr = a.snr; c.speaking = a.speaking; c.silence_score = a.silence_score;
    c.flags = flags; c.tail = tail; c.noise_trace = noise_trace; c.status = status;
    FSMN_LAUNCH(fsmn_stream_ragged_kernel, d.arith, streams, stream, d, packed, c);
    return VADX_OK;
}
