// firered.hip -- FireRedVAD / FireRedAED DetectModel (channel-first DFSMN) for gfx950, plus the
// VadPostprocessor decision kernel shared with MarbleNet.
// Reference: FireRedVAD/Export_FireRedVAD.py:185-326 (FSMN / DFSMNBlock / DFSMN / DetectModel),
// :420-467 (wrapper), FireRedVAD/Inference_FireRed_ONNX.py:102-304 (VadPostprocessor).
//
// One workgroup owns one stateless analysis window (T <= 112 frames, 98 for 16000 samples).
// Activations stay in LDS k-major [channel][frame] for the whole stack:
//   mem [P][T] (block input / FSMN output, updated in place), p [P][T] (FSMN input), h [H][32] tile.
// Pointwise convs = f32-MFMA GEMMs over 32-frame tiles (weights streamed from L2); the dilated
// depthwise look-back / look-ahead FIRs + skip run on the VALU over the whole window once per block.
#include "rebalance.h"
#include "common.h"
#include "layers.h"
#include "pack.h"

#include <math.h>
#include <string.h>

namespace vadx {
namespace firered {

constexpr int THREADS = 512;
constexpr int NMEL = 80, MAX_R = 16, MAX_M = 4, MAX_ODIM = 4, MAX_T = 112;
constexpr int M_LD = 116;               // mem / p row stride (112 + 4)
constexpr int H_LD = 36;                // h tile row stride (32 + 4)
constexpr int MAXP = 128, MAXH = 256;
constexpr int MEM_F = MAXP * M_LD, P_F = MAXP * M_LD, H_F = MAXH * H_LD;
constexpr int LDS_FLOATS = MEM_F + P_F + H_F;

struct Dev {
    int R, M, H, P, N1, S1, N2, S2, odim, T, Hp, Pp;
    int off_fc1, off_fc1b, off_fc2, off_fc2b;
    int off_lb[MAX_R], off_la[MAX_R], off_win[MAX_R], off_bfc1[MAX_R], off_bfc1b[MAX_R], off_bfc2[MAX_R];
    int off_dnn[MAX_M], off_dnnb[MAX_M], off_out, off_outb, total;
    // split-product copies of the point-wise pairs (Hp = 256, Pp = 128 only): A fragments [n-tile][32-k chunk][np planes][QFRAG] of the ONE
    // arithmetic cfg->arithmetic names (split_scheme.h: np = 3 bf16 x 3, 2 fp16 x 2, 0 none = float32 MFMAs)
    int split_ok, arith, np, off_flag, q_fc1, q_fc2, q_bfc1[MAX_R], q_bfc2[MAX_R];
    // M = 1: the dnn layer (P -> H, ReLU) and the output head (H -> odim, rows padded to Pp with zeros) as one more point-wise pair
    int q_dnn0, q_head, off_headb;
};

static int r16(int x) { return (x + 15) & ~15; }

static int derive(const vadx_firered_cfg *c, Dev *d) {
    memset(d, 0, sizeof(*d));
    if (c->idim != NMEL || c->R < 1 || c->R > MAX_R || c->M < 1 || c->M > MAX_M || c->H < 1 || c->P < 1 ||
        c->N1 < 1 || c->N1 > 32 || c->S1 < 1 || c->N2 < 0 || c->N2 > 32 || (c->N2 > 0 && c->S2 < 1) ||
        c->odim < 1 || c->odim > MAX_ODIM || c->frames < 1 || c->frames > MAX_T)
        return -1;
    d->R = c->R; d->M = c->M; d->H = c->H; d->P = c->P; d->N1 = c->N1; d->S1 = c->S1; d->N2 = c->N2; d->S2 = c->S2;
    d->odim = c->odim; d->T = c->frames; d->Hp = r16(c->H); d->Pp = r16(c->P);
    if (d->Hp > MAXH || d->Pp > MAXP) return -1;
    int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 255) & ~255; return r; };      // every section on a 1 KiB boundary (a wave's fragment load = 1 KiB = 16 lines)
    d->off_fc1 = take(d->Hp * NMEL); d->off_fc1b = take(d->Hp);
    d->off_fc2 = take(d->Pp * d->Hp); d->off_fc2b = take(d->Pp);
    for (int r = 0; r < d->R; ++r) {
        d->off_lb[r] = take(d->Pp * d->N1);
        d->off_la[r] = take(d->Pp * (d->N2 > 0 ? d->N2 : 1));
        d->off_win[r] = take(d->Pp * 40);          // merged 40-tap window c[-19..20] per channel (fast FIR path)
        if (r > 0) { d->off_bfc1[r] = take(d->Hp * d->Pp); d->off_bfc1b[r] = take(d->Hp); d->off_bfc2[r] = take(d->Pp * d->Hp); }
    }
    for (int m = 0; m < d->M; ++m) { d->off_dnn[m] = take(d->Hp * (m == 0 ? d->Pp : d->Hp)); d->off_dnnb[m] = take(d->Hp); }
    d->off_out = take(16 * d->Hp); d->off_outb = take(16);      // output head padded to one 16-row MFMA tile
    d->split_ok = d->Hp == 256 && d->Pp == 128;
    // AUTO = bf16 x 3 where the split kernel applies (float32's exponent range: safe without the range protocol), float32 MFMAs otherwise;
    // fp16 x 2 is an explicit request (VADX_ARITH_F16X2) by callers that read vadx_firered_range_flag, as FireRedEngine does; an explicit
    // split arithmetic elsewhere is refused
    d->arith = vadx::arith_internal(c->arithmetic, d->split_ok ? vadx::VADX_AR_B3 : vadx::VADX_AR_F32);
    if (d->arith < 0 || (d->arith != vadx::VADX_AR_F32 && !d->split_ok)) return -1;
    d->np = vadx::planes_of(d->arith);
    if (d->np) {
        const int np = d->np;
        d->q_fc1 = take(16 * 3 * np * vadx::QFRAG);                // 80 mels -> 3 chunks of 32 (k-groups 10, 11 are zero rows)
        d->q_fc2 = take(8 * 8 * np * vadx::QFRAG);
        for (int r = 1; r < d->R; ++r) { d->q_bfc1[r] = take(16 * 4 * np * vadx::QFRAG); d->q_bfc2[r] = take(8 * 8 * np * vadx::QFRAG); }
        if (d->M == 1) { d->q_dnn0 = take(16 * 4 * np * vadx::QFRAG); d->q_head = take(8 * 8 * np * vadx::QFRAG); d->off_headb = take(d->Pp); }
    }
    d->off_flag = take(4);
    d->total = o;
    return 0;
}

// memory = p + lookback(p) + lookahead(p) (+ mem)   -- Export_FireRedVAD.py:213-236, :255-264
// thread = (channel, quarter of the window); the channel's taps sit in registers (loops fully unrolled
// to MAXTAP with guards: a runtime-indexed tap array would live in scratch and serialise on latency).
constexpr int MAXTAP = 32;

// Fast path for undilated filters with <= 20 taps each (the shipped FireRedVAD/AED configs): the
// look-back and look-ahead filters merge into one 40-tap window c[-19..20] around t; each thread slides
// it over 28 frames held in registers -- no guards, no address math in the inner loop.

__device__ __forceinline__ void fsmn_memory_fast(const Dev &d, const float *__restrict__ Pk, int r, bool skip,
                                                 const float *p, float *mem) {
    // thread = (channel PAIR, eighth of the window): both channels ride in the two halves of v_pk_fma_f32 operands
    // (twice the f32 FMA rate of the scalar form; the per-channel summation order is unchanged).
    constexpr int LB = 19, LA = 20, SEG = 14, WIN = SEG + LB + LA;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));       // per call: the clamped indices / in-range predicates below are invariant over the blocks, and hoisted out
                                        // of the block loop they stayed live through the point-wise pairs and spilled (15 registers, the kernel's scratch)
    const int cp = tid >> 3, part = tid & 7, ch = 2 * cp;
    if (ch >= d.Pp) return;
    f32x2 c[LB + 1 + LA];                       // c[j + LB], j = -19..20 ; c[LB] (j = 0) unused (zero)
    {   const f32x4 *w0 = reinterpret_cast<const f32x4 *>(Pk + d.off_win[r] + ch * 40), *w1 = w0 + 10;      // merged at pack time
#pragma unroll
        for (int g = 0; g < 10; ++g) {
            const f32x4 a4 = w0[g], b4 = w1[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) c[4 * g + e] = f32x2{a4[e], b4[e]};
        }
    }
    const float *row0 = p + ch * M_LD, *row1 = row0 + M_LD;
    const int t0 = part * SEG;
    f32x2 win[WIN];
#pragma unroll
    for (int u = 0; u < WIN; ++u) {
        const int t = t0 - LB + u;
        const bool in = t >= 0 && t < d.T;
        const int tc = t < 0 ? 0 : (t > MAX_T - 1 ? MAX_T - 1 : t);      // unconditional loads (clamped) + select:
        const float v0 = row0[tc], v1 = row1[tc];                          // a guarded load costs a branch and a wait each
        win[u] = f32x2{in ? v0 : 0.f, in ? v1 : 0.f};
    }
#pragma unroll
    for (int u = 0; u < SEG; ++u) {
        const int t = t0 + u;
        f32x2 lb = {0.f, 0.f}, la = {0.f, 0.f};
#pragma unroll
        for (int j = -LB; j <= 0; ++j) lb = __builtin_elementwise_fma(c[j + LB], win[u + LB + j], lb);      // same order as the generic path
#pragma unroll
        for (int j = 1; j <= LA; ++j) la = __builtin_elementwise_fma(c[j + LB], win[u + LB + j], la);
        // frames t >= T (< MAX_T) are inside the row: computing / storing them unconditionally is harmless (the next
        // layer's columns are independent and p is zero there) and keeps the loop branch-free
        f32x2 s2 = (win[u + LB] + lb) + la;
        if (skip) s2 += f32x2{mem[ch * M_LD + t], mem[(ch + 1) * M_LD + t]};
        mem[ch * M_LD + t] = s2[0];
        mem[(ch + 1) * M_LD + t] = s2[1];
    }
}

__device__ __forceinline__ void fsmn_memory_generic(const Dev &d, const float *__restrict__ Pk, int r, bool skip,
                                            const float *p, float *mem) {
    const int ch = threadIdx.x >> 2, part = threadIdx.x & 3;
    if (ch >= d.Pp) return;
    float wlb[MAXTAP], wla[MAXTAP];
#pragma unroll
    for (int k = 0; k < MAXTAP; ++k) {
        wlb[k] = k < d.N1 ? Pk[d.off_lb[r] + ch * d.N1 + k] : 0.f;
        wla[k] = k < d.N2 ? Pk[d.off_la[r] + ch * d.N2 + k] : 0.f;
    }
    const float *row = p + ch * M_LD;
    const int per = (d.T + 3) >> 2, t0 = part * per, t1 = (t0 + per < d.T) ? t0 + per : d.T;
    const bool ahead = d.N2 > 0 && d.T > 1;
    for (int t = t0; t < t1; ++t) {
        float lb = 0.f, la = 0.f;
#pragma unroll
        for (int k = 0; k < MAXTAP; ++k) {
            const int idx = t + (k - (d.N1 - 1)) * d.S1;
            if (k < d.N1 && idx >= 0) lb = fmaf(wlb[k], row[idx], lb);
        }
        float s = row[t] + lb;
        if (ahead) {
#pragma unroll
            for (int k = 0; k < MAXTAP; ++k) {
                const int idx = t + d.S2 + k * d.S2;
                if (k < d.N2 && idx < d.T) la = fmaf(wla[k], row[idx], la);
            }
            s += la;
        }
        if (skip) s += mem[ch * M_LD + t];
        mem[ch * M_LD + t] = s;
    }
}

__device__ __forceinline__ void fsmn_memory(const Dev &d, const float *__restrict__ Pk, int r, bool skip, const float *p, float *mem) {
    if (d.S1 == 1 && d.N1 <= 20 && (d.N2 == 0 || d.S2 == 1) && d.N2 <= 20 && d.T > 1 && d.T <= 112 && d.Pp <= 128) fsmn_memory_fast(d, Pk, r, skip, p, mem);
    else fsmn_memory_generic(d, Pk, r, skip, p, mem);
}

// pointwise pair on every 32-frame tile of the window: h = relu(W1 x src + b1); dst = W2 x h (+b2, relu)
// The DFSMN block's P -> H -> P pair at the published widths (H = 256: one pair of n-tiles per wave; P = 128: one
// n-tile per wave; 8 waves).  A wave's slice of BOTH matrices -- 8 blocks x 2 tiles of W1, 16 blocks x 1 tile of W2,
// 128 VGPRs -- is loaded once per block and stays in registers while the window's tiles stream through: no weight
// traffic inside the pair (it was re-streamed from L2 for every 32-frame tile, and every phase opened with an L2 round
// trip that nobody else on the CU could cover: one workgroup per CU, all waves at the same barrier).  Bias / ReLU /
// LDS store as in layer<>.  MT = 2 for a full 32-frame tile, 1 for a last tile of <= 16 frames.
template <int KB1>
struct PairResident {
    f32x4 w1[KB1][2], w2[16][1];
    float bias1[2], bias2;
};

// HAS2: the second (H -> P) layer exists; otherwise the H tile in `h` is the result (dnn layer before the output head)
template <int MT, int KB1, bool HAS2>
__device__ __forceinline__ void pair_tile_resident(const PairResident<KB1> &R, const float *src, float *dst, float *h, int f0, bool relu2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, i = lane & 15;
    int moff[MT], hoff[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { moff[mt] = f0 + 16 * mt; hoff[mt] = 16 * mt; }
    {   f32x4 acc[2][MT];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm_resident<2, MT, KB1>(acc, src, M_LD, moff, lane, R.w1);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[nt][mt][r] + R.bias1[nt], 0.f);
                *reinterpret_cast<f32x4 *>(h + ((wave + 8 * nt) * 16 + i) * H_LD + mt * 16 + 4 * q) = v;
            }
    }
    __syncthreads();
    if (HAS2) {
        f32x4 acc[1][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[0][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm_resident<1, MT, 16>(acc, h, H_LD, hoff, lane, R.w2);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = acc[0][mt][r] + R.bias2; if (relu2) v[r] = fmaxf(v[r], 0.f); }
            *reinterpret_cast<f32x4 *>(dst + (wave * 16 + i) * M_LD + f0 + mt * 16 + 4 * q) = v;
        }
        __syncthreads();
    }
}

template <int KB1, bool HAS2>
__device__ __forceinline__ void load_pair_resident(PairResident<KB1> &R, const float *W1, const float *b1, const float *W2, const float *b2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15;
    const float *row10 = frag_ptr(W1, KB1 * 16, wave, 0, lane), *row11 = frag_ptr(W1, KB1 * 16, wave + 8, 0, lane);
#pragma unroll
    for (int S = 0; S < KB1; ++S) { R.w1[S][0] = ldg4(row10 + FRAG * S); R.w1[S][1] = ldg4(row11 + FRAG * S); }
    if (HAS2) {
        const float *row2 = frag_ptr(W2, 256, wave, 0, lane);
#pragma unroll
        for (int S = 0; S < 16; ++S) R.w2[S][0] = ldg4(row2 + FRAG * S);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) R.bias1[nt] = ldg1(b1 + (wave + 8 * nt) * 16 + i);
    R.bias2 = (HAS2 && b2) ? ldg1(b2 + wave * 16 + i) : 0.f;
}

// (DV: a Dev, or the ragged tick's TickDims -- the point-wise pairs read T, Hp and Pp of it)
template <int KB1, typename DV>
__device__ __forceinline__ void pointwise_pair_resident(const DV &d, const float *W1, const float *b1, const float *src,
                                                        const float *W2, const float *b2, bool relu2, float *dst, float *h) {
    PairResident<KB1> R;
    load_pair_resident<KB1, true>(R, W1, b1, W2, b2);
    for (int f0 = 0; f0 < d.T; f0 += 32) {
        if (d.T - f0 <= 16) pair_tile_resident<1, KB1, true>(R, src, dst, h, f0, relu2);
        else pair_tile_resident<2, KB1, true>(R, src, dst, h, f0, relu2);
    }
}


// ---- the point-wise pair on bf16 x 3 split products (csrc/split3.h), published widths (H = 256, P = 128, 8 waves) ----------------------
// Same data flow as pointwise_pair_resident -- src and dst stay float32 [channel][frame] (the FIR memory works on them), a wave's slice of
// BOTH matrices is resident for the whole window (192 VGPRs of bf16 fragments) -- but the tile is 16 frames and each GEMM runs as six
// v_mfma_f32_16x16x32_bf16 per K = 32 step: 96 bf16 MFMAs per wave and tile instead of 256 f32 ones (6/16 of the matrix time).
// Per tile: the tile's src columns are split into three bf16 planes [k / 8][16 frames][8] (512 items, one per thread) | barrier | GEMM 1,
// weights = A operand: a lane ends with four consecutive H channels of one frame -> bias, ReLU, split, one 8-byte store per plane of the
// H tile | barrier | GEMM 2, activations = A operand: a lane ends with four consecutive frames of one P channel -> one float4 store into
// dst.  The planes live where the f32 kernel keeps its 32-frame H tile (12 KB + 24 KB = its 36 KB).
constexpr int QS_PL_SRC = 16 * 16 * 16, QS_PL_H = 32 * 16 * 16;     // bytes of one plane: src tile (<= 128 ch x 16 frames), H tile (256 x 16)
template <typename SC, int KC1>
struct PairSplit { typename SC::frag w1[2][KC1][SC::NP], w2[8][SC::NP]; f32x4 bias1[2]; float bias2; };

template <typename SC, int KC1>
__device__ __forceinline__ void load_pair_split(PairSplit<SC, KC1> &R, const float *Q1, const float *b1, const float *Q2, const float *b2, int tid) {
    constexpr int NP = SC::NP;
    const int lane = tid & 63, wave = tid >> 6, q = lane >> 4, i = lane & 15;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int kc = 0; kc < KC1; ++kc)
#pragma unroll
            for (int p = 0; p < NP; ++p) R.w1[nt][kc][p] = SC::ld(Q1 + (size_t)(((wave + 8 * nt) * KC1 + kc) * NP + p) * QFRAG, lane);
#pragma unroll
    for (int kc = 0; kc < 8; ++kc)
#pragma unroll
        for (int p = 0; p < NP; ++p) R.w2[kc][p] = SC::ld(Q2 + (size_t)((wave * 8 + kc) * NP + p) * QFRAG, lane);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) R.bias1[nt] = ldg4(b1 + (wave + 8 * nt) * 16 + 4 * q);
    R.bias2 = b2 ? ldg1(b2 + wave * 16 + i) : 0.f;
}

template <typename SC, int KC1, typename DV>
__device__ __forceinline__ void pointwise_pair_split(const DV &d, const float *Q1, const float *b1, int ksrc, const float *src,
                                                     const float *Q2, const float *b2, bool relu2, float *dst, float *hbuf, float &amax) {
    constexpr int NP = SC::NP;
    typedef typename SC::frag frag;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));       // per call: the per-lane LDS offsets below are loop-invariant over the blocks, and hoisted out of the block
                                        // loop they stayed live through the FIR (186 registers of its own) and spilled there (layers.h has the same note)
    const int lane = tid & 63, wave = tid >> 6, q = lane >> 4, i = lane & 15;
    unsigned char *SQ = reinterpret_cast<unsigned char *>(hbuf), *HQ = SQ + 3 * QS_PL_SRC;       // (the plane map is sized for three planes; fp16 x 2 uses two of each)
    PairSplit<SC, KC1> R;
    load_pair_split<SC, KC1>(R, Q1, b1, Q2, b2, tid);
    if (ksrc < KC1 * 32) {             // k-groups beyond the source's channels (80 mels in 96 slots): rows of zeros, written once
        const int kg0 = ksrc / 8, n = (KC1 * 4 - kg0) * 16;
        for (int e = tid; e < NP * n; e += THREADS) {
            const int p = e / n, r = e - p * n;
            *reinterpret_cast<f32x4 *>(SQ + p * QS_PL_SRC + (kg0 * 16 + r) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const int cg = tid >> 4, fr = tid & 15;
    auto split_tile = [&](int f0) {    // this thread's item: channels 4 cg .. 4 cg + 3 of frame f0 + fr -> the three planes of the src tile
        if (4 * cg < ksrc) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = src[(4 * cg + c) * M_LD + f0 + fr];
            u32x2 pp[NP];
            SC::split4(v, pp, amax);
            unsigned char *dp = SQ + ((cg >> 1) * 16 + fr) * 16 + (cg & 1) * 8;
#pragma unroll
            for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x2 *>(dp + p * QS_PL_SRC) = pp[p];
        }
    };
    split_tile(0);
    __syncthreads();
    for (int f0 = 0; f0 < d.T; f0 += 16) {
        {   // GEMM 1: H channels 16 (wave + 8 nt) + 4 q + r of frame i
            f32x4 hi[2][1], lo[2][1];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) { hi[nt][0] = R.bias1[nt]; lo[nt][0] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int kc = 0; kc < KC1; ++kc) {
                frag b[1][NP], a[2][NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    b[0][p] = SC::lds(SQ + p * QS_PL_SRC + ((4 * kc + q) * 16 + i) * 16);
                    a[0][p] = R.w1[0][kc][p];
                    a[1][p] = R.w1[1][kc][p];
                }
                SC::template products<2, 1, true>(a, b, hi, lo);
            }
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                f32x4 v = SC::join(hi[nt][0], lo[nt][0]);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                u32x2 pp[NP];
                SC::split4(v, pp, amax);
                const int g = 4 * (wave + 8 * nt) + q;
                unsigned char *dp = HQ + ((g >> 1) * 16 + i) * 16 + (g & 1) * 8;
#pragma unroll
                for (int p = 0; p < NP; ++p) *reinterpret_cast<u32x2 *>(dp + p * QS_PL_H) = pp[p];
            }
        }
        __syncthreads();
        // the NEXT tile's split rides beside GEMM 2: GEMM 1 is done with the src planes (barrier above), GEMM 2 reads only the H tile, and
        // the barrier at the end of the iteration publishes both the new src planes and the free H tile
        if (f0 + 16 < d.T) split_tile(f0 + 16);
        {   // GEMM 2 (activations = A operand): frames f0 + 4 q + r of P channel 16 wave + i
            f32x4 hi[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}}, lo[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
#pragma unroll
            for (int kc = 0; kc < 8; ++kc) {
                frag b[1][NP], a[1][NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    b[0][p] = SC::lds(HQ + p * QS_PL_H + ((4 * kc + q) * 16 + i) * 16);
                    a[0][p] = R.w2[kc][p];
                }
                SC::template products<1, 1, false>(a, b, hi, lo);
            }
            f32x4 v = SC::join(hi[0][0], lo[0][0]);
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = v[r] + R.bias2; if (relu2) v[r] = fmaxf(v[r], 0.f); }
            *reinterpret_cast<f32x4 *>(dst + (wave * 16 + i) * M_LD + f0 + 4 * q) = v;
        }
        __syncthreads();
    }
}

template <typename DV>
__device__ __forceinline__ void pointwise_pair(const DV &d, const float *W1, const float *b1, int k1b, const float *src,
                                               const float *W2, const float *b2, int relu2, float *dst, float *h) {
    if (W2 && d.Hp == 256 && d.Pp == 128 && blockDim.x == 512) {
        if (k1b == 8) { pointwise_pair_resident<8>(d, W1, b1, src, W2, b2, relu2 != 0, dst, h); return; }      // DFSMN block
        if (k1b == 5) { pointwise_pair_resident<5>(d, W1, b1, src, W2, b2, relu2 != 0, dst, h); return; }      // fc1 (80 mels) / fc2
    }
    for (int f0 = 0; f0 < d.T; f0 += 32) {
        const bool half = (d.T - f0) <= 16;
        LayerArgs a{W1, k1b * 16, d.Hp / 16, 1, k1b, 0, 0, b1, 1, src, M_LD, f0, h, H_LD, 0, nullptr, nullptr};
        if (half) layer<1, false>(a); else layer<2, false>(a);
        __syncthreads();
        if (W2) {
            LayerArgs c{W2, d.Hp, d.Pp / 16, 1, d.Hp / 16, 0, 0, b2, relu2, h, H_LD, 0, dst, M_LD, f0, nullptr, nullptr};
            if (half) layer<1, false>(c); else layer<2, false>(c);
            __syncthreads();
        }
    }
}

template <int AR>
__global__ __launch_bounds__(THREADS, 2) void firered_kernel(Dev d, const float *__restrict__ Pk,
                                                             const float *__restrict__ logmel, float *__restrict__ probs) {
    constexpr bool SPLIT = AR != vadx::VADX_AR_F32;
    typedef typename vadx::SchemeFor<AR>::type SC;
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *mem = lds, *p = lds + MEM_F, *h = p + P_F;
    const int tid = threadIdx.x;
    const float *lm = logmel + (size_t)blockIdx.x * d.T * NMEL;
    // stage log-mel channel-first into `mem` rows 0..79; frames >= T are zero (finite operands)
    for (int e = tid; e < MAX_T * NMEL; e += THREADS) {
        const int t = e / NMEL, mel = e - t * NMEL;
        const float v = lm[(size_t)(t < d.T ? t : d.T - 1) * NMEL + mel];      // unconditional (clamped) load, then select
        mem[mel * M_LD + t] = t < d.T ? v : 0.f;
    }
    for (int e = tid; e < MAXP * M_LD; e += THREADS) p[e] = 0.f;
    __syncthreads();
    // dfsmn.fc1 (80->H, ReLU) ; dfsmn.fc2 (H->P, bias, ReLU) ; fsmn1
    if (SPLIT) pointwise_pair_split<SC, 3>(d, Pk + d.q_fc1, Pk + d.off_fc1b, NMEL, mem, Pk + d.q_fc2, Pk + d.off_fc2b, true, p, h, amax);
    else pointwise_pair(d, Pk + d.off_fc1, Pk + d.off_fc1b, NMEL / 16, mem, Pk + d.off_fc2, Pk + d.off_fc2b, 1, p, h);
    for (int e = tid; e < MAXP * M_LD; e += THREADS) mem[e] = 0.f;        // log-mel rows are dead now
    __syncthreads();
    fsmn_memory(d, Pk, 0, false, p, mem);
    __syncthreads();
    for (int r = 1; r < d.R; ++r) {      // DFSMNBlock: fc1 (P->H, ReLU) ; fc2 (H->P, no bias) ; fsmn + skip
        if (SPLIT) pointwise_pair_split<SC, 4>(d, Pk + d.q_bfc1[r], Pk + d.off_bfc1b[r], d.Pp, mem, Pk + d.q_bfc2[r], nullptr, false, p, h, amax);
        else pointwise_pair(d, Pk + d.off_bfc1[r], Pk + d.off_bfc1b[r], d.Pp / 16, mem, Pk + d.off_bfc2[r], nullptr, 0, p, h);
        fsmn_memory(d, Pk, r, true, p, mem);
        __syncthreads();
    }
    // One dnn layer (the published configuration): dnn (P -> H, ReLU) + output head (H -> odim) are one more point-wise pair on split
    // products -- the head's rows padded to Pp with zeros (as many MFMAs as a block's second layer, at a third of the f32 MFMAs' cost) --
    // over the whole window at once instead of tile by tile on float32 MFMAs; logits land in p[o][t].
    if (SPLIT && d.M == 1) {
        pointwise_pair_split<SC, 4>(d, Pk + d.q_dnn0, Pk + d.off_dnnb[0], d.Pp, mem, Pk + d.q_head, Pk + d.off_headb, false, p, h, amax);
        __syncthreads();
        for (int e = tid; e < d.odim * d.T; e += THREADS) {
            const int o = e / d.T, t = e - o * d.T;
            probs[((size_t)blockIdx.x * d.odim + o) * d.T + t] = sigmoidf_(p[o * M_LD + t]);
        }
        if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
        return;
    }
    // dnns (P->H ReLU, then M-1 x H->H ReLU) and the 1x1 output conv + sigmoid, tile by tile
    float *h2 = p;                        // p is dead: second H-tile buffer for M > 1
    const bool dnn_resident = d.Hp == 256 && d.Pp == 128 && blockDim.x == 512;
    PairResident<8> RD;                   // dnn[0] (P -> H) stays in registers across the window's tiles, like the pairs
    if (dnn_resident) load_pair_resident<8, false>(RD, Pk + d.off_dnn[0], Pk + d.off_dnnb[0], nullptr, nullptr);
    for (int f0 = 0; f0 < d.T; f0 += 32) {
        const bool half = (d.T - f0) <= 16;
        if (dnn_resident) {
            if (half) pair_tile_resident<1, 8, false>(RD, mem, nullptr, h, f0, false);
            else pair_tile_resident<2, 8, false>(RD, mem, nullptr, h, f0, false);
        } else {
            LayerArgs a{Pk + d.off_dnn[0], d.Pp, d.Hp / 16, 1, d.Pp / 16, 0, 0, Pk + d.off_dnnb[0], 1, mem, M_LD, f0, h, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(a); else layer<2, false>(a);
            __syncthreads();
        }
        float *cur = h, *nxt = h2;
        for (int m = 1; m < d.M; ++m) {
            LayerArgs c{Pk + d.off_dnn[m], d.Hp, d.Hp / 16, 1, d.Hp / 16, 0, 0, Pk + d.off_dnnb[m], 1, cur, H_LD, 0, nxt, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(c); else layer<2, false>(c);
            __syncthreads();
            float *tmp = cur; cur = nxt; nxt = tmp;
        }
        // output head (odim <= 4 rows, zero padded to one MFMA tile) -> logits in `lg`, then sigmoid
        float *lg = p + MAXH * H_LD;            // behind h2
        {   LayerArgs o{Pk + d.off_out, d.Hp, 1, 1, d.Hp / 16, 0, 0, Pk + d.off_outb, 0, cur, H_LD, 0, lg, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(o); else layer<2, false>(o); }
        __syncthreads();
        if (tid < 32 * d.odim) {
            const int t = tid & 31, o = tid >> 5;
            if (f0 + t < d.T) probs[((size_t)blockIdx.x * d.odim + o) * d.T + f0 + t] = sigmoidf_(lg[o * H_LD + t]);
        }
        __syncthreads();
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

// ---- streaming variant (FireRedVAD/Export_FireRedVAD.py:479-612): no look-ahead, the look-back context
// of every FSMN comes from an explicit cache [R][B][P][(N1-1)*S1] that is returned updated ---------------
__device__ __forceinline__ void fsmn_memory_stream(const Dev &d, const float *__restrict__ Pk, int r, bool skip,
                                                   const float *p, float *mem, const float *__restrict__ cin,
                                                   float *__restrict__ cout) {
    const int pad = (d.N1 - 1) * d.S1;
    for (int e = threadIdx.x; e < d.P * d.T; e += THREADS) {
        const int ch = e / d.T, t = e - ch * d.T;
        const float *row = p + ch * M_LD, *crow = cin + (size_t)ch * pad, *w = Pk + d.off_lb[r] + ch * d.N1;
        float lb = 0.f;
        for (int k = 0; k < d.N1; ++k) {
            const int j = t + k * d.S1;                       // index into cache ++ p
            lb = fmaf(w[k], j < pad ? crow[j] : row[j - pad], lb);
        }
        float s2 = row[t] + lb;
        if (skip) s2 += mem[ch * M_LD + t];
        mem[ch * M_LD + t] = s2;
    }
    for (int e = threadIdx.x; e < d.P * pad; e += THREADS) {      // new cache = last `pad` entries of cache ++ p
        const int ch = e / pad, j = e - ch * pad, src = d.T + j;
        cout[e] = src < pad ? cin[(size_t)ch * pad + src] : p[ch * M_LD + src - pad];
    }
}

__global__ __launch_bounds__(THREADS, 2) void firered_stream_kernel(Dev d, const float *__restrict__ Pk,
                                                                    const float *__restrict__ logmel,
                                                                    const float *__restrict__ caches_in,
                                                                    float *__restrict__ caches_out, int B,
                                                                    float *__restrict__ probs) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *mem = lds, *p = lds + MEM_F, *h = p + P_F;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int pad = (d.N1 - 1) * d.S1;
    const float *lm = logmel + (size_t)b * d.T * NMEL;
    for (int e = tid; e < MAX_T * NMEL; e += THREADS) {
        const int t = e / NMEL, mel = e - t * NMEL;
        const float v = lm[(size_t)(t < d.T ? t : d.T - 1) * NMEL + mel];      // unconditional (clamped) load, then select
        mem[mel * M_LD + t] = t < d.T ? v : 0.f;
    }
    for (int e = tid; e < MAXP * M_LD; e += THREADS) p[e] = 0.f;
    __syncthreads();
    pointwise_pair(d, Pk + d.off_fc1, Pk + d.off_fc1b, NMEL / 16, mem, Pk + d.off_fc2, Pk + d.off_fc2b, 1, p, h);
    for (int e = tid; e < MAXP * M_LD; e += THREADS) mem[e] = 0.f;
    __syncthreads();
    auto cache = [&](const float *base, int r) { return base + ((size_t)r * B + b) * d.P * pad; };
    fsmn_memory_stream(d, Pk, 0, false, p, mem, cache(caches_in, 0), const_cast<float *>(cache(caches_out, 0)));
    __syncthreads();
    for (int r = 1; r < d.R; ++r) {
        pointwise_pair(d, Pk + d.off_bfc1[r], Pk + d.off_bfc1b[r], d.Pp / 16, mem, Pk + d.off_bfc2[r], nullptr, 0, p, h);
        fsmn_memory_stream(d, Pk, r, true, p, mem, cache(caches_in, r), const_cast<float *>(cache(caches_out, r)));
        __syncthreads();
    }
    float *h2 = p;
    for (int f0 = 0; f0 < d.T; f0 += 32) {
        const bool half = (d.T - f0) <= 16;
        LayerArgs a{Pk + d.off_dnn[0], d.Pp, d.Hp / 16, 1, d.Pp / 16, 0, 0, Pk + d.off_dnnb[0], 1, mem, M_LD, f0, h, H_LD, 0, nullptr, nullptr};
        if (half) layer<1, false>(a); else layer<2, false>(a);
        __syncthreads();
        float *cur = h, *nxt = h2;
        for (int m = 1; m < d.M; ++m) {
            LayerArgs c{Pk + d.off_dnn[m], d.Hp, d.Hp / 16, 1, d.Hp / 16, 0, 0, Pk + d.off_dnnb[m], 1, cur, H_LD, 0, nxt, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(c); else layer<2, false>(c);
            __syncthreads();
            float *tmp = cur; cur = nxt; nxt = tmp;
        }
        float *lg = p + MAXH * H_LD;            // behind h2
        {   LayerArgs o{Pk + d.off_out, d.Hp, 1, 1, d.Hp / 16, 0, 0, Pk + d.off_outb, 0, cur, H_LD, 0, lg, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(o); else layer<2, false>(o); }
        __syncthreads();
        if (tid < 32 * d.odim) {
            const int t = tid & 31, o = tid >> 5;
            if (f0 + t < d.T) probs[((size_t)b * d.odim + o) * d.T + f0 + t] = sigmoidf_(lg[o * H_LD + t]);
        }
        __syncthreads();
    }
}

// ---- VadPostprocessor: one clip per thread, working arrays laid out [frame][clip] (coalesced) -------
struct PostDev {
    int ws, min_sp, max_sp, min_si, merge, extend;
    float thr, inv_ws;
};

__global__ void vadpost_kernel(PostDev q, const float *__restrict__ probs, int stride, const int *__restrict__ nframes,
                               int B, float *__restrict__ wsm, signed char *__restrict__ wdec,
                               signed char *__restrict__ decisions, int *__restrict__ segs, int *__restrict__ counts, int cap) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int n = nframes[b];
    const float *pr = probs + (size_t)b * stride;
#define SM(i) wsm[(size_t)(i) * B + b]
#define DEC(i) wdec[(size_t)(i) * B + b]
    counts[b] = 0;
    if (n <= 0) return;
    // smoothing: float32 running sum exactly like np.cumsum, expanding mean on the first ws-1 frames
    if (q.ws > 1) {
        float cs = 0.f;
        for (int i = 0; i < n; ++i) { cs = __fadd_rn(cs, pr[i]); SM(i) = cs; }      // SM(i) = cumsum[i+1]
        for (int i = n - 1; i >= 0; --i) {
            float v;
            if (i < q.ws - 1) v = __fdiv_rn(SM(i), (float)(i + 1));
            else v = __fmul_rn(__fsub_rn(SM(i), (i - q.ws >= 0) ? SM(i - q.ws) : 0.f), q.inv_ws);
            SM(i) = v;                    // descending order: SM(i - ws) is still a cumsum when read
        }
    } else {
        for (int i = 0; i < n; ++i) SM(i) = pr[i];
    }
    // threshold + 4-state machine
    if (q.min_sp <= 0 && q.min_si <= 0) {
        for (int t = 0; t < n; ++t) DEC(t) = SM(t) >= q.thr ? 1 : 0;
    } else {
        int state = 0, t0 = 0, s0 = 0;
        for (int t = 0; t < n; ++t) {
            const bool hot = SM(t) >= q.thr;
            if (state == 0) { if (hot) { state = 1; t0 = t; } }
            else if (state == 1) {
                if (hot) { if (t - t0 >= q.min_sp) { state = 2; for (int u = t0; u < t; ++u) DEC(u) = 1; } }
                else state = 0;
            } else if (state == 2) { if (!hot) { state = 3; s0 = t; } }
            else { if (!hot) { if (t - s0 >= q.min_si) state = 0; } else state = 2; }
            DEC(t) = state >= 2 ? 1 : 0;
        }
    }
    // extend each rising edge left by the smoothing window
    if (q.ws > 1)
        for (int t = 1; t < n; ++t)
            if (DEC(t) == 1 && DEC(t - 1) == 0) { for (int u = (t >= q.ws ? t - q.ws : 0); u < t; ++u) DEC(u) = 1; }
    if (q.merge > 0) {
        int g0 = -1;
        for (int t = 1; t < n; ++t) {
            const int a = DEC(t - 1), c = DEC(t);
            if (a == 1 && c == 0 && g0 < 0) g0 = t;
            else if (a == 0 && c == 1 && g0 >= 0) { if (t - g0 < q.merge) for (int u = g0; u < t; ++u) DEC(u) = 1; g0 = -1; }
        }
    }
    if (q.extend > 0) {
        int dist = q.extend + 1;
        for (int t = 0; t < n; ++t) { if (DEC(t)) dist = 0; else if (++dist <= q.extend) DEC(t) = 1; }
        dist = q.extend + 1;
        for (int t = n - 1; t >= 0; --t) { if (DEC(t)) dist = 0; else if (++dist <= q.extend) DEC(t) = 1; }
    }
    // split segments longer than max_speech at the lowest raw probability of [pos+max/2, pos+max)
    {
        const int half = q.max_sp >> 1;
        int t = 0;
        while (t < n) {
            if (!DEC(t)) { ++t; continue; }
            const int a = t;
            while (t < n && DEC(t)) ++t;
            if (t - a > q.max_sp) {
                int pos = a;
                const int e = t;
                while (pos + q.max_sp < e) {
                    const int lo = pos + half, hi = (pos + q.max_sp < e) ? pos + q.max_sp : e;
                    if (lo >= hi) break;
                    int arg = lo;
                    float best = pr[lo];
                    for (int u = lo + 1; u < hi; ++u) if (pr[u] < best) { best = pr[u]; arg = u; }
                    DEC(arg) = 0;
                    pos = arg + 1;
                }
            }
        }
    }
    // decisions out + (start_frame, end_frame) pairs (end = first frame after the run)
    int ns = 0, start = -1;
    for (int t = 0; t < n; ++t) {
        const int v = DEC(t);
        decisions[(size_t)b * stride + t] = (signed char)v;
        if (v && start < 0) start = t;
        if (!v && start >= 0) { if (ns < cap) { segs[((size_t)b * cap + ns) * 2] = start; segs[((size_t)b * cap + ns) * 2 + 1] = t; } ++ns; start = -1; }
    }
    if (start >= 0) { if (ns < cap) { segs[((size_t)b * cap + ns) * 2] = start; segs[((size_t)b * cap + ns) * 2 + 1] = n; } ++ns; }
    counts[b] = ns;
#undef SM
#undef DEC
}

}  // namespace firered
}  // namespace vadx

using namespace vadx::firered;
namespace pack = vadx::pack;

extern "C" size_t vadx_firered_packed_floats(const vadx_firered_cfg *cfg) {
    Dev d;
    if (!cfg || derive(cfg, &d)) return 0;
    return (size_t)d.total;
}

extern "C" int vadx_firered_pack_host(const vadx_firered_cfg *cfg, const vadx_firered_weights_host *w_in, float *p) {
    Dev d;
    VADX_REQUIRE(cfg && w_in && p, "vadx_firered_pack_host: NULL argument");
    VADX_REQUIRE(derive(cfg, &d) == 0, "vadx_firered_pack_host: unsupported config (idim 80, H<=256, P<=128, frames<=112, odim<=4)");
    memset(p, 0, sizeof(float) * d.total);
    VADX_REQUIRE(w_in->fc1_w && w_in->fc1_b && w_in->fc2_w && w_in->fc2_b && w_in->out_w && w_in->out_b, "vadx_firered_pack_host: NULL weight pointer");
    for (int r = 1; r < d.R; ++r)
        VADX_REQUIRE(w_in->blk_fc1_w[r] && w_in->blk_fc1_b[r] && w_in->blk_fc2_w[r], "vadx_firered_pack_host: NULL block %d weight", r);
    for (int m = 0; m < d.M; ++m) VADX_REQUIRE(w_in->dnn_w[m] && w_in->dnn_b[m], "vadx_firered_pack_host: NULL dnn %d weight", m);
    // Exact power-of-two rebalancing of the point-wise pairs (csrc/rebalance.h; ordinary checkpoints pass through untouched).  The P-wide trunk
    // carries the skip connections and the streaming caches (caches_in / caches_out of the reference's stream session), so it stays at its true
    // scale and ends every segment: [fc1, fc2], [blk_fc1_r, blk_fc2_r], [dnn_0 .. dnn_(M-1), out] (sigmoid after out).
    std::vector<float> r_fc1(w_in->fc1_w, w_in->fc1_w + (size_t)d.H * NMEL), r_fc1b(w_in->fc1_b, w_in->fc1_b + d.H);
    std::vector<float> r_fc2(w_in->fc2_w, w_in->fc2_w + (size_t)d.P * d.H), r_fc2b(w_in->fc2_b, w_in->fc2_b + d.P);
    std::vector<float> r_out(w_in->out_w, w_in->out_w + (size_t)d.odim * d.H), r_outb(w_in->out_b, w_in->out_b + d.odim);
    std::vector<float> r_b1[16], r_b1b[16], r_b2[16], r_dnn[4], r_dnnb[4];
    int reb_min = 1000;
    vadx::rebalance_chain({{&r_fc1, &r_fc1b}, {&r_fc2, &r_fc2b}}, &reb_min);
    vadx_firered_weights_host w_reb = *w_in;
    w_reb.fc1_w = r_fc1.data(); w_reb.fc1_b = r_fc1b.data(); w_reb.fc2_w = r_fc2.data(); w_reb.fc2_b = r_fc2b.data();
    for (int r = 1; r < d.R; ++r) {
        r_b1[r].assign(w_in->blk_fc1_w[r], w_in->blk_fc1_w[r] + (size_t)d.H * d.P);
        r_b1b[r].assign(w_in->blk_fc1_b[r], w_in->blk_fc1_b[r] + d.H);
        r_b2[r].assign(w_in->blk_fc2_w[r], w_in->blk_fc2_w[r] + (size_t)d.P * d.H);
        vadx::rebalance_chain({{&r_b1[r], &r_b1b[r]}, {&r_b2[r], nullptr}}, &reb_min);
        w_reb.blk_fc1_w[r] = r_b1[r].data(); w_reb.blk_fc1_b[r] = r_b1b[r].data(); w_reb.blk_fc2_w[r] = r_b2[r].data();
    }
    {
        std::vector<vadx::RebLayer> tail;
        for (int m = 0; m < d.M; ++m) {
            r_dnn[m].assign(w_in->dnn_w[m], w_in->dnn_w[m] + (size_t)d.H * (m == 0 ? d.P : d.H));
            r_dnnb[m].assign(w_in->dnn_b[m], w_in->dnn_b[m] + d.H);
            tail.push_back({&r_dnn[m], &r_dnnb[m]});
            w_reb.dnn_w[m] = r_dnn[m].data(); w_reb.dnn_b[m] = r_dnnb[m].data();
        }
        tail.push_back({&r_out, &r_outb});
        vadx::rebalance_chain(tail, &reb_min);
        w_reb.out_w = r_out.data(); w_reb.out_b = r_outb.data();
    }
    const vadx_firered_weights_host *w = &w_reb;
    pack::rows_ld(p + d.off_fc1, w->fc1_w, d.H, NMEL, NMEL); memcpy(p + d.off_fc1b, w->fc1_b, d.H * sizeof(float));
    pack::rows_ld(p + d.off_fc2, w->fc2_w, d.P, d.H, d.Hp); memcpy(p + d.off_fc2b, w->fc2_b, d.P * sizeof(float));
    for (int r = 0; r < d.R; ++r) {
        VADX_REQUIRE(w->fsmn_lb[r] && (d.N2 == 0 || w->fsmn_la[r]), "vadx_firered_pack_host: NULL FSMN filter %d", r);
        memcpy(p + d.off_lb[r], w->fsmn_lb[r], (size_t)d.P * d.N1 * sizeof(float));
        if (d.N2 > 0) memcpy(p + d.off_la[r], w->fsmn_la[r], (size_t)d.P * d.N2 * sizeof(float));
        if (d.N1 <= 20 && d.N2 <= 20)          // look-back taps end at j = 0 (slot 19), look-ahead taps start at j = 1 (slot 20)
            for (int ch = 0; ch < d.P; ++ch) {
                for (int k = 0; k < d.N1; ++k) p[d.off_win[r] + ch * 40 + 19 - (d.N1 - 1) + k] = w->fsmn_lb[r][(size_t)ch * d.N1 + k];
                for (int k = 0; k < d.N2; ++k) p[d.off_win[r] + ch * 40 + 20 + k] = w->fsmn_la[r][(size_t)ch * d.N2 + k];
            }
        if (r > 0) {
            VADX_REQUIRE(w->blk_fc1_w[r] && w->blk_fc1_b[r] && w->blk_fc2_w[r], "vadx_firered_pack_host: NULL block %d weight", r);
            pack::rows_ld(p + d.off_bfc1[r], w->blk_fc1_w[r], d.H, d.P, d.Pp); memcpy(p + d.off_bfc1b[r], w->blk_fc1_b[r], d.H * sizeof(float));
            pack::rows_ld(p + d.off_bfc2[r], w->blk_fc2_w[r], d.P, d.H, d.Hp);
        }
    }
    for (int m = 0; m < d.M; ++m) {
        VADX_REQUIRE(w->dnn_w[m] && w->dnn_b[m], "vadx_firered_pack_host: NULL dnn %d weight", m);
        pack::rows_ld(p + d.off_dnn[m], w->dnn_w[m], d.H, m == 0 ? d.P : d.H, m == 0 ? d.Pp : d.Hp);
        memcpy(p + d.off_dnnb[m], w->dnn_b[m], d.H * sizeof(float));
    }
    pack::rows_ld(p + d.off_out, w->out_w, d.odim, d.H, d.Hp); memcpy(p + d.off_outb, w->out_b, d.odim * sizeof(float));
    // GEMM operands go fragment-major (common.h); the FIR taps stay row-major (VALU)
    vadx::frag_major_inplace(p + d.off_out, 16, d.Hp);
    vadx::frag_major_inplace(p + d.off_fc1, d.Hp, NMEL);
    vadx::frag_major_inplace(p + d.off_fc2, d.Pp, d.Hp);
    for (int r = 1; r < d.R; ++r) {
        vadx::frag_major_inplace(p + d.off_bfc1[r], d.Hp, d.Pp);
        vadx::frag_major_inplace(p + d.off_bfc2[r], d.Pp, d.Hp);
    }
    for (int m = 0; m < d.M; ++m) vadx::frag_major_inplace(p + d.off_dnn[m], d.Hp, m == 0 ? d.Pp : d.Hp);
    if (d.np) {              // split A fragments [n-tile][chunk][np planes][QFRAG] from the ORIGINAL row-major weights, in cfg->arithmetic
        float wmax = 0.f;
        pack::split(d.np, p + d.q_fc1, d.Hp / 16, 3, pack::rowmajor(w->fc1_w, d.H, NMEL), wmax);
        pack::split(d.np, p + d.q_fc2, d.Pp / 16, 8, pack::rowmajor(w->fc2_w, d.P, d.H), wmax);
        for (int r = 1; r < d.R; ++r) {
            pack::split(d.np, p + d.q_bfc1[r], d.Hp / 16, 4, pack::rowmajor(w->blk_fc1_w[r], d.H, d.P), wmax);
            pack::split(d.np, p + d.q_bfc2[r], d.Pp / 16, 8, pack::rowmajor(w->blk_fc2_w[r], d.P, d.H), wmax);
        }
        if (d.M == 1) {
            pack::split(d.np, p + d.q_dnn0, d.Hp / 16, 4, pack::rowmajor(w->dnn_w[0], d.H, d.P), wmax);
            pack::split(d.np, p + d.q_head, d.Pp / 16, 8, pack::rowmajor(w->out_w, d.odim, d.H), wmax);
            memcpy(p + d.off_headb, w->out_b, d.odim * sizeof(float));
        }
        VADX_REQUIRE(d.arith != vadx::VADX_AR_H2 || wmax <= vadx::H_MAX,
                     "vadx_firered_pack_host: a weight (|w| up to %g) is outside the fp16 range: pack with cfg->arithmetic = VADX_ARITH_BF16X3", wmax);
        VADX_REQUIRE(d.arith != vadx::VADX_AR_H2 || reb_min >= vadx::REB_REFUSE,
                     "vadx_firered_pack_host: a weight tensor lies wholly below 2^%d (largest |w| < 2^%d after rebalancing), outside the fp16 range: pack "
                     "with cfg->arithmetic = VADX_ARITH_BF16X3", vadx::REB_REFUSE, reb_min + 1);
    }
    return VADX_OK;
}

// The fp16 x 2 kernel's sticky range flag (as vadx_silero_range_flag)
extern "C" int vadx_firered_range_flag(const vadx_firered_cfg *cfg, const float *packed, int reset, uint32_t *flag_host, float *amax_host, void *stream) {
    Dev d;
    VADX_REQUIRE(cfg && packed && flag_host, "vadx_firered_range_flag: NULL argument");
    VADX_REQUIRE(derive(cfg, &d) == 0, "vadx_firered_range_flag: unsupported config");
    return vadx::range_flag_read(packed + d.off_flag, reset, flag_host, amax_host, stream);
}

extern "C" int vadx_firered_run(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int windows,
                                float *probs, void *stream) {
    Dev d;
    VADX_REQUIRE(cfg && packed && logmel && probs, "vadx_firered_run: NULL argument");
    VADX_REQUIRE(derive(cfg, &d) == 0, "vadx_firered_run: unsupported config");
    VADX_REQUIRE(windows > 0, "vadx_firered_run: windows must be positive");
    VADX_DYN_LDS(firered_kernel<0>, LDS_FLOATS * sizeof(float));
    VADX_DYN_LDS(firered_kernel<1>, LDS_FLOATS * sizeof(float));
    VADX_DYN_LDS(firered_kernel<2>, LDS_FLOATS * sizeof(float));
    if (d.arith == vadx::VADX_AR_H2)
        hipLaunchKernelGGL(firered_kernel<2>, dim3(windows), dim3(THREADS), LDS_FLOATS * sizeof(float), static_cast<hipStream_t>(stream), d, packed, logmel, probs);
    else if (d.arith == vadx::VADX_AR_B3)
        hipLaunchKernelGGL(firered_kernel<1>, dim3(windows), dim3(THREADS), LDS_FLOATS * sizeof(float), static_cast<hipStream_t>(stream), d, packed, logmel, probs);
    else
        hipLaunchKernelGGL(firered_kernel<0>, dim3(windows), dim3(THREADS), LDS_FLOATS * sizeof(float),
                           static_cast<hipStream_t>(stream), d, packed, logmel, probs);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" size_t vadx_vadpost_workspace_bytes(int batch, int stride) {
    if (batch <= 0 || stride <= 0) return 0;
    return (size_t)batch * stride * (sizeof(float) + 1) + 64;
}

extern "C" int vadx_vadpost(const vadx_vadpost_params *prm, const float *probs, int stride, const int32_t *n_frames,
                            int batch, int8_t *decisions, int32_t *segments, int32_t *counts, int cap,
                            void *workspace, size_t workspace_bytes, void *stream) {
    VADX_REQUIRE(prm && probs && n_frames && decisions && segments && counts && workspace, "vadx_vadpost: NULL argument");
    VADX_REQUIRE(batch > 0 && stride > 0 && cap > 0, "vadx_vadpost: batch/stride/cap must be positive");
    if (workspace_bytes < vadx_vadpost_workspace_bytes(batch, stride)) {
        vadx::set_error("vadx_vadpost: workspace %zu B < required %zu B", workspace_bytes, vadx_vadpost_workspace_bytes(batch, stride));
        return VADX_ENOSPACE;
    }
    PostDev q;
    q.ws = prm->smooth_window_size < 1 ? 1 : prm->smooth_window_size;
    q.thr = prm->prob_threshold; q.min_sp = prm->min_speech_frame; q.max_sp = prm->max_speech_frame;
    q.min_si = prm->min_silence_frame; q.merge = prm->merge_silence_frame; q.extend = prm->extend_speech_frame;
    q.inv_ws = (float)(1.0 / (double)q.ws);
    float *wsm = static_cast<float *>(workspace);
    signed char *wdec = reinterpret_cast<signed char *>(wsm + (size_t)batch * stride);
    hipLaunchKernelGGL(vadpost_kernel, dim3((batch + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), q, probs,
                       stride, n_frames, batch, wsm, wdec, reinterpret_cast<signed char *>(decisions), segments, counts, cap);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}



// ---- StreamVadPostprocessor on device (FireRedVAD/Export_FireRedVAD.py:1161-1339): one thread per stream, the state carried between
// chunks in a 32-word record per stream.  Same float32 operations in the same order as the reference's per-frame loop (ring-buffer moving
// average: sum += p - buf[k]; sum / count; compare with the float32 threshold), same four-state machine, forced split at max_speech.
namespace vadx {
namespace firered {
struct StreamPostDev { int ws; float thr; int pad_start, min_sp, max_sp, min_si; };
constexpr int SP_WORDS = 32, SP_MAXWS = 16;      // record: [0,16) window buffer, 16 sum, 17 pos, 18 count, 19 frame_cnt, 20 state, 21 speech_cnt,
                                                 // 22 silence_cnt, 23 hit_max, 24 last_start, 25 last_end
__global__ void stream_vadpost_kernel(StreamPostDev q, const float *__restrict__ probs, long long stride, int frames, int streams,
                                      float *__restrict__ state, int reset, int flush, int *__restrict__ segs, int *__restrict__ counts, int cap) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= streams) return;
    float *rec = state + (size_t)s * SP_WORDS;
    int *ri = reinterpret_cast<int *>(rec);
    float buf[SP_MAXWS];
    float sum = 0.f;
    int pos = 0, cnt = 0, fc = 0, st = 0, sp = 0, si = 0, hit = 0, last_start = -1, last_end = -1;
    if (!reset) {
#pragma unroll
        for (int k = 0; k < SP_MAXWS; ++k) buf[k] = rec[k];
        sum = rec[16]; pos = ri[17]; cnt = ri[18]; fc = ri[19]; st = ri[20]; sp = ri[21]; si = ri[22]; hit = ri[23]; last_start = ri[24]; last_end = ri[25];
    } else {
#pragma unroll
        for (int k = 0; k < SP_MAXWS; ++k) buf[k] = 0.f;
    }
    int *out = segs + (size_t)s * cap * 2, n = 0;
    auto emit = [&](int a, int b) { if (n < cap) { out[2 * n] = a; out[2 * n + 1] = b; } ++n; };
    const float *pr = probs + (size_t)s * stride;
    for (int t = 0; t < frames; ++t) {
        const float p = pr[t];
        ++fc;
        float sm = p;
        if (q.ws > 1) {
            float old = 0.f;
#pragma unroll
            for (int k = 0; k < SP_MAXWS; ++k) if (k == pos) { old = buf[k]; buf[k] = p; }      // (register array: no dynamic indexing)
            sum = __fadd_rn(sum, __fsub_rn(p, old));
            pos = pos + 1 == q.ws ? 0 : pos + 1;
            if (cnt < q.ws) ++cnt;
            sm = __fdiv_rn(sum, (float)cnt);
        }
        const bool speech = sm >= q.thr;
        int e0 = 0, e1 = 0;
        bool ended = false;
        if (hit) { last_start = fc; hit = 0; }           // a forced split re-opens a segment on the next frame
        auto close = [&]() { e0 = last_start; e1 = fc; ended = true; last_start = -1; last_end = fc; };
        if (st == 0) {
            if (speech) { st = 1; sp = 1; } else { ++si; sp = 0; }
        } else if (st == 1) {
            if (speech) {
                ++sp;
                if (sp >= q.min_sp) {
                    st = 2;
                    int a = fc - sp + 1 - q.pad_start;
                    a = a < 1 ? 1 : a;
                    last_start = a > last_end + 1 ? a : last_end + 1;
                    si = 0;
                }
            } else { st = 0; si = 1; sp = 0; }
        } else {
            ++sp;
            if (speech) {
                st = 2; si = 0;
                if (sp >= q.max_sp) { hit = 1; sp = 0; close(); }
            } else if (st == 2) { st = 3; si = 1; }
            else {
                ++si;
                if (si >= q.min_si) { st = 0; sp = 0; close(); }
            }
        }
        if (ended && e0 > 0) emit(e0 - 1 > 0 ? e0 - 1 : 0, e1 - 1 > 0 ? e1 - 1 : 0);
    }
    if (flush && last_start > 0) emit(last_start - 1 > 0 ? last_start - 1 : 0, fc - 1);      // unterminated segment at the end of the stream
    counts[s] = n;
#pragma unroll
    for (int k = 0; k < SP_MAXWS; ++k) rec[k] = buf[k];
    rec[16] = sum; ri[17] = pos; ri[18] = cnt; ri[19] = fc; ri[20] = st; ri[21] = sp; ri[22] = si; ri[23] = hit; ri[24] = last_start; ri[25] = last_end;
}
}  // namespace firered
}  // namespace vadx

extern "C" size_t vadx_stream_vadpost_state_bytes(int streams) { return streams > 0 ? (size_t)streams * vadx::firered::SP_WORDS * 4 : 0; }

extern "C" int vadx_stream_vadpost(const vadx_stream_vadpost_params *prm, const float *probs, int64_t probs_stride, int frames, int streams,
                                   void *state, int reset, int flush, int32_t *segments, int32_t *counts, int cap, void *stream) {
    VADX_REQUIRE(prm && probs && state && segments && counts, "vadx_stream_vadpost: NULL argument");
    VADX_REQUIRE(streams > 0 && frames >= 0 && cap > 0 && probs_stride >= frames, "vadx_stream_vadpost: streams / frames / cap / stride");
    vadx::firered::StreamPostDev q;
    q.ws = prm->smooth_window_size < 1 ? 1 : prm->smooth_window_size;
    VADX_REQUIRE(q.ws <= vadx::firered::SP_MAXWS, "vadx_stream_vadpost: smooth_window_size %d > %d", q.ws, vadx::firered::SP_MAXWS);
    q.thr = prm->speech_threshold;
    q.pad_start = prm->pad_start_frame > q.ws ? prm->pad_start_frame : q.ws;
    q.min_sp = prm->min_speech_frame; q.max_sp = prm->max_speech_frame; q.min_si = prm->min_silence_frame;
    hipLaunchKernelGGL(vadx::firered::stream_vadpost_kernel, dim3((streams + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), q, probs,
                       (long long)probs_stride, frames, streams, static_cast<float *>(state), reset, flush, segments, counts, cap);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_firered_stream_run(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams,
                                       const float *caches_in, float *caches_out, float *probs, void *stream) {
    Dev d;
    VADX_REQUIRE(cfg && packed && logmel && caches_in && caches_out && probs, "vadx_firered_stream_run: NULL argument");
    VADX_REQUIRE(derive(cfg, &d) == 0, "vadx_firered_stream_run: unsupported config");
    VADX_REQUIRE(cfg->N2 == 0, "vadx_firered_stream_run: the streaming model has no look-ahead filter (N2 must be 0)");
    VADX_REQUIRE(streams > 0 && caches_in != caches_out, "vadx_firered_stream_run: streams must be positive, caches must not alias");
    VADX_DYN_LDS(firered_stream_kernel, LDS_FLOATS * sizeof(float));
    hipLaunchKernelGGL(firered_stream_kernel, dim3(streams), dim3(THREADS), LDS_FLOATS * sizeof(float),
                       static_cast<hipStream_t>(stream), d, packed, logmel, caches_in, caches_out, streams, probs);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}


// ---- FireRed Stream-VAD for S live streams (FireRedVAD/Inference_FireRed_ONNX.py:744-822): one tick = `chunks` chunks of cfg->frames
// frames per stream, the FIR caches and the StreamVadPostprocessor state carried in a device record.  A workgroup serves `group` streams:
// their F = chunks * frames columns lie side by side in the LDS rows ([channel][stream slot * F + frame]), so one load of the weight
// fragments (resident or streamed) serves all of them.  The point-wise layers are per column; the FIR of a stream reads its own cache for
// the frames before its own first column, never a neighbour's columns; the decisions run one lane per stream once the probabilities are in
// LDS.  Nothing a stream receives depends on `group`, on S, on its neighbours or on their masks.
namespace vadx {
namespace firered {
constexpr int TK_HDR = 32;               // header words per stream: [0,26) as the stream_vadpost record, with last_start / last_end stored + 1 (so that
                                         // zero bytes are the reset state); 28..29 frames done (int64); the rest zero
constexpr int TK_DONE = 28;
constexpr int TK_LDS_FLOATS = LDS_FLOATS + 2 * MAX_T;        // + slot status [MAX_T] (int) + channel-0 probabilities [MAX_T]

constexpr int TKR_TABLES = 5;            // ragged tick, per slot: first column, columns, stream, (log-mel row = probability column) - column; per column: slot
constexpr int TKR_LDS_FLOATS = TK_LDS_FLOATS + TKR_TABLES * MAX_T + 4;      // + the workgroup's column count

struct TickArgs {
    const float *logmel;
    const unsigned char *reset, *active;
    const unsigned *cin, *hin;           // record sections of state_in: caches [S][R][P][pad], headers [S][TK_HDR]
    unsigned *cout, *hout;
    float *probs;
    int *segs, *counts, *open_start;
    int S, F, group, cap, NC;            // NC = R * P * pad floats of cache per stream
    StreamPostDev q;
};

// The tables of a ragged tick (vadx_firered_stream_tick_ragged), all on the device; the rectangular instantiation takes the empty twin.
struct TickNoTabs {};
struct TickTabs {
    const int *counts, *row_first, *slot_stream, *wg_first;
    unsigned *status;
    int n_wg, n_rows, frames;
};
template <bool RG> struct TickTabsFor { typedef TickNoTabs type; };
template <> struct TickTabsFor<true> { typedef TickTabs type; };

// the workgroup-local Dev of a ragged tick: what the point-wise pairs read of a Dev, T = this workgroup's columns (a whole modified copy
// of the kernel's Dev would live in scratch, 656 bytes a lane: its offset tables are indexed by the block)
struct TickDims { int T, Hp, Pp; };
template <bool RG> struct TickDimsFor { typedef TickNoTabs type; };
template <> struct TickDimsFor<true> { typedef TickDims type; };
__device__ __forceinline__ const Dev &tick_dims(const Dev &d, const TickNoTabs &) { return d; }          // what the point-wise pairs of a tick read
__device__ __forceinline__ const TickDims &tick_dims(const Dev &, const TickDims &dl) { return dl; }

// A ragged workgroup's column map in LDS: slot j holds stream ss[j] in the fj[j] columns from c0[j]; column c belongs to slot cs[c] and is
// log-mel row / probability column lm[slot] + c.  Empty in the rectangular instantiation, where slot j = columns [j * F, (j + 1) * F) of
// stream g0 + j.
struct TickNoMap {};
struct TickMap { const int *c0, *fj, *ss, *lm, *cs; };
template <bool RG> struct TickMapFor { typedef TickNoMap type; };
template <> struct TickMapFor<true> { typedef TickMap type; };

// a stream's count as the ragged tick takes it: -1 when the tables lie about it (count outside [0, 112 / frames], rows outside [0, n_rows))
__device__ __forceinline__ int tick_ragged_count(const TickTabs &rt, int s) {
    const int n = rt.counts[s];
    const long long r0 = rt.row_first[s];
    return n < 0 || n > MAX_T / rt.frames || r0 < 0 || r0 + n > rt.n_rows ? -1 : n;
}

// fsmn_memory_stream for the columns of `group` streams: same operations in the same order per (channel, frame); slot status 0 = no audio
// (the columns stay zero), 1 = live, 2 = live from the reset state (zero cache)
template <bool RG>
__device__ __forceinline__ void fsmn_memory_tick(const Dev &d, int C, const float *__restrict__ Pk, int r, bool skip, const float *p, float *mem,
                                                 const TickArgs &a, int g0, const int *slot, const typename TickMapFor<RG>::type &m) {
    const int pad = (d.N1 - 1) * d.S1;              // C = the workgroup's columns
    const float *cin = reinterpret_cast<const float *>(a.cin);
    float *cout = reinterpret_cast<float *>(a.cout);
    for (int e = threadIdx.x; e < d.P * C; e += THREADS) {
        const int ch = e / C, c = e - ch * C;
        int j, cb, s;                                      // the column's slot, that slot's first column and its stream
        if constexpr (RG) { j = m.cs[c]; cb = m.c0[j]; s = m.ss[j]; }
        else { j = c / a.F; cb = j * a.F; s = g0 + j; }
        const int t = c - cb, st = slot[j];
        if (st == 0) continue;
        const float *row = p + ch * M_LD + cb, *crow = cin + (size_t)s * a.NC + ((size_t)r * d.P + ch) * pad, *w = Pk + d.off_lb[r] + ch * d.N1;
        float lb = 0.f;
        for (int k = 0; k < d.N1; ++k) {
            const int i = t + k * d.S1;                       // index into cache ++ p
            lb = fmaf(w[k], i < pad ? (st == 2 ? 0.f : crow[i]) : row[i - pad], lb);
        }
        float s2 = row[t] + lb;
        if (skip) s2 += mem[ch * M_LD + c];
        mem[ch * M_LD + c] = s2;
    }
    const int per = d.P * pad;
    for (int e = threadIdx.x; e < a.group * per; e += THREADS) {      // new cache = last `pad` entries of cache ++ p
        const int j = e / per, x = e - j * per, ch = x / pad, i = x - ch * pad, st = slot[j];
        if (st == 0) continue;
        int F, cb, s;
        if constexpr (RG) { F = m.fj[j]; cb = m.c0[j]; s = m.ss[j]; }
        else { F = a.F; cb = j * a.F; s = g0 + j; }
        const int src = F + i;
        const size_t at = (size_t)s * a.NC + (size_t)r * per + x;
        cout[at] = src < pad ? (st == 2 ? 0.f : cin[at - i + src]) : p[ch * M_LD + cb + src - pad];
    }
}

// One stream's decisions over its F new probabilities: stream_vadpost_kernel's per-frame loop (flush = 0), operation for operation, on the
// tick record's header.  F is the stream's own frame count this tick (a.F in a rectangular one).
__device__ __forceinline__ void tick_decide(const TickArgs &a, int s, bool fresh, const float *pr, int F) {
    const StreamPostDev &q = a.q;
    const unsigned *hi = a.hin + (size_t)s * TK_HDR;
    unsigned *ho = a.hout + (size_t)s * TK_HDR;
    float buf[SP_MAXWS];
    float sum = 0.f;
    int pos = 0, cnt = 0, fc = 0, st = 0, sp = 0, si = 0, hit = 0, last_start = -1, last_end = -1;
    long long done = 0;
#pragma unroll
    for (int k = 0; k < SP_MAXWS; ++k) buf[k] = fresh ? 0.f : __uint_as_float(hi[k]);
    if (!fresh) {
        sum = __uint_as_float(hi[16]); pos = (int)hi[17]; cnt = (int)hi[18]; fc = (int)hi[19]; st = (int)hi[20]; sp = (int)hi[21]; si = (int)hi[22];
        hit = (int)hi[23]; last_start = (int)hi[24] - 1; last_end = (int)hi[25] - 1;
        done = (long long)(((unsigned long long)hi[TK_DONE + 1] << 32) | hi[TK_DONE]);
    }
    int *out = a.segs + (size_t)s * a.cap * 2, n = 0;
    auto emit = [&](int x, int y) { if (n < a.cap) { out[2 * n] = x; out[2 * n + 1] = y; } ++n; };
    for (int t = 0; t < F; ++t) {
        const float p = pr[t];
        ++fc;
        float sm = p;
        if (q.ws > 1) {
            float old = 0.f;
#pragma unroll
            for (int k = 0; k < SP_MAXWS; ++k) if (k == pos) { old = buf[k]; buf[k] = p; }      // (register array: no dynamic indexing)
            sum = __fadd_rn(sum, __fsub_rn(p, old));
            pos = pos + 1 == q.ws ? 0 : pos + 1;
            if (cnt < q.ws) ++cnt;
            sm = __fdiv_rn(sum, (float)cnt);
        }
        const bool speech = sm >= q.thr;
        int e0 = 0, e1 = 0;
        bool ended = false;
        if (hit) { last_start = fc; hit = 0; }           // a forced split re-opens a segment on the next frame
        auto close = [&]() { e0 = last_start; e1 = fc; ended = true; last_start = -1; last_end = fc; };
        if (st == 0) {
            if (speech) { st = 1; sp = 1; } else { ++si; sp = 0; }
        } else if (st == 1) {
            if (speech) {
                ++sp;
                if (sp >= q.min_sp) {
                    st = 2;
                    int b = fc - sp + 1 - q.pad_start;
                    b = b < 1 ? 1 : b;
                    last_start = b > last_end + 1 ? b : last_end + 1;
                    si = 0;
                }
            } else { st = 0; si = 1; sp = 0; }
        } else {
            ++sp;
            if (speech) {
                st = 2; si = 0;
                if (sp >= q.max_sp) { hit = 1; sp = 0; close(); }
            } else if (st == 2) { st = 3; si = 1; }
            else {
                ++si;
                if (si >= q.min_si) { st = 0; sp = 0; close(); }
            }
        }
        if (ended && e0 > 0) emit(e0 - 1 > 0 ? e0 - 1 : 0, e1 - 1 > 0 ? e1 - 1 : 0);
    }
    done += F;
    a.counts[s] = n;
    a.open_start[s] = last_start > 0 ? last_start - 1 : -1;      // what the end-of-input rule would report, without closing it
#pragma unroll
    for (int k = 0; k < SP_MAXWS; ++k) ho[k] = __float_as_uint(buf[k]);
    ho[16] = __float_as_uint(sum); ho[17] = pos; ho[18] = cnt; ho[19] = fc; ho[20] = st; ho[21] = sp; ho[22] = si; ho[23] = hit;
    ho[24] = last_start + 1; ho[25] = last_end + 1; ho[26] = 0; ho[27] = 0;
    ho[TK_DONE] = (unsigned)((unsigned long long)done & 0xffffffffull); ho[TK_DONE + 1] = (unsigned)((unsigned long long)done >> 32);
    ho[30] = 0; ho[31] = 0;
}

// RG = a ragged tick: workgroup w < rt.n_wg serves the streams slot_stream[wg_first[w] .. wg_first[w + 1]), slot j with counts[s_j] *
// frames columns behind those of the slots before it; workgroup rt.n_wg + s copies the record of stream s when it has no audio.
template <int AR, bool RG>
__global__ __launch_bounds__(THREADS, 2) void firered_stream_tick_kernel(Dev d, const float *__restrict__ Pk, TickArgs a,
                                                                         typename TickTabsFor<RG>::type rt) {
    constexpr bool SPLIT = AR != vadx::VADX_AR_F32;
    typedef typename vadx::SchemeFor<AR>::type SC;
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *mem = lds, *p = lds + MEM_F, *h = p + P_F, *pr0 = h + H_F + MAX_T;
    int *slot = reinterpret_cast<int *>(h + H_F);
    typename TickMapFor<RG>::type m;
    typename TickDimsFor<RG>::type dl;           // RG: the point-wise helpers' Dev, with this workgroup's own column count
    const int tid = threadIdx.x, F = a.F;
    int g0 = blockIdx.x * a.group, C = d.T;      // d.T = group * F columns
    if constexpr (RG) {
        int *tab = reinterpret_cast<int *>(pr0 + MAX_T);
        int *c0 = tab, *fj = tab + MAX_T, *ss = tab + 2 * MAX_T, *lmb = tab + 3 * MAX_T, *cs = tab + 4 * MAX_T, *cw = tab + TKR_TABLES * MAX_T;
        m = TickMap{c0, fj, ss, lmb, cs};
        const int w = blockIdx.x;
        if (w >= rt.n_wg) {
            // a stream without audio (count 0, or a count / rows the tables lie about): the record bit for bit, no segment
            const int s = w - rt.n_wg, n = tick_ragged_count(rt, s);
            if (n < 0 && tid == 0) atomicOr(rt.status, 2u);
            if (n > 0) return;
            for (int e = tid; e < a.NC; e += THREADS) { const size_t at = (size_t)s * a.NC + e; a.cout[at] = a.cin[at]; }
            if (tid < TK_HDR) a.hout[(size_t)s * TK_HDR + tid] = a.hin[(size_t)s * TK_HDR + tid];
            if (tid == 0) { a.counts[s] = 0; a.open_start[s] = -1; }
            return;
        }
        const int j0 = rt.wg_first[w], j1 = rt.wg_first[w + 1], ns = j1 - j0;      // uniform loads
        if (j0 < 0 || ns < 0 || ns > MAX_T || j1 > a.S) {                         // (slot_stream names a stream at most once: <= S entries)
            if (tid == 0) atomicOr(rt.status, 2u);
            return;
        }
        if (tid < MAX_T) {
            int s = -1, n = 0;
            if (tid < ns) {
                s = rt.slot_stream[j0 + tid];
                n = s < 0 || s >= a.S ? -1 : tick_ragged_count(rt, s);
                if (n < 0) { atomicOr(rt.status, 2u); n = 0; }
            }
            fj[tid] = n * rt.frames;
            ss[tid] = s;
        }
        if (tid == 0) *cw = 0;
        __syncthreads();
        if (tid < ns) {
            int c = 0;
            for (int i = 0; i < tid; ++i) c += fj[i];
            const int f = fj[tid], s = ss[tid];
            const bool live = f > 0 && c + f <= MAX_T;          // columns past 112: this slot is skipped, and so is every one behind it
            if (f > 0 && !live) atomicOr(rt.status, 2u);
            slot[tid] = !live ? 0 : (a.reset && a.reset[s]) ? 2 : 1;
            c0[tid] = c;
            if (live) {
                lmb[tid] = rt.row_first[s] * rt.frames - c;
                for (int i = 0; i < f; ++i) cs[c + i] = tid;
                atomicMax(cw, c + f);
            }
        }
        __syncthreads();
        C = __builtin_amdgcn_readfirstlane(*cw);
        if (C == 0) return;
        dl.Hp = d.Hp; dl.Pp = d.Pp;
        dl.T = C;                                                // the helpers' column count: this workgroup's own, wave-uniform
        a.group = ns;                                            // its slots
        g0 = 0;
    } else {
        if (tid < a.group) {
            const int s = g0 + tid;
            const bool live = s < a.S && (!a.active || a.active[s]);
            slot[tid] = !live ? 0 : (a.reset && a.reset[s]) ? 2 : 1;
        }
        __syncthreads();
        // streams without audio: the record bit for bit, NaN probabilities, no segment
        bool any = false;
        for (int j = 0; j < a.group; ++j) any |= slot[j] != 0;
        for (int e = tid; e < a.group * a.NC; e += THREADS) {
            const int j = e / a.NC;
            if (g0 + j < a.S && slot[j] == 0) { const size_t at = (size_t)g0 * a.NC + e; a.cout[at] = a.cin[at]; }
        }
        for (int e = tid; e < a.group * d.odim * F; e += THREADS) {
            const int j = e / (d.odim * F);
            if (g0 + j < a.S && slot[j] == 0) a.probs[(size_t)g0 * d.odim * F + e] = __uint_as_float(0x7fc00000u);
        }
        if (tid < a.group && g0 + tid < a.S && slot[tid] == 0) {
            const size_t at = (size_t)(g0 + tid) * TK_HDR;
            for (int k = 0; k < TK_HDR; ++k) a.hout[at + k] = a.hin[at + k];
            a.counts[g0 + tid] = 0;
            a.open_start[g0 + tid] = -1;
        }
        if (!any) return;
    }
    const auto &dh = tick_dims(d, dl);
    // stage log-mel channel-first into `mem` rows 0..79, the streams' chunks side by side; columns without audio and >= C are zero
    for (int e = tid; e < MAX_T * NMEL; e += THREADS) {
        const int c = e / NMEL, mel = e - c * NMEL;
        float v = 0.f;
        if constexpr (RG) { if (c < C) v = a.logmel[(size_t)(m.lm[m.cs[c]] + c) * NMEL + mel]; }      // every column below C is a live slot's
        else if (c < C && slot[c / F] != 0) v = a.logmel[((size_t)g0 * F + c) * NMEL + mel];
        mem[mel * M_LD + c] = v;
    }
    for (int e = tid; e < MAXP * M_LD; e += THREADS) p[e] = 0.f;
    __syncthreads();
    if (SPLIT) pointwise_pair_split<SC, 3>(dh, Pk + d.q_fc1, Pk + d.off_fc1b, NMEL, mem, Pk + d.q_fc2, Pk + d.off_fc2b, true, p, h, amax);
    else pointwise_pair(dh, Pk + d.off_fc1, Pk + d.off_fc1b, NMEL / 16, mem, Pk + d.off_fc2, Pk + d.off_fc2b, 1, p, h);
    for (int e = tid; e < MAXP * M_LD; e += THREADS) mem[e] = 0.f;
    __syncthreads();
    fsmn_memory_tick<RG>(d, C, Pk, 0, false, p, mem, a, g0, slot, m);
    __syncthreads();
    for (int r = 1; r < d.R; ++r) {
        if (SPLIT) pointwise_pair_split<SC, 4>(dh, Pk + d.q_bfc1[r], Pk + d.off_bfc1b[r], d.Pp, mem, Pk + d.q_bfc2[r], nullptr, false, p, h, amax);
        else pointwise_pair(dh, Pk + d.off_bfc1[r], Pk + d.off_bfc1b[r], d.Pp / 16, mem, Pk + d.off_bfc2[r], nullptr, 0, p, h);
        fsmn_memory_tick<RG>(d, C, Pk, r, true, p, mem, a, g0, slot, m);
        __syncthreads();
    }
    auto put = [&](int o, int c, float z) {        // logit of output o at column c -> probs [S][odim][F], channel 0 also to the decision lanes
        if constexpr (RG) {                        // -> probs [odim][n_rows * frames]; every column below C is a live slot's
            const float v = sigmoidf_(z);
            a.probs[(size_t)o * rt.n_rows * rt.frames + m.lm[m.cs[c]] + c] = v;
            if (o == 0) pr0[c] = v;
        } else {
            const int j = c / F;
            if (slot[j] == 0) return;
            const float v = sigmoidf_(z);
            a.probs[((size_t)(g0 + j) * d.odim + o) * F + c - j * F] = v;
            if (o == 0) pr0[c] = v;
        }
    };
    if (SPLIT && d.M == 1) {          // as firered_kernel: dnn + output head as one more point-wise pair, logits in p[o][c]
        pointwise_pair_split<SC, 4>(dh, Pk + d.q_dnn0, Pk + d.off_dnnb[0], d.Pp, mem, Pk + d.q_head, Pk + d.off_headb, false, p, h, amax);
        __syncthreads();
        for (int e = tid; e < d.odim * C; e += THREADS) {
            const int o = e / C, c = e - o * C;
            put(o, c, p[o * M_LD + c]);
        }
    } else {                          // as firered_stream_kernel, tile by tile
        float *h2 = p;
        for (int f0 = 0; f0 < C; f0 += 32) {
            const bool half = (C - f0) <= 16;
            LayerArgs l0{Pk + d.off_dnn[0], d.Pp, d.Hp / 16, 1, d.Pp / 16, 0, 0, Pk + d.off_dnnb[0], 1, mem, M_LD, f0, h, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(l0); else layer<2, false>(l0);
            __syncthreads();
            float *cur = h, *nxt = h2;
            for (int m = 1; m < d.M; ++m) {
                LayerArgs lm_{Pk + d.off_dnn[m], d.Hp, d.Hp / 16, 1, d.Hp / 16, 0, 0, Pk + d.off_dnnb[m], 1, cur, H_LD, 0, nxt, H_LD, 0, nullptr, nullptr};
                if (half) layer<1, false>(lm_); else layer<2, false>(lm_);
                __syncthreads();
                float *tmp = cur; cur = nxt; nxt = tmp;
            }
            float *lg = p + MAXH * H_LD;            // behind h2
            {   LayerArgs o{Pk + d.off_out, d.Hp, 1, 1, d.Hp / 16, 0, 0, Pk + d.off_outb, 0, cur, H_LD, 0, lg, H_LD, 0, nullptr, nullptr};
                if (half) layer<1, false>(o); else layer<2, false>(o); }
            __syncthreads();
            if (tid < 32 * d.odim) {
                const int t = tid & 31, o = tid >> 5;
                if (f0 + t < C) put(o, f0 + t, lg[o * H_LD + t]);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid < a.group && slot[tid] != 0) {         // one lane per slot, over the stream's own frames
        if constexpr (RG) tick_decide(a, m.ss[tid], slot[tid] == 2, pr0 + m.c0[tid], m.fj[tid]);
        else tick_decide(a, g0 + tid, slot[tid] == 2, pr0 + tid * F, F);
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}
}  // namespace firered
}  // namespace vadx

static size_t tick_cache_words(const Dev &d, int streams) {      // the cache section, rounded to 16 bytes
    return ((size_t)streams * d.R * d.P * (d.N1 - 1) * d.S1 + 3) & ~(size_t)3;
}

extern "C" size_t vadx_firered_stream_state_bytes(const vadx_firered_cfg *cfg, int streams) {
    Dev d;
    if (!cfg || streams <= 0) return 0;
    vadx_firered_cfg c = *cfg;
    c.frames = 1;                            // the record does not depend on the chunk length
    if (derive(&c, &d)) return 0;
    return (tick_cache_words(d, streams) + (size_t)streams * TK_HDR) * 4;
}

extern "C" int vadx_firered_stream_group_max(int frames_per_tick) {
    return frames_per_tick >= 1 && frames_per_tick <= MAX_T ? MAX_T / frames_per_tick : 0;
}

// group = 0: the most streams per workgroup that still leave every compute unit a workgroup (256 CUs, one workgroup each: the LDS rows
// take a whole CU) -- fewer workgroups than that idle part of the device, and the weight stream is cheap next to an idle CU
static int tick_group_auto(int streams, int gmax) {
    int g = streams / 256;
    return g < 1 ? 1 : (g > gmax ? gmax : g);
}

extern "C" int vadx_firered_stream_tick(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams, int chunks,
                                        int group, const vadx_stream_vadpost_params *post, const uint8_t *reset, const uint8_t *active,
                                        const void *state_in, void *state_out, float *probs, int32_t *segments, int32_t *counts, int cap,
                                        int32_t *open_start, void *stream) {
    Dev d;
    VADX_REQUIRE(cfg && packed && logmel && post && state_in && state_out && probs && segments && counts && open_start,
                 "vadx_firered_stream_tick: NULL argument");
    VADX_REQUIRE(streams >= 1 && chunks >= 1 && cap >= 1, "vadx_firered_stream_tick: streams=%d chunks=%d cap=%d must be at least 1", streams, chunks, cap);
    VADX_REQUIRE(derive(cfg, &d) == 0, "vadx_firered_stream_tick: unsupported config (or a split arithmetic on widths the split kernels do not take)");
    VADX_REQUIRE(cfg->N2 == 0, "vadx_firered_stream_tick: the streaming model has no look-ahead filter (N2 must be 0)");
    const long long F = (long long)chunks * d.T;
    VADX_REQUIRE(F <= MAX_T, "vadx_firered_stream_tick: chunks * frames = %lld exceeds the %d frames of a tick", F, MAX_T);
    const int gmax = MAX_T / (int)F;
    VADX_REQUIRE(group >= 0 && group <= gmax, "vadx_firered_stream_tick: group=%d outside [0, %d] (0 = the library's choice)", group, gmax);
    const int ws = post->smooth_window_size < 1 ? 1 : post->smooth_window_size;
    VADX_REQUIRE(ws <= SP_MAXWS, "vadx_firered_stream_tick: smooth_window_size %d > %d", ws, SP_MAXWS);
    const size_t cache_words = tick_cache_words(d, streams), bytes = (cache_words + (size_t)streams * TK_HDR) * 4;
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, bytes), "vadx_firered_stream_tick: state_in and state_out overlap");
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0,
                 "vadx_firered_stream_tick: records must be 16-byte aligned");
    TickArgs a;
    a.logmel = logmel; a.reset = reset; a.active = active;
    a.cin = static_cast<const unsigned *>(state_in); a.hin = a.cin + cache_words;
    a.cout = static_cast<unsigned *>(state_out); a.hout = a.cout + cache_words;
    a.probs = probs; a.segs = segments; a.counts = counts; a.open_start = open_start;
    a.S = streams; a.F = (int)F; a.group = group ? group : tick_group_auto(streams, gmax); a.cap = cap;
    a.NC = d.R * d.P * (d.N1 - 1) * d.S1;
    a.q.ws = ws; a.q.thr = post->speech_threshold; a.q.pad_start = post->pad_start_frame > ws ? post->pad_start_frame : ws;
    a.q.min_sp = post->min_speech_frame; a.q.max_sp = post->max_speech_frame; a.q.min_si = post->min_silence_frame;
    d.T = a.group * a.F;                     // the kernel's columns: the group's streams side by side
    const unsigned grid = (unsigned)((streams + a.group - 1) / a.group);
    const size_t lds = TK_LDS_FLOATS * sizeof(float);
    const TickNoTabs none;
    VADX_DYN_LDS((firered_stream_tick_kernel<0, false>), lds);
    VADX_DYN_LDS((firered_stream_tick_kernel<1, false>), lds);
    VADX_DYN_LDS((firered_stream_tick_kernel<2, false>), lds);
    if (d.arith == vadx::VADX_AR_H2)
        hipLaunchKernelGGL((firered_stream_tick_kernel<2, false>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, none);
    else if (d.arith == vadx::VADX_AR_B3)
        hipLaunchKernelGGL((firered_stream_tick_kernel<1, false>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, none);
    else
        hipLaunchKernelGGL((firered_stream_tick_kernel<0, false>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, none);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

// ---- ragged ticks: stream s advances by counts[s] chunks; every refusal names its argument and comes before any HIP call -------------------
extern "C" int vadx_firered_stream_tick_ragged(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams, int n_rows,
                                               const int32_t *counts, const int32_t *row_first, const int32_t *slot_stream,
                                               const int32_t *wg_first, int n_wg, const vadx_stream_vadpost_params *post, const uint8_t *reset,
                                               const void *state_in, void *state_out, float *probs, int32_t *segments, int32_t *counts_out,
                                               int cap, int32_t *open_start, uint32_t *status, void *stream) {
    const char *who = "vadx_firered_stream_tick_ragged";
    Dev d;
    VADX_REQUIRE(cfg, "%s: cfg is NULL", who);
    VADX_REQUIRE(packed, "%s: packed is NULL", who);
    VADX_REQUIRE(logmel, "%s: logmel is NULL", who);
    VADX_REQUIRE(counts, "%s: counts is NULL", who);
    VADX_REQUIRE(row_first, "%s: row_first is NULL", who);
    VADX_REQUIRE(slot_stream, "%s: slot_stream is NULL", who);
    VADX_REQUIRE(wg_first, "%s: wg_first is NULL", who);
    VADX_REQUIRE(post, "%s: post is NULL", who);
    VADX_REQUIRE(state_in, "%s: state_in is NULL", who);
    VADX_REQUIRE(state_out, "%s: state_out is NULL", who);
    VADX_REQUIRE(probs, "%s: probs is NULL", who);
    VADX_REQUIRE(segments, "%s: segments is NULL", who);
    VADX_REQUIRE(counts_out, "%s: counts_out is NULL", who);
    VADX_REQUIRE(open_start, "%s: open_start is NULL", who);
    VADX_REQUIRE(status, "%s: status is NULL", who);
    VADX_REQUIRE(streams >= 1, "%s: streams=%d must be at least 1", who, streams);
    VADX_REQUIRE(n_rows >= 1, "%s: n_rows=%d must be at least 1", who, n_rows);
    VADX_REQUIRE(n_wg >= 1, "%s: n_wg=%d must be at least 1", who, n_wg);
    VADX_REQUIRE(cap >= 1, "%s: cap=%d must be at least 1", who, cap);
    VADX_REQUIRE(cfg->frames >= 1 && cfg->frames <= MAX_T, "%s: frames=%d outside [1, %d], the frames of a tick", who, cfg->frames, MAX_T);
    VADX_REQUIRE((long long)n_rows * cfg->frames <= 0x7fffffffll, "%s: n_rows=%d rows of frames=%d frames pass 2^31 columns", who, n_rows, cfg->frames);
    VADX_REQUIRE((long long)n_wg + streams <= 0x7fffffffll, "%s: n_wg=%d + streams=%d workgroups pass 2^31", who, n_wg, streams);
    VADX_REQUIRE(derive(cfg, &d) == 0, "%s: unsupported cfg (or a split arithmetic on widths the split kernels do not take)", who);
    VADX_REQUIRE(cfg->N2 == 0, "%s: the streaming model has no look-ahead filter (N2 must be 0)", who);
    const int ws = post->smooth_window_size < 1 ? 1 : post->smooth_window_size;
    VADX_REQUIRE(ws <= SP_MAXWS, "%s: smooth_window_size %d > %d", who, ws, SP_MAXWS);
    const size_t cache_words = tick_cache_words(d, streams), bytes = (cache_words + (size_t)streams * TK_HDR) * 4;
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, bytes), "%s: state_in and state_out overlap", who);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15) == 0,
                 "%s: the records state_in / state_out must be 16-byte aligned", who);
    TickArgs a;
    a.logmel = logmel; a.reset = reset; a.active = nullptr;
    a.cin = static_cast<const unsigned *>(state_in); a.hin = a.cin + cache_words;
    a.cout = static_cast<unsigned *>(state_out); a.hout = a.cout + cache_words;
    a.probs = probs; a.segs = segments; a.counts = counts_out; a.open_start = open_start;
    a.S = streams; a.F = 0; a.group = 0; a.cap = cap;          // F and group are per workgroup, set by the kernel
    a.NC = d.R * d.P * (d.N1 - 1) * d.S1;
    a.q.ws = ws; a.q.thr = post->speech_threshold; a.q.pad_start = post->pad_start_frame > ws ? post->pad_start_frame : ws;
    a.q.min_sp = post->min_speech_frame; a.q.max_sp = post->max_speech_frame; a.q.min_si = post->min_silence_frame;
    TickTabs rt;
    rt.counts = counts; rt.row_first = row_first; rt.slot_stream = slot_stream; rt.wg_first = wg_first; rt.status = status;
    rt.n_wg = n_wg; rt.n_rows = n_rows; rt.frames = cfg->frames;
    const unsigned grid = (unsigned)n_wg + (unsigned)streams;    // the compute workgroups, then one per stream for the records without audio
    const size_t lds = TKR_LDS_FLOATS * sizeof(float);
    VADX_DYN_LDS((firered_stream_tick_kernel<0, true>), lds);
    VADX_DYN_LDS((firered_stream_tick_kernel<1, true>), lds);
    VADX_DYN_LDS((firered_stream_tick_kernel<2, true>), lds);
    if (d.arith == vadx::VADX_AR_H2)
        hipLaunchKernelGGL((firered_stream_tick_kernel<2, true>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, rt);
    else if (d.arith == vadx::VADX_AR_B3)
        hipLaunchKernelGGL((firered_stream_tick_kernel<1, true>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, rt);
    else
        hipLaunchKernelGGL((firered_stream_tick_kernel<0, true>), dim3(grid), dim3(THREADS), lds, static_cast<hipStream_t>(stream), d, packed, a, rt);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}


// ---- windows of ANY length (include/vadx.h: vadx_firered_run_long).  The reference exports the graph at any INPUT_AUDIO_LENGTH or with
// a dynamic axis (FireRedVAD/Export_FireRedVAD.py:29,48,785-807) and runs one window per file (Inference_FireRed_ONNX.py:541-547,
// :644-650); a window of T frames no longer lives in one workgroup's LDS.  The activations live in a global workspace -- per batch `p`
// (two planes, ping-pong) and `mem` (one plane), each f32 [P][frames_total], clip b's frames at columns frame_first[b] .. -- and the
// grid is (window, tile of 64 frames).  R + 1 launches:
//   head        log-mel tile -> fc1 / fc2 pair -> p_0 tile (point-wise: no halo)
//   block r     FIR over p_r read from the workspace with guards (frames < 0 or >= T contribute nothing: a window edge zero-pads the
//               filter), + the skip from the tile's own mem_(r-1), mem_r written in place; then the point-wise pair of block r + 1 on the
//               tile -> the other p plane, or (r = R - 1) dnn + head + sigmoid -> the probabilities.
// A launch boundary is the only ordering the FIR needs: block r reads p_r (all written by the launch before) and writes p_(r+1) to the
// other plane; mem is read and written at the tile's own frames only.
// The bytes of a frame do not depend on the tile or launch that computed it: the point-wise pairs are the device functions of
// firered_kernel (every output column depends on its own input column only), and the FIR sums per frame in fsmn_memory's order --
// look-back taps oldest first, look-ahead taps nearest first, (p + lb) + la, then the skip.  fma(w, 0, acc) = acc for finite w, so a
// guarded tap and fsmn_memory_fast's zero-masked tap are the same number -- but for the sign of a zero: fma(w, 0, -0) is +0 where the
// skipped tap keeps -0.  The accumulators start at +0 and +0 + -0 = +0, so an accumulator is -0 only after a product that underflowed
// to -0, and the sign would show only in a frame whose p is -0 as well; the bitwise tests have not met it.
namespace vadx {
namespace firered {
constexpr int LONG_TILE = VADX_FIRERED_LONG_TILE;
static_assert(LONG_TILE == 64 && LONG_TILE <= MAX_T, "a tile's columns lie in the M_LD rows");

struct LongTabs {
    const int *frame_first, *tile_first, *tile_clip;
    int clips, n_tiles, frames_total, max_frames;
};

struct LongTile {
    long long col;          // the tile's first frame as a column of the workspace planes, the log-mel rows and the probabilities
    int T, t0, n;           // the window's frames, the tile's first frame in its window, the tile's frames (0: the tables lie, do nothing)
};

// (clip, tile) of this workgroup by two uniform loads, as the other ragged kernels; a workgroup whose entries lie -- a clip outside
// [0, clips), a tile outside its clip, an empty or decreasing prefix, a range beyond the totals, a window above the cap, a tile count that
// disagrees with the frame count -- gets n = 0 and returns before its first read or write of the buffers
__device__ __forceinline__ LongTile long_tile(const LongTabs &tb) {
    LongTile k{0, 0, 0, 0};
    const int w = blockIdx.x;
    if (w >= tb.n_tiles) return k;
    const int b = tb.tile_clip[w];
    if (b < 0 || b >= tb.clips) return k;
    const int tf0 = tb.tile_first[b], tf1 = tb.tile_first[b + 1], ff0 = tb.frame_first[b], ff1 = tb.frame_first[b + 1];
    if (tf0 < 0 || w < tf0 || w >= tf1 || ff0 < 0 || ff1 <= ff0 || ff1 > tb.frames_total) return k;
    const int T = ff1 - ff0;
    if (T > tb.max_frames || tf1 - tf0 != (T + LONG_TILE - 1) / LONG_TILE) return k;
    k.T = T;
    k.t0 = (w - tf0) * LONG_TILE;
    k.n = T - k.t0 < LONG_TILE ? T - k.t0 : LONG_TILE;
    k.col = (long long)ff0 + k.t0;
    return k;
}

// LDS rows [channel][tile column] <-> a workspace plane [P][frames_total] (64-bit offsets: 4096 clips of 10 s pass 2^31 bytes a plane)
__device__ __forceinline__ void long_store_tile(const Dev &d, const LongTile &k, const LongTabs &tb, const float *rows, float *plane) {
    for (int e = threadIdx.x; e < d.P * LONG_TILE; e += THREADS) {
        const int ch = e / LONG_TILE, u = e - ch * LONG_TILE;
        if (u < k.n) plane[(size_t)ch * tb.frames_total + k.col + u] = rows[ch * M_LD + u];
    }
}

template <int AR>
__global__ __launch_bounds__(THREADS, 2) void firered_long_head_kernel(Dev d, const float *__restrict__ Pk, const float *__restrict__ logmel,
                                                                       LongTabs tb, float *__restrict__ ws) {
    constexpr bool SPLIT = AR != vadx::VADX_AR_F32;
    typedef typename vadx::SchemeFor<AR>::type SC;
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *mem = lds, *p = lds + MEM_F, *h = p + P_F;
    const int tid = threadIdx.x;
    const LongTile k = long_tile(tb);
    if (k.n == 0) return;
    const TickDims dl{k.n, d.Hp, d.Pp};
    for (int e = tid; e < MAXP * M_LD; e += THREADS) { mem[e] = 0.f; p[e] = 0.f; }
    __syncthreads();
    const float *lm = logmel + (size_t)k.col * NMEL;
    for (int e = tid; e < k.n * NMEL; e += THREADS) {
        const int u = e / NMEL, mel = e - u * NMEL;
        mem[mel * M_LD + u] = lm[e];
    }
    __syncthreads();
    if (SPLIT) pointwise_pair_split<SC, 3>(dl, Pk + d.q_fc1, Pk + d.off_fc1b, NMEL, mem, Pk + d.q_fc2, Pk + d.off_fc2b, true, p, h, amax);
    else pointwise_pair(dl, Pk + d.off_fc1, Pk + d.off_fc1b, NMEL / 16, mem, Pk + d.off_fc2, Pk + d.off_fc2b, 1, p, h);
    __syncthreads();
    long_store_tile(d, k, tb, p, ws);                                  // p_0 -> plane 0
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}

template <int AR>
__global__ __launch_bounds__(THREADS, 2) void firered_long_block_kernel(Dev d, const float *__restrict__ Pk, LongTabs tb, float *__restrict__ ws,
                                                                        int r, float *__restrict__ probs) {
    constexpr bool SPLIT = AR != vadx::VADX_AR_F32;
    typedef typename vadx::SchemeFor<AR>::type SC;
    float amax = 0.f;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *mem = lds, *p = lds + MEM_F, *h = p + P_F;
    const int tid = threadIdx.x;
    const LongTile k = long_tile(tb);
    if (k.n == 0) return;
    const TickDims dl{k.n, d.Hp, d.Pp};
    const size_t plane = (size_t)d.P * tb.frames_total;
    const float *pin = ws + (size_t)(r & 1) * plane;
    float *pout = ws + (size_t)((r + 1) & 1) * plane, *gmem = ws + 2 * plane;
    for (int e = tid; e < MAXP * M_LD; e += THREADS) { mem[e] = 0.f; p[e] = 0.f; }
    __syncthreads();
    {   // the FIR of block r and the skip: thread = (channel, frame of the tile), taps from the blob, p_r from the workspace
        // the reference's T > 1 rule for the look-ahead (Export_FireRedVAD.py:229); where fsmn_memory takes its merged-window path the
        // look-ahead sum is added even when it is empty, and so it is here
        const bool ahead = d.N2 > 0 && k.T > 1;
        const bool add_la = ahead || (d.S1 == 1 && d.N1 <= 20 && (d.N2 == 0 || d.S2 == 1) && d.N2 <= 20 && k.T > 1 && d.Pp <= 128);
        const float *wl = Pk + d.off_lb[r], *wa = Pk + d.off_la[r];
        for (int e = tid; e < d.P * LONG_TILE; e += THREADS) {
            const int ch = e / LONG_TILE, u = e - ch * LONG_TILE;
            if (u >= k.n) continue;
            const int t = k.t0 + u;
            const float *row = pin + (size_t)ch * tb.frames_total + (k.col - k.t0);      // the window's frame 0 of this channel
            float lb = 0.f, la = 0.f;
            for (int j = 0; j < d.N1; ++j) {
                const long long idx = (long long)t + (long long)(j - (d.N1 - 1)) * d.S1;
                if (idx >= 0) lb = fmaf(wl[ch * d.N1 + j], row[idx], lb);
            }
            float s = row[t] + lb;
            if (ahead)
                for (int j = 0; j < d.N2; ++j) {
                    const long long idx = (long long)t + d.S2 + (long long)j * d.S2;
                    if (idx < k.T) la = fmaf(wa[ch * d.N2 + j], row[idx], la);
                }
            if (add_la) s += la;
            const size_t at = (size_t)ch * tb.frames_total + k.col + u;
            if (r > 0) s += gmem[at];
            gmem[at] = s;
            mem[ch * M_LD + u] = s;
        }
    }
    __syncthreads();
    if (r + 1 < d.R) {       // DFSMNBlock r + 1: fc1 (P->H, ReLU) ; fc2 (H->P, no bias) -> p_(r+1), the other plane
        if (SPLIT) pointwise_pair_split<SC, 4>(dl, Pk + d.q_bfc1[r + 1], Pk + d.off_bfc1b[r + 1], d.Pp, mem, Pk + d.q_bfc2[r + 1], nullptr, false, p, h, amax);
        else pointwise_pair(dl, Pk + d.off_bfc1[r + 1], Pk + d.off_bfc1b[r + 1], d.Pp / 16, mem, Pk + d.off_bfc2[r + 1], nullptr, 0, p, h);
        __syncthreads();
        long_store_tile(d, k, tb, p, pout);
        if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
        return;
    }
    // dnn + output head + sigmoid, as firered_kernel's tail -> probs [odim][frames_total]
    if (SPLIT && d.M == 1) {
        pointwise_pair_split<SC, 4>(dl, Pk + d.q_dnn0, Pk + d.off_dnnb[0], d.Pp, mem, Pk + d.q_head, Pk + d.off_headb, false, p, h, amax);
        __syncthreads();
        for (int e = tid; e < d.odim * k.n; e += THREADS) {
            const int o = e / k.n, u = e - o * k.n;
            probs[(size_t)o * tb.frames_total + k.col + u] = sigmoidf_(p[o * M_LD + u]);
        }
        if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
        return;
    }
    float *h2 = p;
    const bool dnn_resident = d.Hp == 256 && d.Pp == 128 && blockDim.x == 512;
    PairResident<8> RD;
    if (dnn_resident) load_pair_resident<8, false>(RD, Pk + d.off_dnn[0], Pk + d.off_dnnb[0], nullptr, nullptr);
    for (int f0 = 0; f0 < k.n; f0 += 32) {
        const bool half = (k.n - f0) <= 16;
        if (dnn_resident) {
            if (half) pair_tile_resident<1, 8, false>(RD, mem, nullptr, h, f0, false);
            else pair_tile_resident<2, 8, false>(RD, mem, nullptr, h, f0, false);
        } else {
            LayerArgs a{Pk + d.off_dnn[0], d.Pp, d.Hp / 16, 1, d.Pp / 16, 0, 0, Pk + d.off_dnnb[0], 1, mem, M_LD, f0, h, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(a); else layer<2, false>(a);
            __syncthreads();
        }
        float *cur = h, *nxt = h2;
        for (int m = 1; m < d.M; ++m) {
            LayerArgs c{Pk + d.off_dnn[m], d.Hp, d.Hp / 16, 1, d.Hp / 16, 0, 0, Pk + d.off_dnnb[m], 1, cur, H_LD, 0, nxt, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(c); else layer<2, false>(c);
            __syncthreads();
            float *tmp = cur; cur = nxt; nxt = tmp;
        }
        float *lg = p + MAXH * H_LD;            // behind h2
        {   LayerArgs o{Pk + d.off_out, d.Hp, 1, 1, d.Hp / 16, 0, 0, Pk + d.off_outb, 0, cur, H_LD, 0, lg, H_LD, 0, nullptr, nullptr};
            if (half) layer<1, false>(o); else layer<2, false>(o); }
        __syncthreads();
        if (tid < 32 * d.odim) {
            const int u = tid & 31, o = tid >> 5;
            if (f0 + u < k.n) probs[(size_t)o * tb.frames_total + k.col + f0 + u] = sigmoidf_(lg[o * H_LD + u]);
        }
        __syncthreads();
    }
    if (AR == vadx::VADX_AR_H2) vadx::range_flag_raise(Pk + d.off_flag, amax);
}
}  // namespace firered
}  // namespace vadx

// cfg as the long entry points read it: every field under derive()'s limits but `frames`, which only has to be valid here (the tables say
// T per window) -- 1 .. VADX_FIRERED_LONG_MAX_FRAMES
static int derive_long(const vadx_firered_cfg *cfg, Dev *d) {
    vadx_firered_cfg c = *cfg;
    c.frames = 1;
    return derive(&c, d);
}

extern "C" size_t vadx_firered_long_workspace_bytes(const vadx_firered_cfg *cfg, int64_t frames_total) {
    Dev d;
    if (!cfg || frames_total < 1 || frames_total > 0x7fffffffll || derive_long(cfg, &d)) return 0;
    return (size_t)3 * d.P * (size_t)frames_total * sizeof(float);
}

extern "C" int vadx_firered_run_long(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, const vadx_firered_long_tables *tables,
                                     float *probs, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "vadx_firered_run_long";
    Dev d;
    VADX_REQUIRE(cfg, "%s: cfg is NULL", who);
    VADX_REQUIRE(packed, "%s: packed is NULL", who);
    VADX_REQUIRE(logmel, "%s: logmel is NULL", who);
    VADX_REQUIRE(tables, "%s: tables is NULL", who);
    VADX_REQUIRE(tables->frame_first, "%s: tables->frame_first is NULL", who);
    VADX_REQUIRE(tables->tile_first, "%s: tables->tile_first is NULL", who);
    VADX_REQUIRE(tables->tile_clip, "%s: tables->tile_clip is NULL", who);
    VADX_REQUIRE(probs, "%s: probs is NULL", who);
    VADX_REQUIRE(workspace, "%s: workspace is NULL", who);
    VADX_REQUIRE(cfg->frames >= 1 && cfg->frames <= VADX_FIRERED_LONG_MAX_FRAMES, "%s: cfg->frames=%d outside [1, %d], the frames of a long window", who,
                 cfg->frames, VADX_FIRERED_LONG_MAX_FRAMES);
    VADX_REQUIRE(tables->clips >= 1, "%s: tables->clips=%d must be at least 1", who, tables->clips);
    VADX_REQUIRE(tables->n_tiles >= 1, "%s: tables->n_tiles=%d must be at least 1", who, tables->n_tiles);
    VADX_REQUIRE(tables->frames_total >= 1, "%s: tables->frames_total=%d must be at least 1", who, tables->frames_total);
    // every tile has at least one of its <= 64 frames (a clip may have none: fewer than 400 samples)
    VADX_REQUIRE(tables->n_tiles <= tables->frames_total && (long long)tables->frames_total <= (long long)tables->n_tiles * LONG_TILE,
                 "%s: tables->n_tiles=%d and tables->frames_total=%d do not fit each other (n_tiles <= frames_total <= %d * n_tiles)", who,
                 tables->n_tiles, tables->frames_total, LONG_TILE);
    VADX_REQUIRE(derive_long(cfg, &d) == 0, "%s: unsupported cfg (or a split arithmetic on widths the split kernels do not take)", who);
    const size_t need = vadx_firered_long_workspace_bytes(cfg, tables->frames_total);
    if (workspace_bytes < need) {
        vadx::set_error("%s: workspace_bytes %zu B < required %zu B (vadx_firered_long_workspace_bytes)", who, workspace_bytes, need);
        return VADX_ENOSPACE;
    }
    const LongTabs tb{tables->frame_first, tables->tile_first, tables->tile_clip, tables->clips, tables->n_tiles, tables->frames_total,
                      VADX_FIRERED_LONG_MAX_FRAMES};
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *ws = static_cast<float *>(workspace);
    const size_t lds = LDS_FLOATS * sizeof(float);
    const dim3 grid((unsigned)tables->n_tiles), block(THREADS);
    VADX_DYN_LDS(firered_long_head_kernel<0>, lds);
    VADX_DYN_LDS(firered_long_head_kernel<1>, lds);
    VADX_DYN_LDS(firered_long_head_kernel<2>, lds);
    VADX_DYN_LDS(firered_long_block_kernel<0>, lds);
    VADX_DYN_LDS(firered_long_block_kernel<1>, lds);
    VADX_DYN_LDS(firered_long_block_kernel<2>, lds);
    if (d.arith == vadx::VADX_AR_H2) hipLaunchKernelGGL(firered_long_head_kernel<2>, grid, block, lds, st, d, packed, logmel, tb, ws);
    else if (d.arith == vadx::VADX_AR_B3) hipLaunchKernelGGL(firered_long_head_kernel<1>, grid, block, lds, st, d, packed, logmel, tb, ws);
    else hipLaunchKernelGGL(firered_long_head_kernel<0>, grid, block, lds, st, d, packed, logmel, tb, ws);
    VADX_HIP_TRY(hipGetLastError());
    for (int r = 0; r < d.R; ++r) {
        if (d.arith == vadx::VADX_AR_H2) hipLaunchKernelGGL(firered_long_block_kernel<2>, grid, block, lds, st, d, packed, tb, ws, r, probs);
        else if (d.arith == vadx::VADX_AR_B3) hipLaunchKernelGGL(firered_long_block_kernel<1>, grid, block, lds, st, d, packed, tb, ws, r, probs);
        else hipLaunchKernelGGL(firered_long_block_kernel<0>, grid, block, lds, st, d, packed, tb, ws, r, probs);
        VADX_HIP_TRY(hipGetLastError());
    }
    return VADX_OK;
}
