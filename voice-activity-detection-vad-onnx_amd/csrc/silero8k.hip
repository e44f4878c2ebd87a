// silero8k.hip -- Silero-VAD v5, the 8 kHz sub-network's encoder for gfx950: one tile kernel written once for the three arithmetics
// (float32 MFMAs, bf16 x 3 and fp16 x 2 split products, csrc/split_scheme.h).  Its packed blob: csrc/silero_common.h (map), csrc/silero_pack.hip.
//
// The 8 kHz network differs from the 16 kHz one only before conv2:
//   x [288] = 32 context + 256 new samples, reflect-padded right by 32 -> [320]
//   -> conv1d(basis [130][1][128], stride 64): 4 frames of 65 bins (re, im) -> |.|  [65][4]
//   -> conv1 65->128 k3 s1 p1 + ReLU -> conv2 .. conv4 and W_ih exactly as at 16 kHz.
// Work decomposition: one workgroup of eight waves per (16 clips) x (1 window).  Every GEMM has its constant operand (basis, weights) as
// the A operand, streamed from the blob as fragments, and the activations as the B operand, read from LDS as float32 rows
// [frame][clip][channel] and split by the lane that reads them (split arithmetics).  The STFT is the dense 130 x 128 product (nine
// row tiles: re bins 0..63, im bins 0..63, then re / im of bin 64 as rows 0 / 1 of the ninth), so no DFT symmetry of the basis is assumed.
// conv1 runs channels 0..63 on the matrix pipe and channel 64 (Nyquist) as a VALU term.  The output is gx in the layout the three
// recurrent kernels read ([T][G][8 waves][4 gates][64 lanes][4], b_ih + b_hh folded in), so they run unchanged.  A tile's numbers do
// not depend on the workgroup that computes it (one tile per workgroup, one instruction sequence).
#include "silero_common.h"
#include "split_scheme.h"

#include <math.h>

namespace vadx {
namespace silero {

// ---- LDS map (floats): 51 456 B per workgroup.  R0: X [16 clips][320 (+4)] -> conv1 output [4 frames][16][128 (+4)] -> conv3 output [16][64 (+4)];
// R1: |STFT| [4 frames][16][64 (+4)] + bin 64 [4][16] -> conv2 output [2][16][64 (+4)] -> conv4 output [16][128 (+4)].
constexpr int K8_THREADS = 512;
constexpr int XLD = 324, L64 = 68, L128 = 132;
constexpr int R0_F = 4 * 16 * L128;                       // 8448 >= 16 * XLD = 5184
constexpr int R1_F = 4 * 16 * L64 + 64;
constexpr int K8_LDS_BYTES = (R0_F + R1_F) * 4;
static_assert(16 * XLD <= R0_F && 2 * K8_LDS_BYTES <= 160 * 1024, "8 kHz encoder LDS map");

struct SchemeF32 {
    static constexpr int ARITH = VADX_AR_F32;
    static constexpr bool RANGE_CHECK = false;
};

// One arithmetic's operands of a K = 32 step: W = the A fragments of one (row tile, chunk), Bv = this lane's B operand (column i = lane & 15).
template <class Sch> struct Ops;
template <> struct Ops<SchemeF32> {
    static constexpr int CHUNK = 2 * FRAG;                // floats of one (row tile, chunk) in the blob
    struct W { f32x4 v[2]; };
    struct Bv { f32x4 v[2]; };
    static __device__ __forceinline__ void ldw(W &w, const float *f, int lane) {
        w.v[0] = ldg4(f + 4 * lane);
        w.v[1] = ldg4(f + FRAG + 4 * lane);
    }
    // k = 16 s + 4 q + j of the chunk (the FRAG-major weights' order)
    static __device__ __forceinline__ void ldb(Bv &b, const float *row, int q, float &) {
        b.v[0] = *reinterpret_cast<const f32x4 *>(row + 4 * q);
        b.v[1] = *reinterpret_cast<const f32x4 *>(row + 16 + 4 * q);
    }
    static __device__ __forceinline__ void mma(const W &w, const Bv &b, f32x4 &hi, f32x4 &lo) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            hi = mfma16(w.v[0][j], b.v[0][j], hi);
            lo = mfma16(w.v[1][j], b.v[1][j], lo);
        }
    }
    static __device__ __forceinline__ f32x4 join(const f32x4 hi, const f32x4 lo) { return hi + lo; }
};
template <class Sch> struct SplitOps {
    static constexpr int NP = Sch::NP;
    static constexpr int CHUNK = NP * 256;
    typedef typename Sch::frag frag;
    struct W { frag p[NP]; };
    struct Bv { frag p[NP]; };
    static __device__ __forceinline__ void ldw(W &w, const float *f, int lane) {
#pragma unroll
        for (int p = 0; p < NP; ++p) w.p[p] = Sch::ld(f + p * 256, lane);
    }
    // k = 8 q + e of the chunk, split into the NP planes here
    static __device__ __forceinline__ void ldb(Bv &b, const float *row, int q, float &amax) {
        const f32x4 x0 = *reinterpret_cast<const f32x4 *>(row + 8 * q), x1 = *reinterpret_cast<const f32x4 *>(row + 8 * q + 4);
        u32x2 pa[NP], pb[NP];
        Sch::split4(x0, pa, amax);
        Sch::split4(x1, pb, amax);
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int p = 0; p < NP; ++p) b.p[p] = __builtin_bit_cast(frag, (u32x4_{pa[p][0], pa[p][1], pb[p][0], pb[p][1]}));
    }
    static __device__ __forceinline__ void mma(const W &w, const Bv &b, f32x4 &hi, f32x4 &lo) {
        f32x4 h[1][1] = {{hi}}, l[1][1] = {{lo}};
        const frag (&a)[1][NP] = reinterpret_cast<const frag (&)[1][NP]>(w.p);
        const frag (&bb)[1][NP] = reinterpret_cast<const frag (&)[1][NP]>(b.p);
        Sch::template products<1, 1, true>(a, bb, h, l);
        hi = h[0][0];
        lo = l[0][0];
    }
    static __device__ __forceinline__ f32x4 join(const f32x4 hi, const f32x4 lo) { return Sch::join(hi, lo); }
};
template <> struct Ops<SchemeB3> : SplitOps<SchemeB3> {};
template <> struct Ops<SchemeH2> : SplitOps<SchemeH2> {};

// fragment addresses of one (row tile, chunk) in the blob, per arithmetic
template <class Sch> __device__ __forceinline__ const float *stft_w(const float *P, int rt, int kc) {
    const int o = Sch::ARITH == VADX_AR_F32 ? OFF8_SF : (Sch::ARITH == VADX_AR_B3 ? OFF8_SQ : OFF8_SH);
    return P + o + (rt * 4 + kc) * Ops<Sch>::CHUNK;
}
template <class Sch> __device__ __forceinline__ const float *c1_w(const float *P, int rt, int tap, int kc) {
    const int o = Sch::ARITH == VADX_AR_F32 ? OFF8_C1F : (Sch::ARITH == VADX_AR_B3 ? OFF8_C1Q : OFF8_C1H);
    return P + o + ((rt * 3 + tap) * 2 + kc) * Ops<Sch>::CHUNK;
}
// the shared sections, in the orders the 16 kHz kernels stream them (silero_common.h)
template <class Sch> __device__ __forceinline__ const float *c2_w(const float *P, int rt, int tap, int kc) {
    if (Sch::ARITH == VADX_AR_F32) return P + OFF_C2 + (rt * 24 + tap * 8 + 2 * kc) * FRAG;
    return P + (Sch::ARITH == VADX_AR_B3 ? OFF_Q2 : OFF_H2) + ((rt * 4 + kc) * 3 + tap) * Ops<Sch>::CHUNK;
}
template <class Sch> __device__ __forceinline__ const float *c3_w(const float *P, int rt, int th, int kc) {      // th = tap - 1
    if (Sch::ARITH == VADX_AR_F32) return P + OFF_C3 + (rt * 8 + th * 4 + 2 * kc) * FRAG;
    return P + (Sch::ARITH == VADX_AR_B3 ? OFF_Q3 : OFF_H3) + ((rt * 2 + th) * 2 + kc) * Ops<Sch>::CHUNK;
}
template <class Sch> __device__ __forceinline__ const float *c4_w(const float *P, int rt, int kc) {
    if (Sch::ARITH == VADX_AR_F32) return P + OFF_C4 + (rt * 4 + 2 * kc) * FRAG;
    return P + (Sch::ARITH == VADX_AR_B3 ? OFF_Q4 : OFF_H4) + (rt * 2 + kc) * Ops<Sch>::CHUNK;
}
template <class Sch> __device__ __forceinline__ const float *ih_w(const float *P, int ut, int g, int kc) {
    if (Sch::ARITH == VADX_AR_F32) return P + OFF_IH + ((g * 8 + ut) * 8 + 2 * kc) * FRAG;
    return P + (Sch::ARITH == VADX_AR_B3 ? OFF_QIH : OFF_HIH) + ((ut * 4 + kc) * 4 + g) * Ops<Sch>::CHUNK;
}

// Phase 0 of a ragged tile (silero_common.h: "ragged batches"), the 8 kHz sibling of stage_ragged: window `base` .. base + 287 of the sixteen
// slots of group grp into X, then the right reflect pad of 32, laid out as the rectangular phase 0 stages it.  Slot c reads its clip as that
// reads a row with n_samples = the slot's own length: zeros before the clip and beyond its end, the pad mirrored over that.  A float4 inside
// the clip is one vector load when the clip starts on a multiple of four elements (base and p are multiples of four), four single loads
// otherwise; `whole` (uniform: the window ends below the group's shortest accepted length) spares the per-float4 range test.
template <typename SampleT>
__device__ __forceinline__ void stage_ragged8k(float *X, const SampleT *__restrict__ audio, float in_scale, const RgArg<true> &rg, int grp,
                                               long long base, int tid) {
    const bool ptr_ok = (reinterpret_cast<uintptr_t>(audio) & (SampleIO<SampleT>::VEC_ALIGN - 1)) == 0;
    int shortest;
    {
        long long o_;
        rg_slot(rg, grp * 16 + (tid & 15), o_, shortest);
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) shortest = min(shortest, __shfl_xor(shortest, d));
        shortest = min(shortest, rg.t.grp_min_len[grp]);
    }
    const bool whole = base >= 0 && base + 288 <= (long long)shortest;
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        const int e = tid + K8_THREADS * it;                  // 16 clips x 72 groups of four samples
        if (e < 16 * 72) {
            const int c = e / 72, p = 4 * (e - c * 72);
            long long off;
            int len;
            if (!rg_slot(rg, grp * 16 + c, off, len) && p == 0) atomicOr(rg.t.status, 1u);
            const SampleT *src = audio + off;
            const long long idx = base + p;
            f32x4 v;
            if (ptr_ok && (off & 3) == 0 && (whole || (idx >= 0 && idx + 3 < len))) {
                v = SampleIO<SampleT>::load4(src + idx, in_scale);
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    v[jj] = (idx + jj >= 0 && idx + jj < len) ? SampleIO<SampleT>::load1(src + idx + jj, in_scale) : 0.f;
            }
            float *row = X + c * XLD;
            *reinterpret_cast<f32x4 *>(row + p) = v;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int pp = p + jj;
                if (pp >= 255 && pp <= 286) row[574 - pp] = v[jj];
            }
        }
    }
}

__device__ __forceinline__ f32x4 relu4(const f32x4 y, const f32x4 b) {
    return f32x4{fmaxf(y[0] + b[0], 0.f), fmaxf(y[1] + b[1], 0.f), fmaxf(y[2] + b[2], 0.f), fmaxf(y[3] + b[3], 0.f)};
}

// RG (a ragged batch, silero_common.h): the tile is (group, window) of the workgroup table -- RG_RUN workgroups per entry, one per window of
// the run --, the sixteen slots are staged by stage_ragged8k and the group's gx tiles lie consecutively; everything behind phase 0 is the
// rectangular kernel's code.
template <class Sch, typename SampleT, bool RG = false>
__global__ __launch_bounds__(K8_THREADS, 2) void silero8k_encode_kernel(
    const float *__restrict__ P, const SampleT *__restrict__ audio, float in_scale, long long n_samples,
    long long row_stride, long long origin, int B, int G, int T, int Gws, int g0, float *__restrict__ gx, const RgArg<RG> rg) {
    typedef Ops<Sch> O;
    extern __shared__ __attribute__((aligned(16))) float lds8[];
    float *X = lds8, *A1 = lds8, *A3 = lds8;                  // R0
    float *M1 = lds8 + R0_F, *NYQ = M1 + 4 * 16 * L64;        // R1
    float *A2 = lds8 + R0_F, *A4 = lds8 + R0_F;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, i = lane & 15;
    int grp = blockIdx.x % G, t = blockIdx.x / G;
    size_t tile = (size_t)t * Gws + g0 + grp;
    if constexpr (RG) {
        const int ent = blockIdx.x / RG_RUN;
        grp = rg.t.wg_tab[2 * ent];
        t = rg.t.wg_tab[2 * ent + 1] * RG_RUN + blockIdx.x % RG_RUN;
        if (t >= rg.t.gx_first[grp + 1] - rg.t.gx_first[grp]) return;      // (uniform) the group's last run is a partial one
        tile = (size_t)rg.t.gx_first[grp] + t;
    }
    float *dst = gx + tile * GX_TILE_FLOATS + (size_t)wave * 4 * 256 + lane * 4;

    // a blob without the 8 kHz tag (a 16 kHz blob), or one the fp16 x 2 kernels cannot run on: NaN gate pre-activations and a flag bit,
    // never plausible scores
    {
        const bool wrong_net = ldg1(P + OFF8_TAG) != TAG8K;
        const bool no_h2 = Sch::RANGE_CHECK && ldg1(P + OFF_HFLAG) == 0.f;
        if (wrong_net || no_h2) {
            if (tid == 0 && blockIdx.x == 0) atomicOr(reinterpret_cast<unsigned *>(const_cast<float *>(P)) + OFF_HFLAG + 1, wrong_net ? 4u : 2u);
            const float qnan = __builtin_nanf("");
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4 *>(dst + g * 256) = f32x4{qnan, qnan, qnan, qnan};
            return;
        }
    }
    float amax = 0.f;           // running max |x| of everything this thread splits (fp16 x 2)

    // ---------------- phase 0: the 16 windows (288 samples each) + right reflect pad of 32: X[c][288 + m] = X[c][286 - m]
    if constexpr (RG) {
        stage_ragged8k<SampleT>(X, audio, in_scale, rg, grp, (long long)t * 256 + origin, tid);
    } else {
        const long long base = (long long)t * 256 + origin;
        const bool vec_ok = ((row_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(audio) & (SampleIO<SampleT>::VEC_ALIGN - 1)) == 0) &&
                            n_samples >= 4;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int e = tid + K8_THREADS * it;              // 16 clips x 72 groups of four samples
            if (e < 16 * 72) {
                const int c = e / 72, p = 4 * (e - c * 72);
                const long long b = (long long)grp * 16 + c, idx = base + p;
                const bool bvalid = b < B;
                const SampleT *src = audio + (bvalid ? b : 0) * row_stride;
                f32x4 v;
                if (vec_ok && bvalid && idx >= 0 && idx + 3 < n_samples) {
                    v = SampleIO<SampleT>::load4(src + idx, in_scale);
                } else {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        v[jj] = (bvalid && idx + jj >= 0 && idx + jj < n_samples) ? SampleIO<SampleT>::load1(src + idx + jj, in_scale) : 0.f;
                }
                float *row = X + c * XLD;
                *reinterpret_cast<f32x4 *>(row + p) = v;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int pp = p + jj;
                    if (pp >= 255 && pp <= 286) row[574 - pp] = v[jj];
                }
            }
        }
    }
    __syncthreads();

    // ---------------- phase 1: dense STFT (K = 128) -> |.|.  Wave = (bin tile bt: re tile bt and im tile bt + 4, frames 2 fp, 2 fp + 1);
    // waves with bt = 0 also run the ninth tile (bin 64) for their two frames.
    {
        const int bt = wave & 3, fp = wave >> 2;
        const bool nyq_w = bt == 0;
        f32x4 hi[3][2], lo[3][2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int f = 0; f < 2; ++f) hi[a][f] = lo[a][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            typename O::W w[3];
            O::ldw(w[0], stft_w<Sch>(P, bt, kc), lane);
            O::ldw(w[1], stft_w<Sch>(P, bt + 4, kc), lane);
            if (nyq_w) O::ldw(w[2], stft_w<Sch>(P, 8, kc), lane);
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                typename O::Bv b;
                O::ldb(b, X + i * XLD + 64 * (2 * fp + f) + 32 * kc, q, amax);
                O::mma(w[0], b, hi[0][f], lo[0][f]);
                O::mma(w[1], b, hi[1][f], lo[1][f]);
                if (nyq_w) O::mma(w[2], b, hi[2][f], lo[2][f]);
            }
        }
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const f32x4 re = O::join(hi[0][f], lo[0][f]), im = O::join(hi[1][f], lo[1][f]);
            f32x4 m;
#pragma unroll
            for (int r = 0; r < 4; ++r) m[r] = mag_sqrt(re[r] * re[r] + im[r] * im[r]);
            *reinterpret_cast<f32x4 *>(M1 + ((2 * fp + f) * 16 + i) * L64 + 16 * bt + 4 * q) = m;
            if (nyq_w && q == 0) {
                const f32x4 n = O::join(hi[2][f], lo[2][f]);
                NYQ[(2 * fp + f) * 16 + i] = mag_sqrt(n[0] * n[0] + n[1] * n[1]);
            }
        }
    }
    __syncthreads();

    // ---------------- phase 2: conv1 65->128, k3 s1 p1, ReLU.  Wave = output channel tile; channels 0..63 on the matrix pipe (each input
    // frame's B operand serves the taps that read it), channel 64 on VALU.
    {
        const int rt = wave;
        f32x4 hi[4], lo[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) hi[f] = lo[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            typename O::W w[3];
#pragma unroll
            for (int tap = 0; tap < 3; ++tap) O::ldw(w[tap], c1_w<Sch>(P, rt, tap, kc), lane);
#pragma unroll
            for (int fi = 0; fi < 4; ++fi) {
                typename O::Bv b;
                O::ldb(b, M1 + (fi * 16 + i) * L64 + 32 * kc, q, amax);
#pragma unroll
                for (int tap = 0; tap < 3; ++tap) {
                    const int f = fi + 1 - tap;
                    if (f >= 0 && f < 4) O::mma(w[tap], b, hi[f], lo[f]);
                }
            }
        }
        f32x4 wn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) wn[r] = ldg4(P + OFF8_C1N + (16 * rt + 4 * q + r) * 4);
        const f32x4 bias = ldg4(P + OFF_B1 + 16 * rt + 4 * q);
        float nq[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) nq[f] = NYQ[f * 16 + i];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f32x4 y = O::join(hi[f], lo[f]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int tap = 0; tap < 3; ++tap) {
                    const int fi = f + tap - 1;
                    if (fi >= 0 && fi < 4) y[r] = fmaf(wn[r][tap], nq[fi], y[r]);
                }
            *reinterpret_cast<f32x4 *>(A1 + (f * 16 + i) * L128 + 16 * rt + 4 * q) = relu4(y, bias);
        }
    }
    __syncthreads();

    // ---------------- phase 3: conv2 128->64, k3 s2 p1, ReLU.  Wave = (output channel tile, output frame fo); input frames 2 fo - 1 + tap.
    {
        const int rt = wave & 3, fo = wave >> 2;
        f32x4 hi = {0.f, 0.f, 0.f, 0.f}, lo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 3; ++tap) {
            const int fi = 2 * fo - 1 + tap;
            if (fi < 0) continue;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                typename O::W w;
                O::ldw(w, c2_w<Sch>(P, rt, tap, kc), lane);
                typename O::Bv b;
                O::ldb(b, A1 + (fi * 16 + i) * L128 + 32 * kc, q, amax);
                O::mma(w, b, hi, lo);
            }
        }
        const f32x4 y = relu4(O::join(hi, lo), ldg4(P + OFF_B2 + 16 * rt + 4 * q));
        *reinterpret_cast<f32x4 *>(A2 + (fo * 16 + i) * L64 + 16 * rt + 4 * q) = y;
    }
    __syncthreads();

    // ---------------- phase 4: conv3 64->64, k3 s2 p1, ReLU (one output frame; tap 0 reads padding, taps 1, 2 read frames 0, 1)
    if (wave < 4) {
        const int rt = wave;
        f32x4 hi = {0.f, 0.f, 0.f, 0.f}, lo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int th = 0; th < 2; ++th)
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                typename O::W w;
                O::ldw(w, c3_w<Sch>(P, rt, th, kc), lane);
                typename O::Bv b;
                O::ldb(b, A2 + (th * 16 + i) * L64 + 32 * kc, q, amax);
                O::mma(w, b, hi, lo);
            }
        const f32x4 y = relu4(O::join(hi, lo), ldg4(P + OFF_B3 + 16 * rt + 4 * q));
        *reinterpret_cast<f32x4 *>(A3 + i * L64 + 16 * rt + 4 * q) = y;
    }
    __syncthreads();

    // ---------------- phase 5: conv4 64->128, k3 s1 p1, ReLU (one frame: centre tap only)
    {
        const int rt = wave;
        f32x4 hi = {0.f, 0.f, 0.f, 0.f}, lo = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            typename O::W w;
            O::ldw(w, c4_w<Sch>(P, rt, kc), lane);
            typename O::Bv b;
            O::ldb(b, A3 + i * L64 + 32 * kc, q, amax);
            O::mma(w, b, hi, lo);
        }
        const f32x4 y = relu4(O::join(hi, lo), ldg4(P + OFF_B4 + 16 * rt + 4 * q));
        *reinterpret_cast<f32x4 *>(A4 + i * L128 + 16 * rt + 4 * q) = y;
    }
    __syncthreads();

    // ---------------- phase 6: W_ih x + b_ih + b_hh, gate-major (D rows = hidden units 16 wave + 4 q + r, columns = clips)
    {
        f32x4 hi[4], lo[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            hi[g] = ldg4(P + OFF_BG + g * 128 + wave * 16 + 4 * q);
            lo[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            typename O::Bv b;
            O::ldb(b, A4 + i * L128 + 32 * kc, q, amax);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typename O::W w;
                O::ldw(w, ih_w<Sch>(P, wave, g, kc), lane);
                O::mma(w, b, hi[g], lo[g]);
            }
        }
        // a workgroup that split anything outside the fp16 range hands the recurrent kernel NaN (ABI 7), and raises the sticky flag
        const bool poison = Sch::RANGE_CHECK && __syncthreads_or(!(amax <= H_MAX));
        if (!poison) {
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4 *>(dst + g * 256) = O::join(hi[g], lo[g]);
        } else {
            const float qnan = __builtin_nanf("");
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4 *>(dst + g * 256) = f32x4{qnan, qnan, qnan, qnan};
        }
    }
    if (Sch::RANGE_CHECK) range_flag_raise(P + OFF_HFLAG + 1, amax);
}

template <class Sch, typename S>
static int launch8k(const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride, long long origin, int batch,
                    int G, int steps, int Gws, int first_group, float *gx, void *stream) {
    VADX_DYN_LDS((silero8k_encode_kernel<Sch, S>), K8_LDS_BYTES);
    const long long nblk = (long long)G * steps;
    hipLaunchKernelGGL((silero8k_encode_kernel<Sch, S>), dim3((unsigned)nblk), dim3(K8_THREADS), K8_LDS_BYTES,
                       static_cast<hipStream_t>(stream), packed, src, in_scale, n_valid, row_stride, origin, batch, G, steps, Gws,
                       first_group, gx, RgArg<false>{});
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

// one workgroup per window of every run of the workgroup table (the caller has checked n_runs * RG_RUN < 2^31)
template <class Sch, typename S>
static int launch8k_ragged(const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx, void *stream, long long origin) {
    VADX_DYN_LDS((silero8k_encode_kernel<Sch, S, true>), K8_LDS_BYTES);
    hipLaunchKernelGGL((silero8k_encode_kernel<Sch, S, true>), dim3((unsigned)(rg.t.n_runs * RG_RUN)), dim3(K8_THREADS), K8_LDS_BYTES,
                       static_cast<hipStream_t>(stream), packed, src, in_scale, rg.n_src, 0LL, origin, rg.t.clips, rg.t.groups, 0, 0, 0, gx,
                       rg);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

template <typename S>
int silero8k_encode_ragged_launch(int arith, const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx,
                                  void *stream, long long origin) {
    if (arith == VADX_AR_H2) return launch8k_ragged<SchemeH2, S>(packed, src, in_scale, rg, gx, stream, origin);
    if (arith == VADX_AR_B3) return launch8k_ragged<SchemeB3, S>(packed, src, in_scale, rg, gx, stream, origin);
    return launch8k_ragged<SchemeF32, S>(packed, src, in_scale, rg, gx, stream, origin);
}
template int silero8k_encode_ragged_launch<float>(int, const float *, const float *, float, const RgArg<true> &, float *, void *, long long);
template int silero8k_encode_ragged_launch<int16_t>(int, const float *, const int16_t *, float, const RgArg<true> &, float *, void *, long long);

template <typename S>
int silero8k_encode_launch(int arith, const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                           long long origin, int batch, int G, int steps, int Gws, int first_group, float *gx, void *stream) {
    if (arith == VADX_AR_H2)
        return launch8k<SchemeH2, S>(packed, src, in_scale, n_valid, row_stride, origin, batch, G, steps, Gws, first_group, gx, stream);
    if (arith == VADX_AR_B3)
        return launch8k<SchemeB3, S>(packed, src, in_scale, n_valid, row_stride, origin, batch, G, steps, Gws, first_group, gx, stream);
    return launch8k<SchemeF32, S>(packed, src, in_scale, n_valid, row_stride, origin, batch, G, steps, Gws, first_group, gx, stream);
}
template int silero8k_encode_launch<float>(int, const float *, const float *, float, long long, long long, long long, int, int, int, int,
                                           int, float *, void *);
template int silero8k_encode_launch<int16_t>(int, const float *, const int16_t *, float, long long, long long, long long, int, int, int,
                                             int, int, float *, void *);

}  // namespace silero
}  // namespace vadx
