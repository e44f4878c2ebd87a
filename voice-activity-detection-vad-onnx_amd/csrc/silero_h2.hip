// silero_h2.hip -- Silero-VAD v5 (16 kHz) encoder + recurrent kernels on fp16 x 2 split products (csrc/split2.h), gfx950.
//
// Same inputs, same packed blob (its OFF_H* sections) and the same gx layout as silero_encode_split_kernel / silero_encode_kernel; what
// changes against the bf16 x 3 kernel (csrc/silero_split.hip):
//   * every product -- the folded STFT included -- is THREE v_mfma_f32_16x16x32_f16 per K = 32 step (h0 h0 -> hi; h0 h1', h1' h0 -> mid,
//     joined as hi + 2^-11 mid) instead of six bf16 MFMAs: 2 160 fp16 MFMAs per 16-window tile (STFT 480, conv1 960, conv2 240, conv3 48,
//     conv4 48, W_ih 384) against 1 024 f32 + 3 360 bf16; a weight is 4 bytes of fragments instead of 6, an activation two LDS planes
//     instead of three;
//   * the STFT's operands e = x[n] + x[256 - n], o = x[n] - x[256 - n] are formed ONCE per sample pair (thread = clip x four pairs x parity
//     class, all four frames), split, and parked as B planes for all four frames (64 KB, in place of the staged window); wave (bin tile,
//     frame pair) then runs both classes and both parts of its two frames, so nothing has to meet through LDS; bin 64 (its own mirror) is
//     row 0 of a fifth bin tile whose (class, part) pieces are dealt over the eight waves -- no VALU dot product;
//   * a workgroup encodes NSUB = 4 tiles (consecutive windows of one clip group) one after the other up to conv3 and runs conv4 and W_ih
//     ONCE for all of them: those two weight streams serve 64 columns instead of 16; a slot past the last window is
//     skipped outright (no recomputed tile);
//   * the kernels keep the running max |x| of everything they split; a workgroup that saw a value outside the fp16 range raises the
//     blob's sticky flag (OFF_HFLAG + 1) and the host recomputes the batch on the bf16 x 3 kernels (vadx_silero_range_flag).
// Reference being reproduced: the `session.run` of Silero/modeling_modified/utils_vad.py:116-119 (see silero.hip).
#include "silero_common.h"
#include "split2.h"

// Every phase re-derives its thread indices from a laundered copy of the thread id: nothing computed from them (LDS offsets, fragment
// pointers of LATER phases) can then be hoisted to the top of the tile loop, where it would sit in registers -- or in scratch -- through
// every phase in between.
#define H2_IDS()                                                                                           \
    int t_ = tid0;                                                                                         \
    asm volatile("" : "+v"(t_));                                                                           \
    const int tid = t_, lane = tid & 63, wave = tid >> 6, q = lane >> 4, i = lane & 15;                    \
    (void)tid; (void)lane; (void)wave; (void)q; (void)i
// (round 6, measured at config 2, built then removed: wave priority 1 (s_setprio) inside the GEMM loops -- 3.59 -> 3.85 ms, the waves in their
//  VALU phases are starved and reach the barriers later; the second tile's samples requested at the start of the first tile's conv2 phase
//  instead of in its own staging phase -- 3.59 -> 4.35 ms: the 24 registers do not exist beside conv2's, scratch 36 -> 148 B; a persistent grid
//  of 512 workgroups walking the tile pairs, the upper half started 0 / 24 000 / 48 000 / 72 000 shader cycles late so that a CU's two
//  workgroups run a fixed fraction of a tile period apart -- 3.55 -> 3.60 / 3.60 / 3.60 / 3.61 ms: no offset beats the dispatcher's own
//  staggering.)

namespace vadx {
namespace silero {

constexpr int H2_THREADS = 512;
constexpr int H2_WAVES_PER_SIMD = 4;
// how many steps ahead of the MFMAs the STFT's and conv1's fragment streams run (register sets = steps + 1)
constexpr int H2_AHS = 2, H2_AH1 = 2;
// ---- LDS map (BYTES): 81 920 B per workgroup => two workgroups per CU (eight waves of <= 128 VGPRs each)
//   R0 [0, 65536): X f32 [16 clips][642]
//                  -> STFT operand planes [E|O][e|o][2 planes][8 k-groups][4 frames x 16 clips][8 fp16]                (65 536 B)
//                  -> |X| planes [2][4 frames][16 k-groups][16 clips][8 fp16] at 0 (32 768 B) -> conv1 output planes (same shape, in place)
//                  -> after the last tile's conv3: conv4 output planes [tile][2][16][16][8] at 0 (4 x 8 KB)
//      from the STFT's last barrier of a tile on (the operand planes are dead): [32768, 65536) holds the f32 scratch (Nyquist magnitudes
//              [4 frames][16 clips], bin-64 partial sums [8 waves][2 frames][16 clips], the range verdicts), conv2's K-half exchange (8 KB),
//              conv3's (4 KB) and conv2's output planes [2 planes][2 frames][8 k-groups][16][8] (8 KB) at 53248.  The next tile's staged
//              window (41 088 B) overwrites none of conv3's inputs, so conv3's epilogue needs no barrier behind it.
//   R1 [65536, 81920): conv3 output planes of the workgroup's tiles [tile][2 planes][8 k-groups][16][8] -- the only region that lives
//              through the next tile's staging
constexpr int H2_EO_PL = 8192, H2_EO_KG = 1024;                 // one (class, e|o, plane) block; one k-group row of 64 columns
constexpr int H2_PL128 = 16384, H2_FR128 = 4096;
constexpr int H2_SCR = 32768;                                   // f32 scratch [512]: nyq at +0, bin-64 partials at +256 floats
constexpr int H2_EXC2 = 36864, H2_EXC3 = 45056;
constexpr int H2_C2 = 53248, H2_PL2 = 4096, H2_FR2 = 2048;
constexpr int H2_R1 = 65536, H2_T3 = 4096, H2_PL3 = 2048;
constexpr int H2_C4 = 0, H2_T4 = 8192, H2_PL4 = 4096;
// tiles a workgroup encodes one after the other before ONE joint conv4 / W_ih pass (R1 holds their conv3 planes)
constexpr int H2_NSUB = 4;
constexpr int H2_LDS_BYTES = H2_R1 + H2_NSUB * H2_T3;
static_assert(16 * X_LDM * 4 <= H2_EXC3 && H2_EXC3 + 4096 <= H2_C2 && H2_C2 + 2 * H2_PL2 <= H2_R1, "fp16 x 2 encoder LDS map: a tile");
static_assert(H2_C4 + H2_NSUB * H2_T4 <= H2_SCR && 2 * H2_LDS_BYTES <= 160 * 1024, "fp16 x 2 encoder LDS map: the tail");

__device__ __forceinline__ int hpl_off(int kg8, int clip) { return (kg8 * 16 + clip) * 16; }

// a producer lane's four consecutive channels 4 g .. 4 g + 3 of clip i: one 8-byte store into each of the two planes
__device__ __forceinline__ void store_h4(unsigned char *base, int plane_stride, int g, int i, const f32x4 v, float &amax) {
    u32x2 p0, p1;
    split2x4(v, p0, p1, amax);
    unsigned char *d = base + hpl_off(g >> 1, i) + (g & 1) * 8;
    *reinterpret_cast<u32x2 *>(d) = p0;
    *reinterpret_cast<u32x2 *>(d + plane_stride) = p1;
}
__device__ __forceinline__ void store_h1(unsigned char *base, int plane_stride, int slot, int i, float v, float &amax) {
    unsigned short h0, h1;
    split2x1(v, h0, h1, amax);
    unsigned char *d = base + hpl_off(slot >> 3, i) + (slot & 7) * 2;
    *reinterpret_cast<unsigned short *>(d) = h0;
    *reinterpret_cast<unsigned short *>(d + plane_stride) = h1;
}
// the wave's B fragments (two planes) of the 32-k chunk kc: lane 16 q + i reads k-group 4 kc + q of clip i
__device__ __forceinline__ void load_b2(f16x8 (&b)[2], const unsigned char *base, int plane_stride, int kc, int q, int i) {
    const unsigned char *s = base + hpl_off(4 * kc + q, i);
    b[0] = *reinterpret_cast<const f16x8 *>(s);
    b[1] = *reinterpret_cast<const f16x8 *>(s + plane_stride);
}
__device__ __forceinline__ void load_a2(f16x8 (&a)[2], const float *frag2, int lane) {
    a[0] = ldh(frag2, lane);
    a[1] = ldh(frag2 + HF, lane);
}

// RG (a ragged batch, silero_common.h): workgroup blk takes entry blk of the workgroup table -- (group, run of NSUB = RG_RUN consecutive
// windows) --, its valid slots are the windows the group still has, the sixteen clips are staged by stage_ragged and the group's gx tiles
// lie consecutively.  The range protocol is the rectangular one: the workgroup's verdict poisons its own tiles.
template <typename SampleT, int NSUB, bool RG = false>
__global__ __launch_bounds__(H2_THREADS, H2_WAVES_PER_SIMD) void silero_encode_h2_kernel(
    const float *__restrict__ P, const SampleT *__restrict__ audio, float in_scale, long long n_samples,
    long long row_stride, long long origin, int B, int G, int T, int Gws, int g0, float *__restrict__ gx, const RgArg<RG> rg) {
    static_assert(!RG || NSUB == RG_RUN, "the workgroup table has one entry per NSUB windows");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *X = reinterpret_cast<float *>(smem);
    float *scr = reinterpret_cast<float *>(smem + H2_SCR), *nyq = scr, *b64p = scr + 256;

    int tid0 = threadIdx.x;
    float amax = 0.f;                   // running max |x| of everything this thread splits
    if (ldg1(P + OFF_HFLAG) == 0.f) {   // uniform: this blob cannot run on fp16 x 2 (basis without the fold, a weight outside the range)
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(reinterpret_cast<unsigned *>(const_cast<float *>(P)) + OFF_HFLAG + 1, 2u);
        return;
    }
    const long long blk = blockIdx.x;
    // the workgroup's tiles: a workgroup's NSUB tiles are CONSECUTIVE WINDOWS of one clip group (window t = NSUB * (blk / G) + sub of
    // group blk % G): the next tile's samples are the next 2 KB of the same sixteen rows -- same pages, same DRAM rows as the loads the
    // previous tile has just made -- instead of sixteen rows 10 MB away (adjacent groups of one window, the round-5 order).  The valid
    // slots are a prefix of the NSUB; nvalid depends on blockIdx alone (workgroup-uniform), so a slot past the last window skips its whole
    // tile, barriers included, and the tail multiplies only the nvalid column tiles.
    int nvalid = (int)min((long long)NSUB, (long long)T - (blk / G) * NSUB);
    if constexpr (RG) {
        const int g_ = rg.t.wg_tab[2 * blk], r_ = rg.t.wg_tab[2 * blk + 1];
        nvalid = min(NSUB, rg.t.gx_first[g_ + 1] - rg.t.gx_first[g_] - r_ * NSUB);
    }
    {
    // Cross-phase fragment prefetch: the first sets of the STFT's weight stream are requested BEFORE the barrier that ends the staging phase
    // (global loads stay in flight across s_barrier, which only waits for lgkmcnt), so the L2 round trip that used to open the STFT runs
    // under the staging epilogue.  pre_s = those sets.
#pragma unroll 1
    for (int sub = 0; sub < nvalid; ++sub) {
    // per tile: nothing derived from the thread index is hoisted out of the tile loop (see silero_split.hip)
    int grp = (int)(blk % G), t = (int)(blk / G) * NSUB + sub;
    if constexpr (RG) {
        grp = rg.t.wg_tab[2 * blk];
        t = rg.t.wg_tab[2 * blk + 1] * NSUB + sub;
    }

    // ---------------- phase 0: the 16 windows (576 samples each) + right reflect pad of 64, even / odd samples in separate planes of the
    // clip row (as silero_encode_kernel stages them for the folded pass)
    auto xslot = [](int pp) { return (pp & 1) * X_ODD + (pp >> 1); };
    if constexpr (RG) {
        H2_IDS();
        (void)xslot;
        stage_ragged<SampleT, H2_THREADS>(X, true, audio, in_scale, rg, grp, (long long)t * 512 + origin, tid);
    } else {
        H2_IDS();
        const long long base = (long long)t * 512 + origin;
        const bool vec_ok = ((row_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(audio) & (SampleIO<SampleT>::VEC_ALIGN - 1)) == 0) && n_samples >= 4;
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const bool fast = vec_ok && base >= 0 && base + 576 <= n_samples && (long long)grp * 16 + 16 <= B;
        if (fast) {     // wave w stages clips 2w and 2w+1: wave-uniform row base + 16 * lane bytes, six loads back to back
            f32x4 xv[2][3];
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                const SampleT *src = audio + ((long long)grp * 16 + 2 * wv + k2) * row_stride + base;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int f = j < 2 ? lane + 64 * j : min(lane + 128, 143);
                    xv[k2][j] = SampleIO<SampleT>::load4(src + 4 * f, in_scale);
                }
            }
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                float *row = X + (2 * wv + k2) * X_LDM;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int f = lane + 64 * j;
                    if (j < 2 || lane < 16) {
                        const f32x4 v = xv[k2][j];
                        *reinterpret_cast<float2 *>(row + 2 * f) = float2{v[0], v[2]};
                        *reinterpret_cast<float2 *>(row + X_ODD + 2 * f) = float2{v[1], v[3]};
                    }
                }
                // right reflect pad (0, 64): padded sample 1150 - p = sample p for p = 511 .. 574.  p = 512 + 4 lane + jj sits in the third load of
                // lanes 0 .. 15 (slot parity = parity of jj, plane index 319 - 2 lane - ...), p = 511 in the second load of lane 63 -- spelled out:
                // the generic per-element test cost ~40 VALU instructions per clip for sixteen lanes' worth of stores
                if (lane < 16) {
                    const f32x4 v = xv[k2][2];
                    row[319 - 2 * lane] = v[0];
                    row[X_ODD + 318 - 2 * lane] = v[1];
                    row[318 - 2 * lane] = v[2];
                    if (lane < 15) row[X_ODD + 317 - 2 * lane] = v[3];
                }
                if (lane == 63) row[X_ODD + 319] = xv[k2][1][3];
            }
        } else {        // edge windows, short clips, groups past the batch: clamped unconditional loads, patched per element
            f32x4 x4[5];
            if (vec_ok) {
#pragma unroll
                for (int it = 0; it < 5; ++it) {
                    const int e = min(tid + H2_THREADS * it, 16 * 144 - 1), c = e / 144, p = 4 * (e - c * 144);
                    const long long b = (long long)grp * 16 + c, idx = base + p;
                    const SampleT *src = audio + (b < B ? b : 0) * row_stride;
                    const long long idc = idx < 0 ? 0 : (idx + 3 < n_samples ? idx : ((n_samples - 4) & ~3LL));
                    x4[it] = SampleIO<SampleT>::load4(src + idc, in_scale);
                }
            }
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                const int e = tid + H2_THREADS * it;             // 16 clips x 144 float4
                if (e < 16 * 144) {
                    const int c = e / 144, p = 4 * (e - c * 144);
                    const long long b = (long long)grp * 16 + c;
                    const bool bvalid = b < B;
                    const SampleT *src = audio + (bvalid ? b : 0) * row_stride;
                    const long long idx = base + p;
                    float v[4];
                    if (vec_ok && bvalid && idx >= 0 && idx + 3 < n_samples) {
                        v[0] = x4[it][0]; v[1] = x4[it][1]; v[2] = x4[it][2]; v[3] = x4[it][3];
                    } else {
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
                            v[jj] = (bvalid && idx + jj >= 0 && idx + jj < n_samples) ? SampleIO<SampleT>::load1(src + idx + jj, in_scale) : 0.f;
                    }
                    float *row = X + c * X_LDM;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const int pp = p + jj;
                        row[xslot(pp)] = v[jj];
                        if (pp >= 511 && pp <= 574) row[xslot(1150 - pp)] = v[jj];       // reflect pad (0,64)
                    }
                }
            }
        }
    }
    f16x8 pre_s[H2_AHS][2];           // the STFT's first sets: in flight while the samples go to registers and the operand planes are built
    {
        H2_IDS();
        const float *wq = P + OFF_HSF + (size_t)(wave & 3) * (2 * 2 * 2 * 2 * HF);
#pragma unroll
        for (int s0_ = 0; s0_ < H2_AHS; ++s0_) load_a2(pre_s[s0_], wq + s0_ * 2 * HF, lane);
    }
    __syncthreads();

    // ---------------- phase 1: the folded STFT on split products -> magnitudes -> the two fp16 planes of conv1's input.
    // Per frame f (samples 128 f .. 128 f + 255 of the padded window) and pair index n = 1..128: e = x[n] + x[256 - n] (cos part),
    // o = the difference (sin part), in two classes (E: n = 2 m + 2, O: n = 2 m + 1: the frequency fold); bins k <= 63 of tile tl:
    //   X[k] = E + O, X[128 - k] = +-(E - O), with E / O = the class's partial sums (silero_common.h: stft_fold_class).
    // Input-channel slot s of conv1: s <= 64 = bin s, s = 64 + k = bin 128 - k; bin 128 (Nyquist) goes to the scratch.
    {
        H2_IDS();
        const int tl = wave & 3, fp = wave >> 2;                  // GEMM role: bins 16 tl + 4 q + r (and 128 - them), frames 2 fp, 2 fp + 1, clip i
        f32x4 mk[2], mn[2];
        float b64[2];
        {
            // ---- operand role: thread (clip pc, four consecutive pairs 4 pj .. 4 pj + 3 of class cls) reads its 32 samples out of X
            const int cls = wave >> 2, pc = tid & 15, pj = (tid >> 4) & 15;
            float xa[4][4], xb[4][4];                             // [frame][k]: the pair's two samples
            {
                const float *row = X + pc * X_LDM + (cls ? X_ODD : 1) + 4 * pj, *rowb = X + pc * X_LDM + (cls ? X_ODD : 0) + 127 - 4 * pj;
#pragma unroll
                for (int f = 0; f < 4; ++f)
#pragma unroll
                    for (int k = 0; k < 4; ++k) { xa[f][k] = row[64 * f + k]; xb[f][k] = rowb[64 * f - k]; }
            }
            float x0p[2];                                         // the n = 0 sample of the GEMM role's two frames (even class)
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) x0p[fr] = X[i * X_LDM + 64 * (2 * fp + fr)];
            // bin 64's piece of this wave: (class bc, part bp) of the fifth tile for the wave's two frames; the n = 0 tap rides in the
            // even class's accumulator (row 0 = lanes q = 0, element 0)
            const int bc = (wave >> 1) & 1, bp = wave & 1;
            __syncthreads();          // every sample is in registers: the operand planes may overwrite X
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                f32x4 ev, ov;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // (plain v_add_f32 / v_sub_f32, spelled out: left to the compiler the pair sums become v_pk_add_f32 with a CROSS op_sel swizzle
                    //  -- xb is read in descending order -- and that form returned wrong sums in roughly every second tile once two workgroups
                    //  (four waves per SIMD) shared a CU, while the same binary was bit-exact at one workgroup per CU: profiles/r06_pk_hazard.txt,
                    //  DESIGN.md section 4e)
                    float e_, o_;
                    asm volatile("v_add_f32 %0, %1, %2" : "=v"(e_) : "v"(xa[f][k]), "v"(xb[f][k]));
                    asm volatile("v_sub_f32 %0, %1, %2" : "=v"(o_) : "v"(xa[f][k]), "v"(xb[f][k]));
                    ev[k] = e_;
                    ov[k] = o_;
                }
                unsigned char *d = smem + (cls * 4) * H2_EO_PL + (pj >> 1) * H2_EO_KG + (16 * f + pc) * 16 + 8 * (pj & 1);
                u32x2 p0, p1;
                split2x4(ev, p0, p1, amax);
                *reinterpret_cast<u32x2 *>(d) = p0;
                *reinterpret_cast<u32x2 *>(d + H2_EO_PL) = p1;
                split2x4(ov, p0, p1, amax);
                *reinterpret_cast<u32x2 *>(d + 2 * H2_EO_PL) = p0;
                *reinterpret_cast<u32x2 *>(d + 3 * H2_EO_PL) = p1;
            }
            __syncthreads();
            // ---- the wave's GEMM: (class, part) = (E re, E im, O re, O im) x two chunks x its two frames
            const f32x4 c0 = ldg4(P + OFF_S0 + tl * 16 + 4 * q), s0 = ldg4(P + OFF_S0 + 64 + tl * 16 + 4 * q);
            const float b64n0 = bc ? 0.f : ldg1(P + OFF_B64 + 256 + bp);
            f32x4 hi[4][2], mid[4][2];
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                hi[0][fr] = c0 * x0p[fr];
                hi[1][fr] = s0 * x0p[fr];
                hi[2][fr] = f32x4{0.f, 0.f, 0.f, 0.f};
                hi[3][fr] = hi[2][fr];
#pragma unroll
                for (int a4 = 0; a4 < 4; ++a4) mid[a4][fr] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float *wb = P + OFF_HSF + (size_t)((4 * 2 + bc) * 2 + bp) * (2 * 2 * HF);
            {
                const float *wq = P + OFF_HSF + (size_t)tl * (2 * 2 * 2 * 2 * HF);
                constexpr int AH = H2_AHS;
                f16x8 a[AH + 1][2];
#pragma unroll
                for (int s0_ = 0; s0_ < AH; ++s0_) { a[s0_][0] = pre_s[s0_][0]; a[s0_][1] = pre_s[s0_][1]; }
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) {          // s8 = (class, part, chunk) in OFF_HSF's order
                    if (s8 + AH < 8) load_a2(a[(s8 + AH) % (AH + 1)], wq + (s8 + AH) * 2 * HF, lane);
                    f16x8 b[2][2];
#pragma unroll
                    for (int fr = 0; fr < 2; ++fr) {
                        const unsigned char *bs = smem + ((s8 >> 1) * 2) * H2_EO_PL + (4 * (s8 & 1) + q) * H2_EO_KG + (16 * (2 * fp + fr) + i) * 16;
                        b[fr][0] = *reinterpret_cast<const f16x8 *>(bs);
                        b[fr][1] = *reinterpret_cast<const f16x8 *>(bs + H2_EO_PL);
                    }
                    const f16x8 (&ac)[2] = a[s8 % (AH + 1)];      // the two frames alternate so that consecutive MFMAs hit different accumulators
#pragma unroll
                    for (int fr = 0; fr < 2; ++fr) mid[s8 >> 1][fr] = mfma_f16(ac[1], b[fr][0], mid[s8 >> 1][fr]);
#pragma unroll
                    for (int fr = 0; fr < 2; ++fr) mid[s8 >> 1][fr] = mfma_f16(ac[0], b[fr][1], mid[s8 >> 1][fr]);
#pragma unroll
                    for (int fr = 0; fr < 2; ++fr) hi[s8 >> 1][fr] = mfma_f16(ac[0], b[fr][0], hi[s8 >> 1][fr]);
                }
            }
            f16x8 ab[2][2];                               // the bin-64 piece's two chunks: requested before the magnitudes, used after them
            load_a2(ab[0], wb, lane);
            load_a2(ab[1], wb + 2 * HF, lane);
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                const f32x4 ere = join2(hi[0][fr], mid[0][fr]), eim = join2(hi[1][fr], mid[1][fr]);
                const f32x4 ore = join2(hi[2][fr], mid[2][fr]), oim = join2(hi[3][fr], mid[3][fr]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pre = ere[r] + ore[r], pim = eim[r] + oim[r], nre = ere[r] - ore[r], nim = eim[r] - oim[r];
                    mk[fr][r] = mag_sqrt(pre * pre + pim * pim);
                    mn[fr][r] = mag_sqrt(nre * nre + nim * nim);
                }
            }
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                f32x4 bhi = {b64n0 * x0p[fr], 0.f, 0.f, 0.f}, bmid = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    f16x8 b[2];
                    const unsigned char *bs = smem + ((bc * 2 + bp) * 2) * H2_EO_PL + (4 * ch + q) * H2_EO_KG + (16 * (2 * fp + fr) + i) * 16;
                    b[0] = *reinterpret_cast<const f16x8 *>(bs);
                    b[1] = *reinterpret_cast<const f16x8 *>(bs + H2_EO_PL);
                    mfma_split3(ab[ch], b, bhi, bmid);
                }
                b64[fr] = fmaf(bmid[0], H1_INV, bhi[0]);
            }
        }
        __syncthreads();          // every wave is done reading the operand planes: the |X| planes may overwrite them
        {
            H2_IDS();             // (fresh indices: the store offsets below must not be computed -- and parked -- in front of the GEMM)
            const int g = 4 * (wave & 3) + q;
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                const int f = 2 * (wave >> 2) + fr;
                unsigned char *frp = smem + f * H2_FR128;
                store_h4(frp, H2_PL128, g, i, mk[fr], amax);                  // slots 4 g + r        = bins 4 g + r
                store_h4(frp, H2_PL128, 16 + g, i, mn[fr], amax);             // slots 64 + 4 g + r   = bins 128 - (4 g + r); g = 0, r = 0 is bin 128:
                if (g == 0) nyq[f * 16 + i] = mn[fr][0];                      //   it goes to the scratch, and slot 64 is rewritten below with bin 64
                if (q == 0) b64p[(wave * 2 + fr) * 16 + i] = b64[fr];
            }
        }
        __syncthreads();
        if (tid < 64) {                                                       // bin 64: frame tid / 16, clip tid % 16
            const int f = tid >> 4, c = tid & 15;
            const float *pp = b64p + ((f >> 1) * 8 + (f & 1)) * 16 + c;       // waves 4 (f >> 1) + (class, part), part fastest
            const float re = pp[0] + pp[2 * 2 * 16], im = pp[1 * 2 * 16] + pp[3 * 2 * 16];
            store_h1(smem + f * H2_FR128, H2_PL128, 64, c, mag_sqrt(re * re + im * im), amax);
        }
    }
    __syncthreads();

    // ---------------- phase 2: conv1 129->128, k3 s1 p1, ReLU -- direct: out[f] = sum_tap W[tap] in[f + tap - 1], wave = 16 output channels
    {
        H2_IDS();
        const int rt = wave;
        f32x4 hi[4], mid[4];
        {   // bias + input channel 128 (the Nyquist bin) on the VALU
            const f32x4 bias = ldg4(P + OFF_B1 + 16 * rt + 4 * q);
            f32x4 wn[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wn[r] = ldg4(P + OFF_Q1N + (16 * rt + 4 * q + r) * 4);
            float nq[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) nq[f] = nyq[f * 16 + i];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = fmaf(wn[r][1], nq[f], bias[r]);
                    if (f > 0) v = fmaf(wn[r][0], nq[f - 1], v);
                    if (f < 3) v = fmaf(wn[r][2], nq[f + 1], v);
                    hi[f][r] = v;
                }
                mid[f] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const float *wq = P + OFF_H1 + rt * (4 * 3 * 2 * HF);
        constexpr int AH = H2_AH1;
        f16x8 a[AH + 1][2];
#pragma unroll
        for (int s0_ = 0; s0_ < AH; ++s0_) load_a2(a[s0_], wq + s0_ * 2 * HF, lane);
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            f16x8 b[4][2];
#pragma unroll
            for (int f = 0; f < 4; ++f) load_b2(b[f], smem + f * H2_FR128, H2_PL128, kc, q, i);
#pragma unroll
            for (int tap = 0; tap < 3; ++tap) {
                const int s = kc * 3 + tap;
                if (s + AH < 12) load_a2(a[(s + AH) % (AH + 1)], wq + (s + AH) * 2 * HF, lane);
                const f16x8 (&ac)[2] = a[s % (AH + 1)];
                // three products per (frame, tap), frames innermost so that consecutive MFMAs hit different accumulators
#define H2_TERM(AP, BP, ACC)                                                                  \
    _Pragma("unroll") for (int f = 0; f < 4; ++f) {                                           \
        const int fi = f + tap - 1;                                                           \
        if (fi >= 0 && fi < 4) ACC[f] = mfma_f16(ac[AP], b[fi][BP], ACC[f]);                  \
    }
                H2_TERM(1, 0, mid) H2_TERM(0, 1, mid) H2_TERM(0, 0, hi)
#undef H2_TERM
            }
        }
        __syncthreads();          // every wave is done reading the |X| planes: conv1's output may now overwrite them
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const f32x4 s = join2(hi[f], mid[f]);
            f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = fmaxf(s[r], 0.f);
            store_h4(smem + f * H2_FR128, H2_PL128, 4 * rt + q, i, y, amax);
        }
    }
    __syncthreads();

    // ---------------- phase 3: conv2 128->64, k3 s2 p1, ReLU: out frame o reads in frames 2 o - 1 .. 2 o + 1; wave = (16 channels, half of K)
    {
        H2_IDS();
        const int rt = wave & 3, kh = wave >> 2;
        f32x4 hi[2], mid[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) { hi[o] = f32x4{0.f, 0.f, 0.f, 0.f}; mid[o] = hi[o]; }
        const float *wq = P + OFF_H2 + (rt * 4 + 2 * kh) * (3 * 2 * HF);
        constexpr int RING = 3;      // two steps ahead on three register sets
        f16x8 a[RING][2];
#pragma unroll
        for (int s = 0; s < 2; ++s) load_a2(a[s], wq + s * 2 * HF, lane);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 b[4][2];
#pragma unroll
            for (int f = 0; f < 4; ++f) load_b2(b[f], smem + f * H2_FR128, H2_PL128, 2 * kh + kk, q, i);
#pragma unroll
            for (int tap = 0; tap < 3; ++tap) {
                const int s = kk * 3 + tap;
                if (s + 2 < 6) load_a2(a[(s + 2) % RING], wq + (s + 2) * 2 * HF, lane);
                const f16x8 (&ac)[2] = a[s % RING];
#define H2_TERM(AP, BP, ACC)                                                                  \
    _Pragma("unroll") for (int o = 0; o < 2; ++o) {                                           \
        const int fi = 2 * o + tap - 1;                                                       \
        if (fi >= 0) ACC[o] = mfma_f16(ac[AP], b[fi][BP], ACC[o]);                            \
    }
                H2_TERM(1, 0, mid) H2_TERM(0, 1, mid) H2_TERM(0, 0, hi)
#undef H2_TERM
            }
        }
        f32x4 s2[2] = {join2(hi[0], mid[0]), join2(hi[1], mid[1])};
        float *exc = reinterpret_cast<float *>(smem + H2_EXC2);
        if (kh == 1) {
#pragma unroll
            for (int o = 0; o < 2; ++o) *reinterpret_cast<f32x4 *>(exc + ((rt * 2 + o) * 64 + lane) * 4) = s2[o];
        }
        __syncthreads();
        if (kh == 0) {
            const f32x4 bias = ldg4(P + OFF_B2 + 16 * rt + 4 * q);
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const f32x4 other = *reinterpret_cast<const f32x4 *>(exc + ((rt * 2 + o) * 64 + lane) * 4);
                f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(s2[o][r] + other[r] + bias[r], 0.f);
                store_h4(smem + H2_C2 + o * H2_FR2, H2_PL2, 4 * rt + q, i, y, amax);
            }
        }
    }
    f16x8 pre_3[2][2];                  // conv3's two sets: in flight across the barrier
    {
        H2_IDS();
        const float *w3 = P + OFF_H3 + ((wave & 3) * 2 + (wave >> 2)) * (2 * 2 * HF);
        load_a2(pre_3[0], w3, lane);
        load_a2(pre_3[1], w3 + 2 * HF, lane);
    }
    __syncthreads();

    // ---------------- phase 4: conv3 64->64, k3 s2 p1, ReLU (one output frame; tap 0 reads padding): wave = (16 channels, tap 1 | 2).  Its
    // output goes to the tile's slot of R1; the next tile's staging touches none of conv3's inputs (see the LDS map), so no barrier follows
    {
        H2_IDS();
        const int rt = wave & 3, th = wave >> 2;      // tap th + 1 reads conv2's frame th
        f32x4 hi = {0.f, 0.f, 0.f, 0.f}, mid = hi;
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            f16x8 b[2];
            load_b2(b, smem + H2_C2 + th * H2_FR2, H2_PL2, kc, q, i);
            mfma_split3(pre_3[kc], b, hi, mid);
        }
        float *exc = reinterpret_cast<float *>(smem + H2_EXC3);
        if (th == 1) *reinterpret_cast<f32x4 *>(exc + (rt * 64 + lane) * 4) = join2(hi, mid);
        __syncthreads();
        if (th == 0) {
            const f32x4 bias = ldg4(P + OFF_B3 + 16 * rt + 4 * q);
            const f32x4 s3 = join2(hi, mid), other = *reinterpret_cast<const f32x4 *>(exc + (rt * 64 + lane) * 4);
            f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = fmaxf(s3[r] + other[r] + bias[r], 0.f);
            store_h4(smem + H2_R1 + sub * H2_T3, H2_PL3, 4 * rt + q, i, y, amax);
        }
    }
    }      // sub

    // W_ih step j (0 .. 15) multiplies fragment pair s = 4 kc + g: gate half gh = j / 8 (gates 2 gh, 2 gh + 1), kc = (j / 2) % 4, g = 2 gh + j % 2
    auto ih_s = [](int j) { return 4 * ((j >> 1) & 3) + 2 * (j >> 3) + (j & 1); };
    __syncthreads();         // every tile's conv3 planes are in R1; R0 is free
    // ---------------- phase 5: conv4 64->128, k3 s1 p1, ReLU (one frame in / out: centre tap only), the nvalid tiles at once: R1 -> R0
    {
        H2_IDS();
        const int rt = wave;
        const f32x4 bias = ldg4(P + OFF_B4 + 16 * rt + 4 * q);
        f32x4 hi[NSUB], mid[NSUB];
#pragma unroll
        for (int sb = 0; sb < NSUB; ++sb) { hi[sb] = bias; mid[sb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const float *w4 = P + OFF_H4 + wave * (2 * 2 * HF);
        f16x8 a[2][2];
        load_a2(a[0], w4, lane);
        load_a2(a[1], w4 + 2 * HF, lane);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc)
#pragma unroll
            for (int sb = 0; sb < NSUB; ++sb) {
                if (sb < nvalid) {
                    f16x8 b[2];
                    load_b2(b, smem + H2_R1 + sb * H2_T3, H2_PL3, kc, q, i);
                    mfma_split3(a[kc], b, hi[sb], mid[sb]);
                }
            }
#pragma unroll
        for (int sb = 0; sb < NSUB; ++sb) {
            if (sb < nvalid) {
                const f32x4 s = join2(hi[sb], mid[sb]);
                f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = fmaxf(s[r], 0.f);
                store_h4(smem + H2_C4 + sb * H2_T4, H2_PL4, 4 * rt + q, i, y, amax);
            }
        }
        // nothing is split after this point: the workgroup's verdict on the fp16 range (one word per wave, read behind the barrier below)
        const bool bad = !(amax <= H_MAX);
        if (__ballot(bad) != 0ULL && lane == 0) reinterpret_cast<unsigned *>(scr)[128 + wave] = 1u;
        else if (lane == 0) reinterpret_cast<unsigned *>(scr)[128 + wave] = 0u;
    }
    __syncthreads();

    // ---------------- phase 6: LSTM input projection for the workgroup's tiles at once (D rows = hidden units 16 wave + 4 q + r, columns =
    // clips), in two gate halves {0, 1}, {2, 3} so that the accumulators of four column tiles fit: every W_ih fragment pair is loaded once
    // and multiplies the nvalid column tiles (the B planes are read once per half)
    {
        H2_IDS();
        // a workgroup that split anything outside the fp16 range hands the recurrent kernel NaN, not numbers that look like gate
        // pre-activations: a caller that never reads vadx_silero_range_flag gets NaN scores for these clips, not plausible ones
        const unsigned *bw = reinterpret_cast<const unsigned *>(scr) + 128;
        const bool poison = __builtin_amdgcn_readfirstlane((int)(bw[0] | bw[1] | bw[2] | bw[3] | bw[4] | bw[5] | bw[6] | bw[7])) != 0;
        const float *wq = P + OFF_HIH + wave * (4 * 4 * 2 * HF);
        // the fragment ring holds two k-chunks (the current one's two gates and the next one's, requested when the current one starts)
        f16x8 a[2][2][2];
#pragma unroll
        for (int gg = 0; gg < 2; ++gg) load_a2(a[0][gg], wq + ih_s(gg) * 2 * HF, lane);
#pragma unroll
        for (int gh = 0; gh < 2; ++gh) {
            f32x4 hi[NSUB][2], mid[NSUB][2];
#pragma unroll
            for (int gg = 0; gg < 2; ++gg) {
                const f32x4 bg = ldg4(P + OFF_BG + (2 * gh + gg) * 128 + wave * 16 + 4 * q);
#pragma unroll
                for (int sb = 0; sb < NSUB; ++sb) { hi[sb][gg] = bg; mid[sb][gg] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                const int j = 8 * gh + 2 * kc;            // the step of (kc, gate 2 gh)
#pragma unroll
                for (int gg = 0; gg < 2; ++gg)
                    if (j + 2 < 16) load_a2(a[((j >> 1) + 1) & 1][gg], wq + ih_s(j + 2 + gg) * 2 * HF, lane);
                const f16x8 (&ac)[2][2] = a[(j >> 1) & 1];
                // column tile outermost: one tile's B pair is live at a time (a single accumulation chain costs the 16x16x32 MFMA nothing)
#pragma unroll
                for (int sb = 0; sb < NSUB; ++sb) {
                    if (sb < nvalid) {
                        f16x8 b[2];
                        load_b2(b, smem + H2_C4 + sb * H2_T4, H2_PL4, kc, q, i);
#pragma unroll
                        for (int gg = 0; gg < 2; ++gg)
                            mfma_split3(ac[gg], b, hi[sb][gg], mid[sb][gg]);
                    }
                }
            }
#pragma unroll
            for (int sb = 0; sb < NSUB; ++sb) {
                if (sb >= nvalid) continue;
                const int t_s = (int)(blk / G) * NSUB + sb, grp_s = (int)(blk % G);
                size_t tile = (size_t)t_s * Gws + g0 + grp_s;
                if constexpr (RG) tile = (size_t)rg.t.gx_first[rg.t.wg_tab[2 * blk]] + rg.t.wg_tab[2 * blk + 1] * NSUB + sb;
                float *dst = gx + tile * GX_TILE_FLOATS + (size_t)wave * 4 * 256 + lane * 4;
                if (!poison) {           // (workgroup-uniform: a branch, not 32 selects)
#pragma unroll
                    for (int gg = 0; gg < 2; ++gg) *reinterpret_cast<f32x4 *>(dst + (2 * gh + gg) * 256) = join2(hi[sb][gg], mid[sb][gg]);
                } else {
                    const float qnan = __builtin_nanf("");
#pragma unroll
                    for (int gg = 0; gg < 2; ++gg) *reinterpret_cast<f32x4 *>(dst + (2 * gh + gg) * 256) = f32x4{qnan, qnan, qnan, qnan};
                }
            }
        }
    }
    }      // blk
    // ---- range check: anything split above the largest finite fp16 raises the blob's sticky flag.  (A NaN sample does not: v_max3_f32
    // returns its non-NaN operands, so NaN never reaches amax -- it travels through the products instead.)
    if (!(amax <= H_MAX)) {
        unsigned *fl = reinterpret_cast<unsigned *>(const_cast<float *>(P)) + OFF_HFLAG + 1;
        atomicOr(fl, 1u);
        atomicMax(fl + 1, __float_as_uint(amax));
    }
}

// ---- persistent LSTM on fp16 x 2 products ------------------------------------------------------
// Same decomposition as silero_lstm_split_kernel: one persistent workgroup per 16 clips, wave w owns hidden units 16 w .. 16 w + 15 of all
// four gates, h exchanged through double-buffered LDS planes, one barrier per step.  Both planes of W_hh stay in VGPRs for the whole
// clip (128 registers: no weight bytes in LDS at all); 48 v_mfma_f32_16x16x32_f16 per wave and step instead of 96 bf16.  |h| <= 1 and W_hh
// passed the pack-time range check, so nothing here can leave the fp16 range.
constexpr int LH_HPL = 4096, LH_HBUF = 8192;     // h planes [2 buffers][2 planes][16 k-groups][16 clips][8 fp16]
// The decoder's per-wave partial sums wait in an LDS ring and the scores leave in blocks of LH_BLK steps: after the barrier of a block's last
// step (and of the clip's last step) 256 lanes -- 16 clips x 16 steps -- add db + part[0] + ... + part[7] in that order, take the sigmoid and store
// 64 contiguous bytes per clip.  (Per step, wave 0 alone used to read the eight partials and issue sixteen scattered 4-byte stores behind every
// barrier, and the other seven waves met it late at the next one.)  Two blocks: the waves that do not flush run ahead into the next block's
// slots while the other one is read; a block is written again only after a later barrier, which the flushing waves pass after their reads.
constexpr int LH_BLK = 16;
constexpr int LH_SLOT = 8 * 16 + 4;              // floats per step [8 waves][16 clips], +4: the flush's reads (lane = 16 clip + step) hit 64 banks
constexpr int LH_PART = 2 * LH_HBUF;             // f32 [2 blocks][LH_BLK steps][LH_SLOT]
constexpr int LH_BYTES = LH_PART + 2 * LH_BLK * LH_SLOT * 4;
// gx (the encoder's gate pre-activations, 32 KB per step and workgroup out of HBM: 2.6 GB per launch at config 2 = 4.3 TB/s) is requested
// LH_GX_AHEAD steps ahead: with one step of lead a lone workgroup ran 1.42 us per step and the full grid 1.95 -- the loaded HBM's
// latency exceeds a step.
constexpr int LH_GX_AHEAD = 3;

// RG (a ragged batch): as silero_lstm_kernel's ragged instantiation (csrc/silero.hip) -- T_g steps over the group's consecutive gx tiles,
// column n = the clip of slot 16 grp + n, frozen behind its own last window; a flush block stores a clip's scores for t < T_b only, into
// its own row, and the NaN of a poisoned group stays inside its clips' rows.
template <bool RG = false>
__global__ __launch_bounds__(512, 2) void silero_lstm_h2_kernel(
    const float *__restrict__ P, const float *__restrict__ gx, const float *__restrict__ state0,
    int B, int G, int T, float *__restrict__ probs, long long probs_stride, float *__restrict__ state_n, const RgArg<RG> rg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *part = reinterpret_cast<float *>(smem + LH_PART);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, n = lane & 15;
    const int grp = blockIdx.x;
    long long b = (long long)grp * 16 + n;
    bool bvalid = b < B;
    int Tb = T;                                   // RG: the column's own window count
    float *prow = nullptr;                        // RG: the clip's row of the packed scores
    size_t gx0 = (size_t)grp, gstep_tiles = (size_t)G;
    if constexpr (RG) {
        const int clip = rg_clip(rg, grp * 16 + n);
        long long o_;
        int l_;
        const bool refused = !rg_slot(rg, grp * 16 + n, o_, l_);
        T = rg.t.gx_first[grp + 1] - rg.t.gx_first[grp];
        gx0 = (size_t)rg.t.gx_first[grp];
        gstep_tiles = 1;
        bvalid = clip >= 0;
        b = bvalid ? clip : 0;
        Tb = bvalid ? min((int)(rg.t.probs_first[b + 1] - rg.t.probs_first[b]), T) : 0;
        prow = probs + rg.t.probs_first[b];
        if (refused && wave == 0 && q == 0) atomicOr(rg.t.status, 1u);
    }
    const int u0 = wave * 16 + 4 * q;             // this lane's 4 hidden units
    if (ldg1(P + OFF_HFLAG) == 0.f) {   // uniform: this blob cannot run on fp16 x 2 (a weight outside the fp16 range): as the encoder, flag bit 1,
        if (tid == 0 && grp == 0) atomicOr(reinterpret_cast<unsigned *>(const_cast<float *>(P)) + OFF_HFLAG + 1, 2u);      // and no plausible score
        if (wave == 0 && lane < 16 && bvalid) {
            if constexpr (RG) for (int t = 0; t < Tb; ++t) prow[t] = __builtin_nanf("");
            else for (int t = 0; t < T; ++t) probs[b * probs_stride + t] = __builtin_nanf("");
        }
        return;
    }

    f16x8 a[4][4][2];
    {
        const float *wq = P + OFF_HHH + (size_t)wave * (4 * 4 * 2 * HF);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) load_a2(a[g][kc], wq + (g * 4 + kc) * 2 * HF, lane);
    }
    // the decoder's ReLU as (h + |h|) / 2 with the 1/2 folded into its weights: the same value bit for bit (both scalings are exact), but a NaN
    // state stays NaN in the score -- fmaxf(h, 0) would turn it into 0 and a poisoned clip (see the encoder's gx) into a plausible number
    const f32x4 dwh = ldg4(P + OFF_DW + u0) * 0.5f;
    const float db = P[OFF_DB];

    float amax = 0.f;
    f32x4 c = {0.f, 0.f, 0.f, 0.f}, h = {0.f, 0.f, 0.f, 0.f};
    if (state0 != nullptr && bvalid) {
        h = *reinterpret_cast<const f32x4 *>(state0 + b * 128 + u0);
        c = *reinterpret_cast<const f32x4 *>(state0 + ((long long)B + b) * 128 + u0);
    }
    store_h4(smem, LH_HPL, 4 * wave + q, n, h, amax);
    __syncthreads();

    const float *gsrc = gx + gx0 * GX_TILE_FLOATS + (size_t)wave * 4 * 256 + lane * 4;
    const size_t gstep = gstep_tiles * GX_TILE_FLOATS;
    // the gx ring (LH_GX_AHEAD steps) is indexed statically: the step loop is unrolled by its depth
// (round 6, measured, removed: gate-major MFMA order -- a gate's twelve products finish before the next gate's start, so that its non-linearity
//  runs under the next gate's MFMAs, all four B fragment pairs held in registers -- 0.590 -> 0.597 ms with gx two steps ahead, 0.65 with three
//  (44 B of scratch): the compiler interleaves v_exp / v_rcp with the MFMAs as intended, the step is no shorter.)
    constexpr int GA = LH_GX_AHEAD;
    f32x4 gq[GA][4];
#pragma unroll
    for (int j = 0; j < GA; ++j) {
        const int tj = j < T ? j : T - 1;
#pragma unroll
        for (int g = 0; g < 4; ++g) gq[j][g] = *reinterpret_cast<const f32x4 *>(gsrc + tj * gstep + g * 256);
    }

    int cur = 0;
    for (int t0 = 0; t0 < T; t0 += GA) {
#pragma unroll
    for (int j = 0; j < GA; ++j) {
        const int t = t0 + j;
        if (t >= T) break;
        f32x4 hi[4], mid[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) { hi[g] = gq[j][g]; mid[g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        {
            const int tn = (t + GA < T) ? t + GA : T - 1;
#pragma unroll
            for (int g = 0; g < 4; ++g) gq[j][g] = *reinterpret_cast<const f32x4 *>(gsrc + tn * gstep + g * 256);
        }
        const unsigned char *hb = smem + cur * LH_HBUF;
        float dpart = 0.f;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            f16x8 bb[2];
            load_b2(bb, hb, LH_HPL, kc, q, n);
            // the three products, gates innermost so that consecutive MFMAs hit different accumulators
#pragma unroll
            for (int g = 0; g < 4; ++g) mid[g] = mfma_f16(a[g][kc][1], bb[0], mid[g]);
#pragma unroll
            for (int g = 0; g < 4; ++g) mid[g] = mfma_f16(a[g][kc][0], bb[1], mid[g]);
#pragma unroll
            for (int g = 0; g < 4; ++g) hi[g] = mfma_f16(a[g][kc][0], bb[0], hi[g]);
        }
        const f32x4 h_in = h, c_in = c;           // (RG) what a column behind its last window keeps
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = gate_sigmoid(fmaf(mid[0][r], H1_INV, hi[0][r])), fg = gate_sigmoid(fmaf(mid[1][r], H1_INV, hi[1][r]));
            const float gg = gate_tanh(fmaf(mid[2][r], H1_INV, hi[2][r])), og = gate_sigmoid(fmaf(mid[3][r], H1_INV, hi[3][r]));
            c[r] = fg * c[r] + ig * gg;
            h[r] = og * gate_tanh(c[r]);
            dpart = fmaf(dwh[r], h[r] + __builtin_fabsf(h[r]), dpart);
        }
        if constexpr (RG) {
            if (t >= Tb) { h = h_in; c = c_in; }
        }
        const int nxt = cur ^ 1;
        store_h4(smem + nxt * LH_HBUF, LH_HPL, 4 * wave + q, n, h, amax);
        dpart += __shfl_xor(dpart, 16);
        dpart += __shfl_xor(dpart, 32);
        if (q == 0) part[(t & (2 * LH_BLK - 1)) * LH_SLOT + wave * 16 + n] = dpart;
        __syncthreads();
        if ((t & (LH_BLK - 1)) == LH_BLK - 1 || t == T - 1) {        // uniform: this block's scores leave
            const int fc = tid >> 4, fs = tid & (LH_BLK - 1), t_blk = t & ~(LH_BLK - 1);
            const long long fb = (long long)grp * 16 + fc;
            if constexpr (RG) {      // clip fc's row and window count; a refused slot's scores are NaN
                if (tid < 16 * LH_BLK) {
                    const int fclip = rg_clip(rg, grp * 16 + fc);
                    const long long r0 = fclip >= 0 ? rg.t.probs_first[fclip] : 0;
                    const int ftb = fclip >= 0 ? min((int)(rg.t.probs_first[fclip + 1] - r0), T) : 0;
                    long long o_;
                    int l_;
                    const bool fref = !rg_slot(rg, grp * 16 + fc, o_, l_);
                    if (t_blk + fs <= t && t_blk + fs < ftb) {
                        const float *pp = part + ((t_blk + fs) & (2 * LH_BLK - 1)) * LH_SLOT + fc;
                        float s = db;
#pragma unroll
                        for (int w = 0; w < 8; ++w) s += pp[w * 16];
                        probs[r0 + t_blk + fs] = fref ? __builtin_nanf("") : sigmoidf_(s);
                    }
                }
            } else
            if (tid < 16 * LH_BLK && fb < B && t_blk + fs <= t) {
                const float *pp = part + ((t_blk + fs) & (2 * LH_BLK - 1)) * LH_SLOT + fc;
                float s = db;
#pragma unroll
                for (int w = 0; w < 8; ++w) s += pp[w * 16];
                probs[fb * probs_stride + t_blk + fs] = sigmoidf_(s);
            }
        }
        cur = nxt;
    }
    }
    if (state_n != nullptr && bvalid) {
        *reinterpret_cast<f32x4 *>(state_n + b * 128 + u0) = h;
        *reinterpret_cast<f32x4 *>(state_n + ((long long)B + b) * 128 + u0) = c;
    }
    if (!(amax <= H_MAX)) {           // only a caller-supplied initial state can do this
        unsigned *fl = reinterpret_cast<unsigned *>(const_cast<float *>(P)) + OFF_HFLAG + 1;
        atomicOr(fl, 1u);
        atomicMax(fl + 1, __float_as_uint(amax));
    }
    // ... and then this clip group's scores are NaN, not numbers (cf. the encoder's gx).  The overwrite comes from other lanes than the flushes'
    // stores to the same addresses: those are drained (the fence waits for them) before the barrier, so that the NaNs land last.
    __threadfence();
    __syncthreads();
    if (__ballot(!(amax <= H_MAX)) != 0ULL && lane == 0) reinterpret_cast<unsigned *>(part)[wave] = 1u;
    else if (lane == 0) reinterpret_cast<unsigned *>(part)[wave] = 0u;
    __syncthreads();
    {
        const unsigned *bw = reinterpret_cast<const unsigned *>(part);
        if ((bw[0] | bw[1] | bw[2] | bw[3] | bw[4] | bw[5] | bw[6] | bw[7]) != 0u && wave == 0 && lane < 16 && bvalid) {
            if constexpr (RG) for (int t = 0; t < Tb; ++t) prow[t] = __builtin_nanf("");
            else for (int t = 0; t < T; ++t) probs[b * probs_stride + t] = __builtin_nanf("");
        }
    }
}

int silero_lstm_h2_launch(const float *packed, const float *gx, const float *state0, int batch, int G, int steps, float *probs,
                          long long probs_stride, float *state_n, void *stream) {
    hipLaunchKernelGGL(silero_lstm_h2_kernel<false>, dim3(G), dim3(512), LH_BYTES, static_cast<hipStream_t>(stream), packed, gx, state0, batch, G,
                       steps, probs, probs_stride, state_n, RgArg<false>{});
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

int silero_lstm_h2_ragged_launch(const float *packed, const float *gx, const RgArg<true> &rg, float *probs, float *state_n, void *stream,
                                 const float *state0) {
    hipLaunchKernelGGL(silero_lstm_h2_kernel<true>, dim3(rg.t.groups), dim3(512), LH_BYTES, static_cast<hipStream_t>(stream), packed, gx,
                       state0, rg.t.clips, rg.t.groups, 0, probs, 0LL, state_n, rg);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

template <typename S>
int silero_encode_h2_launch(const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                            long long origin, int batch, int G, int steps, int Gws, int first_group, float *gx, void *stream) {
    constexpr int NS = H2_NSUB;
    constexpr int LDS = H2_LDS_BYTES;
    VADX_DYN_LDS((silero_encode_h2_kernel<S, NS>), LDS);
    const long long nblk = (long long)G * ((steps + NS - 1) / NS);
    hipLaunchKernelGGL((silero_encode_h2_kernel<S, NS>), dim3((unsigned)nblk), dim3(H2_THREADS), LDS, static_cast<hipStream_t>(stream),
                       packed, src, in_scale, n_valid, row_stride, origin, batch, G, steps, Gws, first_group, gx, RgArg<false>{});
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
template <typename S>
int silero_encode_h2_ragged_launch(const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx, void *stream,
                                   long long origin) {
    constexpr int NS = H2_NSUB;
    constexpr int LDS = H2_LDS_BYTES;
    VADX_DYN_LDS((silero_encode_h2_kernel<S, NS, true>), LDS);
    hipLaunchKernelGGL((silero_encode_h2_kernel<S, NS, true>), dim3((unsigned)rg.t.n_runs), dim3(H2_THREADS), LDS, static_cast<hipStream_t>(stream),
                       packed, src, in_scale, rg.n_src, 0LL, origin, rg.t.clips, rg.t.groups, 0, 0, 0, gx, rg);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
template int silero_encode_h2_ragged_launch<float>(const float *, const float *, float, const RgArg<true> &, float *, void *, long long);
template int silero_encode_h2_ragged_launch<int16_t>(const float *, const int16_t *, float, const RgArg<true> &, float *, void *, long long);
template int silero_encode_h2_launch<float>(const float *, const float *, float, long long, long long, long long, int, int, int, int, int, float *, void *);
template int silero_encode_h2_launch<int16_t>(const float *, const int16_t *, float, long long, long long, long long, int, int, int, int, int, float *, void *);

}  // namespace silero
}  // namespace vadx
