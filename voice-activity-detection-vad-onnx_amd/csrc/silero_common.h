// silero_common.h -- what the two Silero encoder kernels share: the packed-blob map (filled by csrc/silero_pack.hip), the staged-window layout, the STFT passes.
// (csrc/silero.hip: exact-f32 MFMA encoder; csrc/silero_split.hip: bf16 x 3 split-product encoder, csrc/split3.h)
#pragma once
#include "common.h"

namespace vadx {
namespace silero {

// ---- packed weight blob (float offsets) -------------------------------------------------------
// Encoder GEMM weights are stored FRAGMENT-MAJOR: [16-row tile][16-k block S][lane = 16q+i][4], i.e. exactly the
// f32x4 each lane feeds to the four MFMAs of block S (row 16*tile+i, k = 16S+4q+j).  One wave-wide load is then
// one contiguous 1 KB run (8 full cache lines) instead of 16 half-used lines of a row-major matrix.
constexpr int OFF_STFT = 0;                        // [8 waves][re16|im16][256]  (bins 0..127), k-permuted per 16
constexpr int OFF_NYQ = OFF_STFT + 256 * 256;      // [2][256]                   (bin 128 re, im)
constexpr int C1_KP = 128;                         // input channels 0..127 on MFMA; channel 128 (Nyquist) on VALU
// conv1 runs in the Winograd F(4,3) domain (see "phase 2"): 6 transformed weight planes U_j = G g instead of 3 taps
constexpr int OFF_C1 = OFF_NYQ + 2 * 256;          // [8 oc tiles][6 planes][8 blocks][FRAG]
constexpr int OFF_C1N = OFF_C1 + 128 * 6 * C1_KP;  // [128][8]  the six transformed taps of input channel 128 (+2 pad)
constexpr int OFF_B1 = OFF_C1N + 128 * 8;          // [128]
constexpr int OFF_C2 = OFF_B1 + 128;               // [4 oc tiles][3 taps x 8 blocks][FRAG]
constexpr int OFF_B2 = OFF_C2 + 64 * 3 * 128;      // [64]
constexpr int OFF_C3 = OFF_B2 + 64;                // [4 oc tiles][2 taps x 4 blocks][FRAG]  taps 1,2 (tap 0 only sees padding)
constexpr int OFF_B3 = OFF_C3 + 64 * 2 * 64;       // [64]
constexpr int OFF_C4 = OFF_B3 + 64;                // [8 oc tiles][4 blocks][FRAG]  tap 1 only
constexpr int OFF_B4 = OFF_C4 + 128 * 64;          // [128]
constexpr int OFF_IH = OFF_B4 + 128;               // [4 gates][8 unit tiles][8 blocks][FRAG]
constexpr int OFF_BG = OFF_IH + 512 * 128;         // [512] b_ih + b_hh
constexpr int OFF_HH = OFF_BG + 512;               // [512][128]
constexpr int OFF_DW = OFF_HH + 512 * 128;         // [128]
constexpr int OFF_DB = OFF_DW + 128;               // [1] (+3 pad)
// Folded STFT basis (used when the table has the DFT's time and frequency symmetries, see pack_host and
// stft_fold_class): symmetrised coefficients of bins 0..63 for the even-n / odd-n classes.
constexpr int OFF_SF = OFF_DB + 4;                 // [4 bin tiles][E|O][re|im][4 blocks][FRAG]
constexpr int OFF_S0 = OFF_SF + 4 * 2 * 2 * 4 * 256;   // [2][64]   the n = 0 column (re, im) of bins 0..63
constexpr int OFF_B64 = OFF_S0 + 128;              // [2][128] bin 64, time-folded (re, im), n = 1..128; then [4]: n = 0 (re, im)
constexpr int OFF_FOLD = OFF_B64 + 256 + 4;        // [1] (+3 pad)  1.0 = folded pass valid
// ---- split-product encoder (csrc/silero_split.hip): the same conv / W_ih weights as bf16 x 3 A fragments (csrc/split3.h: one
// fragment = QFRAG floats = 64 lanes x 8 bf16 of one (16-row tile, 32-k chunk, plane)), in the order each wave streams them.
// conv1 is the DIRECT three-tap conv here (each tap fragment serves up to four frames; the Winograd planes serve one each and the matrix
// time they save is cheap on this pipe), its input channels in the order the STFT pass leaves them: slot s <= 64 = bin s,
// slot 64 + k = bin 128 - k (k = 1..63); bin 128 (Nyquist) stays a VALU term.
constexpr int QF = 256;                                   // = vadx::QFRAG
// (every fragment section below starts on a 1 KiB boundary of the blob -- FRAG_ALIGN floats; a wave's fragment load is 64 lanes x 16 B =
//  1 KiB contiguous, and until round 6 the sections sat 48 B past a 64-byte line: every load touched 17 lines instead of 16, every 16-lane quarter
//  5 instead of 4 -- a quarter more L1 traffic for the kernel whose binding resource turned out to be L1 throughput)
constexpr int FRAG_ALIGN = 256;
constexpr int OFF_Q1 = (OFF_FOLD + 4 + FRAG_ALIGN - 1) / FRAG_ALIGN * FRAG_ALIGN;      // [8 oc tiles][4 chunks][3 taps][3 planes][QF]
constexpr int OFF_Q1N = OFF_Q1 + 8 * 4 * 3 * 3 * QF;      // [128 oc][4]: taps 0..2 of input channel 128 (+1 pad), f32
constexpr int OFF_Q2 = OFF_Q1N + 128 * 4;                 // [4 oc tiles][4 chunks][3 taps][3 planes][QF]
constexpr int OFF_Q3 = OFF_Q2 + 4 * 4 * 3 * 3 * QF;       // [4 oc tiles][2 taps (1, 2)][2 chunks][3 planes][QF]
constexpr int OFF_Q4 = OFF_Q3 + 4 * 2 * 2 * 3 * QF;       // [8 oc tiles][2 chunks][3 planes][QF]   centre tap
constexpr int OFF_QIH = OFF_Q4 + 8 * 2 * 3 * QF;          // [8 unit tiles][4 chunks][4 gates][3 planes][QF]
constexpr int OFF_QHH = OFF_QIH + 8 * 4 * 4 * 3 * QF;     // [8 unit tiles][4 gates][4 chunks][3 planes][QF]   W_hh for the split recurrent kernel
// folded STFT basis (OFF_SF's coefficients) as split fragments: [4 bin tiles][E|O][re|im][2 chunks of 32 pairs][3 planes][QF]; pair m of
// the class = sample n = 2 m + 2 (E) / 2 m + 1 (O), in natural order
constexpr int OFF_QSF = OFF_QHH + 8 * 4 * 4 * 3 * QF;
// ---- fp16 x 2 encoder (csrc/silero_h2.hip, csrc/split2.h): the same weights as fragment PAIRS (h0 plane, h1 * 2^11 plane; one fragment =
// HF floats = 64 lanes x 8 fp16), in the order each wave streams them
constexpr int HF = 256;                                   // = vadx::HFRAG
constexpr int OFF_H1 = OFF_QSF + 4 * 2 * 2 * 2 * 3 * QF;  // conv1 [8 oc tiles][4 chunks][3 taps][2 planes][HF], input slots as OFF_Q1
constexpr int OFF_H2 = OFF_H1 + 8 * 4 * 3 * 2 * HF;       // conv2 [4 oc tiles][4 chunks][3 taps][2][HF]
constexpr int OFF_H3 = OFF_H2 + 4 * 4 * 3 * 2 * HF;       // conv3 [4 oc tiles][2 taps (1, 2)][2 chunks][2][HF]
constexpr int OFF_H4 = OFF_H3 + 4 * 2 * 2 * 2 * HF;       // conv4 [8 oc tiles][2 chunks][2][HF]   centre tap
constexpr int OFF_HIH = OFF_H4 + 8 * 2 * 2 * HF;          // W_ih [8 unit tiles][4 chunks][4 gates][2][HF]
constexpr int OFF_HHH = OFF_HIH + 8 * 4 * 4 * 2 * HF;     // W_hh [8 unit tiles][4 gates][4 chunks][2][HF]
// folded STFT basis: [5 bin tiles][E|O][re|im][2 chunks of 32 pairs][2][HF]; tiles 0..3 = bins 0..63 (OFF_SF's coefficients), tile 4 row 0 =
// bin 64 (OFF_B64's time-folded coefficients, rows 1..15 zero); pair m of the class = sample n = 2 m + 2 (E) / 2 m + 1 (O)
constexpr int OFF_HSF = OFF_HHH + 8 * 4 * 4 * 2 * HF;
// [0] 1.0 = the fp16 x 2 kernels may run on this blob (every weight inside the fp16 range, folded basis); [1] sticky range flag, written
// by the kernels as an unsigned (non-zero: some activation left the fp16 range, the batch must be recomputed on the bf16 x 3 kernels);
// [2] bits of the largest |activation| seen by a flagged workgroup; [3] pad
constexpr int OFF_HFLAG = OFF_HSF + 5 * 2 * 2 * 2 * 2 * HF;
constexpr int PACKED_FLOATS = OFF_HFLAG + 4;
// ---- the 8 kHz blob (csrc/silero8k.hip): the 16 kHz layout (PACKED_FLOATS floats), every section the two networks share at its 16 kHz offset
// (conv2..4, W_ih, W_hh in all three layouts, biases, decoder, OFF_HFLAG), the 8 kHz STFT and conv1 in [0, OFF_B1) -- where a 16 kHz blob keeps
// ITS STFT and conv1, which an 8 kHz launch never reads.  conv1's bias sits at OFF_B1.  Fragment orders: [row tile][tap][32-k chunk] x one
// chunk's fragments (f32: two FRAG blocks of 256 floats; bf16 x 3: three QF planes; fp16 x 2: two HF planes).
constexpr int OFF8_SF = 0;                                // STFT f32  [9 row tiles][4 chunks][2 FRAG]
constexpr int OFF8_SQ = OFF8_SF + 9 * 4 * 2 * 256;        //      bf16 x 3 [9][4][3][QF]
constexpr int OFF8_SH = OFF8_SQ + 9 * 4 * 3 * QF;         //      fp16 x 2 [9][4][2][HF]
constexpr int OFF8_C1F = OFF8_SH + 9 * 4 * 2 * HF;        // conv1 (input channels 0..63) f32 [8 oc tiles][3 taps][2 chunks][2 FRAG]
constexpr int OFF8_C1Q = OFF8_C1F + 8 * 3 * 2 * 2 * 256;  //      bf16 x 3 [8][3][2][3][QF]
constexpr int OFF8_C1H = OFF8_C1Q + 8 * 3 * 2 * 3 * QF;   //      fp16 x 2 [8][3][2][2][HF]
constexpr int OFF8_C1N = OFF8_C1H + 8 * 3 * 2 * 2 * HF;   // [128 oc][4]: taps 0..2 of input channel 64 (+1 pad), f32
constexpr int OFF8_END = OFF8_C1N + 128 * 4;
// the tag: a pad word of the 16 kHz layout (behind OFF_FOLD), zero in every 16 kHz blob.  An 8 kHz launch on a blob without it writes NaN gx
// and raises bit 2 of the range flag.
constexpr int OFF8_TAG = OFF_FOLD + 1;
constexpr float TAG8K = 8000.f;
static_assert(FRAG == 256 && OFF8_END <= OFF_B1 && OFF8_SF % FRAG_ALIGN == 0 && OFF8_SQ % FRAG_ALIGN == 0 && OFF8_SH % FRAG_ALIGN == 0 &&
                  OFF8_C1F % FRAG_ALIGN == 0 && OFF8_C1Q % FRAG_ALIGN == 0 && OFF8_C1H % FRAG_ALIGN == 0,
              "8 kHz blob map");

constexpr int X_LDM = 642;            // staged window row: 576 samples + 64 reflect pad (+2: bank = 2 clip + q, conflict free)
// gx: per (t, group) 8 waves x 4 gates x 64 lanes x 4 floats
constexpr int GX_TILE_FLOATS = 8 * 4 * 256;

// m-major operand variant of gemm_pass for the STFT: act element (m, k) at act[m*ldm + k], this lane's
// m = lane&15, the k consumed by (block S, sub-step j, quarter q) is 16S + q + 4j (the basis rows are
// packed with the matching permutation, so weights still arrive as one 16-B load per block).
// SWAP: the table is the A operand, so D rows = table rows (bins) and D columns = act rows (clips) -- the orientation the split-product
// encoder's LDS planes want (a lane then holds four consecutive bins of one clip).  Same registers either way.
template <int NT, int MT, int KB, bool SWAP = false>
__device__ __forceinline__ void gemm_pass_mmajor(f32x4 (&acc)[NT][MT], const float *act, int ldm,
                                                 const int (&koff)[MT], const float *const (&wrow)[NT], int lane) {
    const int q = lane >> 4, i = lane & 15;
    const float *ap = act + i * ldm + q;
    f32x4 wcur[NT], wnxt[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wcur[nt] = *reinterpret_cast<const f32x4 *>(wrow[nt] + 4 * q);
#pragma unroll 1
    for (int S = 0; S < KB; ++S) {
        const int Sn = (S + 1 < KB) ? S + 1 : S;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wnxt[nt] = *reinterpret_cast<const f32x4 *>(wrow[nt] + 16 * Sn + 4 * q);
        const float *aps = ap + 16 * S;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = aps[4 * j + koff[mt]];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float wj = wcur[nt][j];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = SWAP ? mfma16(wj, av[mt], acc[nt][mt]) : mfma16(av[mt], wj, acc[nt][mt]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wcur[nt] = wnxt[nt];
    }
}

// Folded STFT pass.  A windowed real-DFT basis (symmetric window) has two symmetries that the dense 258x256
// conv ignores:
//   time      c[k][256-n] =  c[k][n],  s[k][256-n] = -s[k][n]        -> contract x[n] +- x[256-n] over n = 1..128
//   frequency c[128-k][n] = (-1)^n c[k][n],  s[128-k][n] = -(-1)^n s[k][n]
//                                                                    -> bins k and 128-k share the partial sums over
//                                                                       even n (E) and odd n (O): X[k] = E + O, X[128-k] = +-(E - O)
// so bins 0..63 (4 tiles) over two 64-long contractions give all of bins 0..63 and 65..128: a quarter of the dense
// pass's MFMAs, for two VALU adds per operand pair.  (Bin 64 pairs with itself and goes through the VALU.)
// X is staged de-interleaved: per clip row an even-sample plane [0..320] and an odd-sample plane [321..641], so the
// contraction index of either class walks its plane with unit stride (bank = 2*clip + q: conflict free).
// Class E: n = 2m + 2 (plane index m + 1, mirror 127 - m); class O: n = 2m + 1 (plane index m, mirror 127 - m);
// contraction slot (block S, sub-step j, quarter q) <-> m = 16S + q + 4j.
constexpr int X_ODD = 322;            // offset of the odd plane inside a clip row (even: the staging code stores sample pairs 8 B wide)
template <bool SWAP = false>
__device__ __forceinline__ void stft_fold_class(f32x4 (&are)[2], f32x4 (&aim)[2], const float *fwd, const float *rev,
                                                const float *wre, const float *wim) {
    f32x4 cre = *reinterpret_cast<const f32x4 *>(wre), cim = *reinterpret_cast<const f32x4 *>(wim);
#pragma unroll
    for (int S = 0; S < 4; ++S) {
        const int Sn = (S + 1 < 4) ? S + 1 : S;
        const f32x4 nre = *reinterpret_cast<const f32x4 *>(wre + FRAG * Sn);
        const f32x4 nim = *reinterpret_cast<const f32x4 *>(wim + FRAG * Sn);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (forming the two frames' operands as f32x2 pairs for v_pk_add_f32 -- half the adds -- costs more in register
            // shuffles than it saves: 291 instead of 199 VALU instructions in this loop)
            float e[2], o[2];
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const float a = fwd[16 * S + 4 * j + 64 * f], b = rev[64 * f - 16 * S - 4 * j];
                e[f] = a + b;
                o[f] = a - b;
            }
#pragma unroll
            for (int f = 0; f < 2; ++f) are[f] = SWAP ? mfma16(cre[j], e[f], are[f]) : mfma16(e[f], cre[j], are[f]);
#pragma unroll
            for (int f = 0; f < 2; ++f) aim[f] = SWAP ? mfma16(cim[j], o[f], aim[f]) : mfma16(o[f], cim[j], aim[f]);
        }
        cre = nre;
        cim = nim;
    }
}

// |STFT| magnitude: the bare v_sqrt_f32 (1 ulp).  sqrtf() is the correctly rounded, denormal-safe library routine -- about fifteen
// VALU instructions per value -- and on gfx950 VALU work does not hide under v_mfma_f32_16x16x4_f32: the two ADD UP on a SIMD
// (tools/mfma_valu_overlap.sh: 15.2 ns per MFMA alone, +1.8 ns per v_fma_f32 placed beside it, one or two waves per SIMD alike).
__device__ __forceinline__ float mag_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Sample fetch of phase 0: the reference feeds Silero float32 = int16 * 0.000030517578 (Silero/Inference_Silero_VAD_ONNX.py:83);
// the PCM16 instantiation reads the int16 samples themselves (half the HBM read, no f32 copy of the batch) and applies
// that very multiplication -- one f32 rounding, bit-identical to the host-side product.
template <typename SampleT> struct SampleIO;
template <> struct SampleIO<float> {
    static constexpr int VEC_ALIGN = 16;
    static __device__ __forceinline__ f32x4 load4(const float *p, float) { return *reinterpret_cast<const f32x4 *>(p); }
    static __device__ __forceinline__ float load1(const float *p, float) { return *p; }
};
template <> struct SampleIO<int16_t> {
    static constexpr int VEC_ALIGN = 8;
    static __device__ __forceinline__ f32x4 load4(const int16_t *p, float scale) {
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        const s16x4 v = *reinterpret_cast<const s16x4 *>(p);
        return f32x4{(float)v[0] * scale, (float)v[1] * scale, (float)v[2] * scale, (float)v[3] * scale};
    }
    static __device__ __forceinline__ float load1(const int16_t *p, float scale) { return (float)*p * scale; }
};

// ---- ragged batches (include/vadx.h: vadx_silero_ragged) -----------------------------------------
// The ragged kernels are second instantiations of the rectangular ones under the compile-time flag RG: (group, window) comes from the
// workgroup table, the staging base and length are per slot, a group's gx tiles lie consecutively.  The rectangular instantiation's last
// kernel argument is an empty struct: nothing of the tables reaches its code.
enum : int { RG_RUN = VADX_SILERO_RAGGED_RUN };      // windows per entry of the workgroup table
template <bool RG> struct RgArg {};
template <> struct RgArg<true> {
    vadx_silero_ragged t;
    long long n_src;          // elements of the source vector: every slot is checked against it before anything of it is read
};

// Slot `slot` as the device accepts it: (off, len) of a clip that lies inside the source vector, (0, 0) for an empty slot and for one
// that does not (-> false: the slot is refused).  Nothing is read through a refused slot's offset.
__device__ __forceinline__ bool rg_slot(const RgArg<true> &rg, int slot, long long &off, int &len) {
    const bool used = rg.t.slot_clip[slot] >= 0;
    const long long o = rg.t.slot_off[slot];
    const int l = rg.t.slot_len[slot];
    const bool ok = used && l >= 1 && o >= 0 && o <= rg.n_src - (long long)l;
    off = ok ? o : 0;
    len = ok ? l : 0;
    return ok || !used;
}
// the caller's clip of a slot (-1: none) -- an index outside [0, clips) counts as none
__device__ __forceinline__ int rg_clip(const RgArg<true> &rg, int slot) {
    const int c = rg.t.slot_clip[slot];
    return (unsigned)c < (unsigned)rg.t.clips ? c : -1;
}

// Phase 0 of a ragged tile: window `base` .. base + 575 (+ reflect pad) of the sixteen slots of group grp into X, laid out as the
// rectangular kernels stage it.  Slot c reads its clip as those read a row with n_samples = its own length: zeros before the clip and
// beyond its end, the pad mirrored over that.  A float4 that lies inside the clip is one vector load when the clip starts on a multiple of
// four elements (base and p are multiples of four), single loads otherwise; `whole` (uniform: the window ends below the group's shortest
// accepted length) spares the per-float4 range test.
template <typename SampleT, int THREADS>
__device__ __forceinline__ void stage_ragged(float *X, bool fold, const SampleT *__restrict__ audio, float in_scale,
                                             const RgArg<true> &rg, int grp, long long base, int tid) {
    auto xslot = [fold](int pp) { return fold ? (pp & 1) * X_ODD + (pp >> 1) : pp; };
    const bool ptr_ok = (reinterpret_cast<uintptr_t>(audio) & (SampleIO<SampleT>::VEC_ALIGN - 1)) == 0;
    int shortest;
    {
        long long o_;
        rg_slot(rg, grp * 16 + (tid & 15), o_, shortest);
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) shortest = min(shortest, __shfl_xor(shortest, d));
        shortest = min(shortest, rg.t.grp_min_len[grp]);
    }
    const bool whole = base >= 0 && base + 576 <= (long long)shortest;
#pragma unroll 1
    for (int it = 0; it < (16 * 144 + THREADS - 1) / THREADS; ++it) {
        const int e = tid + THREADS * it;                // 16 clips x 144 float4
        if (e < 16 * 144) {
            const int c = e / 144, p = 4 * (e - c * 144);
            long long off;
            int len;
            if (!rg_slot(rg, grp * 16 + c, off, len) && p == 0) atomicOr(rg.t.status, 1u);
            const SampleT *src = audio + off;
            const long long idx = base + p;
            float v[4];
            if (ptr_ok && (off & 3) == 0 && (whole || (idx >= 0 && idx + 3 < len))) {
                const f32x4 x = SampleIO<SampleT>::load4(src + idx, in_scale);
                v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    v[jj] = (idx + jj >= 0 && idx + jj < len) ? SampleIO<SampleT>::load1(src + idx + jj, in_scale) : 0.f;
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

// host: the ragged launches of the three kernel sets (csrc/silero.hip picks by cfg).  origin: the first window's first sample within a slot
// (-64: a clip, whose context is zeros; 0: a staged stream row [context | windows], csrc/silero_stream.hip); state0: NULL = zeros, or
// [2][clips][128] indexed by clip
template <typename S>
int silero_encode_split_ragged_launch(const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx, void *stream,
                                      long long origin = -64LL);
template <typename S>
int silero_encode_h2_ragged_launch(const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx, void *stream,
                                   long long origin = -64LL);
int silero_lstm_split_ragged_launch(const float *packed, const float *gx, const RgArg<true> &rg, float *probs, float *state_n, void *stream,
                                    const float *state0 = nullptr);
int silero_lstm_h2_ragged_launch(const float *packed, const float *gx, const RgArg<true> &rg, float *probs, float *state_n, void *stream,
                                 const float *state0 = nullptr);
// csrc/silero.hip: the ragged encoder and recurrent launches on an argument the caller has checked, kernel set by cfg, network by rate --
// what vadx_silero_encode_ragged / _recur_ragged issue, also called by the ragged stream tick
template <typename S>
int silero_encode_ragged_launch(int rate, const vadx_silero_cfg *cfg, const float *packed, const S *src, float in_scale, const RgArg<true> &rg,
                                float *gx, void *stream, long long origin);
int silero_recur_ragged_launch(const vadx_silero_cfg *cfg, const float *packed, const float *gx, const RgArg<true> &rg, float *probs,
                               float *state_n, void *stream, const float *state0);

// host: launch of the split-product encoder (csrc/silero_split.hip); arguments as silero_encode_kernel's
template <typename S>
int silero_encode_split_launch(const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                               long long origin, int batch, int G, int steps, int Gws, int first_group, float *gx, void *stream);

// csrc/silero_h2.hip: the fp16 x 2 encoder and recurrent kernels (arguments as the bf16 x 3 launches)
template <typename S>
int silero_encode_h2_launch(const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                            long long origin, int batch, int G, int steps, int Gws, int first_group, float *gx, void *stream);
int silero_lstm_h2_launch(const float *packed, const float *gx, const float *state0, int batch, int G, int steps, float *probs,
                          long long probs_stride, float *state_n, void *stream);

// csrc/silero.hip: the encoder and recurrent launches behind every Silero entry point (the kernel set comes from cfg), also called by the
// stream path (csrc/silero_stream.hip)
template <typename S>
int silero_encode_launch(const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                         long long origin, int batch, int steps, void *ws, size_t ws_bytes, void *stream,
                         const vadx_silero_cfg *cfg, int first_group = 0, int total_batch = 0);
int silero_recur_launch(const float *packed, const void *ws, size_t ws_bytes, int batch, int steps,
                        const float *state0, float *probs, long long probs_stride, float *state_n, void *stream,
                        const vadx_silero_cfg *cfg);

// csrc/silero8k.hip: the 8 kHz network's encoder (arith = VADX_AR_*; arguments otherwise as silero_encode_split_launch, windows of 256)
template <typename S>
int silero8k_encode_launch(int arith, const float *packed, const S *src, float in_scale, long long n_valid, long long row_stride,
                           long long origin, int batch, int G, int steps, int Gws, int first_group, float *gx, void *stream);
// ... and its ragged launch (the tables' windows are windows of 256)
template <typename S>
int silero8k_encode_ragged_launch(int arith, const float *packed, const S *src, float in_scale, const RgArg<true> &rg, float *gx,
                                  void *stream, long long origin = -32LL);

int silero_lstm_split_launch(const float *packed, const float *gx, const float *state0, int batch, int G, int steps, float *probs,
                             long long probs_stride, float *state_n, void *stream);

}  // namespace silero
}  // namespace vadx
