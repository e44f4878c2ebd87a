// silero_pack.hip -- host only: the Silero packed blob of the 16 kHz and the 8 kHz network (the map: csrc/silero_common.h).  No kernel here.
// Every tensor is one view of the (rebalanced) weights and up to three lines: its float32 fragment-major section, its bf16 x 3 and its
// fp16 x 2 fragments in the order the kernels stream them (csrc/pack.h owns the walk).
#include "silero_common.h"
#include "pack.h"
#include "rebalance.h"

#include <math.h>
#include <string.h>
#include <vector>

using namespace vadx::silero;
using vadx::SchemeB3;
using vadx::SchemeH2;
namespace pack = vadx::pack;

namespace {

// A tensor's split section [n0][n1][n2][NP planes][QF]: one (16-row tile, 32-k chunk) per (a, b, c), view(a, b, c, i, k) = the weight at
// row i, contraction index k of that group; hmax as Sch::put_host's running max
template <class Sch, class View>
void sections(float *dst, int n0, int n1, int n2, View view, float &hmax) {
    for (int a = 0; a < n0; ++a)
        for (int b = 0; b < n1; ++b)
            for (int c = 0; c < n2; ++c)
                pack::group<Sch>(dst + (size_t)(((a * n1 + b) * n2 + c) * Sch::NP) * QF, [&](int i, int k) { return view(a, b, c, i, k); }, hmax);
}

// conv weight [co][cin][3 taps] as (co, ci, tap) -> float
auto conv_view(const float *w, int cin) {
    return [=](int co, int ci, int tap) { return w[((size_t)co * cin + ci) * 3 + tap]; };
}

// contraction slot 16S + 4q + j <-> k = 16S + q + 4j of the m-major STFT passes (its own inverse)
int kperm(int k) { return 16 * (k / 16) + 4 * (k % 4) + (k % 16) / 4; }

// The 16 kHz network's own sections: STFT basis [258][256] (dense rows and, when the table allows it, the folded basis), conv1 [128][129][3]
void pack_front_16k(const vadx_silero_weights_host *w, float *p, float &hmax) {
    // STFT basis rows regrouped per wave: [wave][re 16 bins | im 16 bins][256]
    for (int wv = 0; wv < 8; ++wv)
        for (int part = 0; part < 2; ++part)
            for (int i = 0; i < 16; ++i)
                for (int k = 0; k < 256; ++k)
                    p[OFF_STFT + (size_t)(wv * 32 + part * 16 + i) * 256 + kperm(k)] = w->stft_basis[(size_t)(part * 129 + wv * 16 + i) * 256 + k];
    memcpy(p + OFF_NYQ, w->stft_basis + (size_t)128 * 256, 256 * sizeof(float));
    memcpy(p + OFF_NYQ + 256, w->stft_basis + (size_t)257 * 256, 256 * sizeof(float));
    {   // folded basis: valid when the table has the time symmetry c[k][256-n] == c[k][n], s[k][256-n] == -s[k][n]
        // (n = 1..127; s[k][128] == 0) AND the frequency symmetry c[128-k][n] == (-1)^n c[k][n],
        // s[128-k][n] == -(-1)^n s[k][n], both up to f32 rounding of the table (1e-6 of the largest entry) -- which
        // every windowed real-DFT basis satisfies.  Otherwise the kernel takes the dense pass.
        const float *re = w->stft_basis, *im = w->stft_basis + (size_t)129 * 256;
        float amax = 0.f, dev = 0.f;
        for (size_t e = 0; e < (size_t)258 * 256; ++e) amax = fmaxf(amax, fabsf(w->stft_basis[e]));
        for (int k = 0; k <= 128; ++k) {
            for (int n = 1; n < 128; ++n) {
                dev = fmaxf(dev, fabsf(re[k * 256 + n] - re[k * 256 + 256 - n]));
                dev = fmaxf(dev, fabsf(im[k * 256 + n] + im[k * 256 + 256 - n]));
            }
            dev = fmaxf(dev, fabsf(im[k * 256 + 128]));
        }
        for (int k = 0; k < 64; ++k)
            for (int n = 0; n < 256; ++n) {
                const float sg = (n & 1) ? -1.f : 1.f;
                dev = fmaxf(dev, fabsf(re[(128 - k) * 256 + n] - sg * re[k * 256 + n]));
                dev = fmaxf(dev, fabsf(im[(128 - k) * 256 + n] + sg * im[k * 256 + n]));
            }
        const bool fold = dev <= 1e-6f * amax;
        p[OFF_FOLD] = fold ? 1.f : 0.f;
        if (fold) {
            // symmetrised coefficient of bin k (<= 64) at sample n: average of the four table entries that must agree
            auto C = [&](int k, int n) {
                const float sg = (n & 1) ? -1.f : 1.f;
                const int nm = (256 - n) & 255;
                return 0.25f * (re[k * 256 + n] + re[k * 256 + nm] + sg * (re[(128 - k) * 256 + n] + re[(128 - k) * 256 + nm]));
            };
            auto S = [&](int k, int n) {
                const float sg = (n & 1) ? -1.f : 1.f;
                const int nm = (256 - n) & 255;
                return 0.25f * (im[k * 256 + n] - im[k * 256 + nm] - sg * (im[(128 - k) * 256 + n] - im[(128 - k) * 256 + nm]));
            };
            for (int k = 0; k < 64; ++k) {
                p[OFF_S0 + k] = 0.5f * (re[k * 256] + re[(128 - k) * 256]);
                p[OFF_S0 + 64 + k] = 0.5f * (im[k * 256] - im[(128 - k) * 256]);
            }
            for (int n = 1; n <= 128; ++n) {          // bin 64, time-folded only
                const float h = (n == 128) ? 0.5f : 1.f;
                p[OFF_B64 + n - 1] = h * 0.5f * (re[64 * 256 + n] + re[64 * 256 + ((256 - n) & 255)]);
                p[OFF_B64 + 128 + n - 1] = (n == 128) ? 0.f : 0.5f * (im[64 * 256 + n] - im[64 * 256 + 256 - n]);
            }
            p[OFF_B64 + 256] = re[64 * 256];
            p[OFF_B64 + 257] = im[64 * 256];
            // the folded table [5 bin tiles x 16][E|O][re|im][64 pairs]: pair m of a class = sample n = 2 m + 2 (E) / 2 m + 1 (O); rows 0..63 =
            // bins 0..63, row 64 = bin 64 (OFF_B64's coefficients; only the fp16 x 2 STFT runs it on the matrix pipe), rows 65..79 zero
            std::vector<float> sf((size_t)80 * 256, 0.f);
            for (int cls = 0; cls < 2; ++cls)
                for (int m = 0; m < 64; ++m) {
                    const int n = cls ? 2 * m + 1 : 2 * m + 2;
                    for (int k = 0; k < 64; ++k) {
                        // n = 128 is its own mirror: x[128] gets added to itself, so its coefficient is halved
                        sf[(size_t)k * 256 + (cls * 2 + 0) * 64 + m] = (n == 128) ? 0.5f * C(k, 128) : C(k, n);
                        sf[(size_t)k * 256 + (cls * 2 + 1) * 64 + m] = (n == 128) ? 0.f : S(k, n);
                    }
                    sf[(size_t)64 * 256 + (cls * 2 + 0) * 64 + m] = p[OFF_B64 + n - 1];
                    sf[(size_t)64 * 256 + (cls * 2 + 1) * 64 + m] = p[OFF_B64 + 128 + n - 1];
                }
            auto fold_view = [&](int tl, int cp, int kc, int i, int k) { return sf[(size_t)(16 * tl + i) * 256 + cp * 64 + 32 * kc + k]; };
            pack::f32(p + OFF_SF, 256, 64, 256, [&](int r, int c) { return sf[(size_t)r * 256 + (c & ~63) + kperm(c % 64)]; });
            sections<SchemeB3>(p + OFF_QSF, 4, 4, 2, fold_view, hmax);      // pairs in natural order
            sections<SchemeH2>(p + OFF_HSF, 5, 4, 2, fold_view, hmax);
        }
    }
    const auto c1 = conv_view(w->enc_w[0], 129);
    {   // conv1 in the Winograd F(4,3) domain: U_j[co][ci] = sum_t G[j][t] g[co][ci][t], evaluated in float64
        static const double G[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                       {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
        auto U = [&](int co, int ci, int j) {
            return (float)(G[j][0] * (double)c1(co, ci, 0) + G[j][1] * (double)c1(co, ci, 1) + G[j][2] * (double)c1(co, ci, 2));
        };
        pack::f32(p + OFF_C1, 6 * C1_KP, 128, 6 * C1_KP, [&](int co, int c) { return U(co, c % C1_KP, c / C1_KP); });
        for (int co = 0; co < 128; ++co)
            for (int j = 0; j < 6; ++j) p[OFF_C1N + co * 8 + j] = U(co, 128, j);
    }
    // the split encoders run conv1 as the direct three-tap conv, input channels in the order the STFT pass leaves the bins in
    auto c1_view = [&](int rt, int kc, int tap, int i, int k) {
        const int slot = 32 * kc + k;
        return c1(16 * rt + i, slot <= 64 ? slot : 192 - slot, tap);
    };
    sections<SchemeB3>(p + OFF_Q1, 8, 4, 3, c1_view, hmax);
    sections<SchemeH2>(p + OFF_H1, 8, 4, 3, c1_view, hmax);
    for (int co = 0; co < 128; ++co)
        for (int tap = 0; tap < 3; ++tap) p[OFF_Q1N + co * 4 + tap] = c1(co, 128, tap);
}

// The 8 kHz network's own sections, in [0, OFF_B1): the dense STFT basis [130][128] and conv1 [128][65][3]
void pack_front_8k(const vadx_silero_weights_host *w, float *p, float &hmax) {
    // STFT rows: tiles 0..3 = re of bins 0..63, 4..7 = im of bins 0..63, 8 = re (row 0) and im (row 1) of bin 64
    auto stft = [&](int r, int k) {
        const int src = r < 64 ? r : (r < 128 ? 65 + (r - 64) : (r == 128 ? 64 : (r == 129 ? 129 : -1)));
        return src < 0 ? 0.f : w->stft_basis[(size_t)src * 128 + k];
    };
    pack::f32(p + OFF8_SF, 128, 9 * 16, 128, stft);
    pack::split<SchemeB3>(p + OFF8_SQ, 9, 4, stft, hmax);
    pack::split<SchemeH2>(p + OFF8_SH, 9, 4, stft, hmax);
    // conv1: input channels 0..63 as fragments [8 oc tiles][3 taps][2 chunks], channel 64 as VALU taps
    const auto c1 = conv_view(w->enc_w[0], 65);
    auto c1_view = [&](int rt, int tap, int kc, int i, int k) { return c1(16 * rt + i, 32 * kc + k, tap); };
    pack::f32(p + OFF8_C1F, 3 * 64, 128, 3 * 64, [&](int co, int c) { return c1(co, c % 64, c / 64); });
    sections<SchemeB3>(p + OFF8_C1Q, 8, 3, 2, c1_view, hmax);
    sections<SchemeH2>(p + OFF8_C1H, 8, 3, 2, c1_view, hmax);
    for (int co = 0; co < 128; ++co)
        for (int tap = 0; tap < 3; ++tap) p[OFF8_C1N + co * 4 + tap] = c1(co, 64, tap);
    p[OFF8_TAG] = TAG8K;
}

// Every section the two networks share: conv2..4, W_ih, W_hh in all three layouts, the biases, the decoder
void pack_shared(const vadx_silero_weights_host *w, float *p, float &hmax) {
    const auto c2 = conv_view(w->enc_w[1], 128), c3 = conv_view(w->enc_w[2], 64), c4 = conv_view(w->enc_w[3], 64);
    auto ih = [&](int g, int unit, int k) { return w->lstm_w_ih[(size_t)(g * 128 + unit) * 128 + k]; };
    auto hh = [&](int g, int unit, int k) { return w->lstm_w_hh[(size_t)(g * 128 + unit) * 128 + k]; };
    // conv2: three taps of 128 input channels
    auto c2_view = [&](int rt, int kc, int tap, int i, int k) { return c2(16 * rt + i, 32 * kc + k, tap); };
    pack::f32(p + OFF_C2, 3 * 128, 64, 3 * 128, [&](int co, int c) { return c2(co, c % 128, c / 128); });
    sections<SchemeB3>(p + OFF_Q2, 4, 4, 3, c2_view, hmax);
    sections<SchemeH2>(p + OFF_H2, 4, 4, 3, c2_view, hmax);
    // conv3 (stride 2 over two frames): taps 1, 2 -- tap 0 only sees padding
    auto c3_view = [&](int rt, int th, int kc, int i, int k) { return c3(16 * rt + i, 32 * kc + k, th + 1); };
    pack::f32(p + OFF_C3, 2 * 64, 64, 2 * 64, [&](int co, int c) { return c3(co, c % 64, c / 64 + 1); });
    sections<SchemeB3>(p + OFF_Q3, 4, 2, 2, c3_view, hmax);
    sections<SchemeH2>(p + OFF_H3, 4, 2, 2, c3_view, hmax);
    // conv4 (one frame): the centre tap
    auto c4_view = [&](int r, int k) { return c4(r, k, 1); };
    pack::f32(p + OFF_C4, 64, 128, 64, c4_view);
    pack::split<SchemeB3>(p + OFF_Q4, 8, 2, c4_view, hmax);
    pack::split<SchemeH2>(p + OFF_H4, 8, 2, c4_view, hmax);
    // W_ih: row = gate * 128 + unit; a wave owns one 16-unit tile of all four gates
    auto ih_view = [&](int wv, int kc, int g, int i, int k) { return ih(g, 16 * wv + i, 32 * kc + k); };
    pack::f32(p + OFF_IH, 128, 512, 128, pack::rowmajor(w->lstm_w_ih, 512, 128));
    sections<SchemeB3>(p + OFF_QIH, 8, 4, 4, ih_view, hmax);
    sections<SchemeH2>(p + OFF_HIH, 8, 4, 4, ih_view, hmax);
    // W_hh: row-major for the float32 recurrent kernel
    auto hh_view = [&](int wv, int g, int kc, int i, int k) { return hh(g, 16 * wv + i, 32 * kc + k); };
    memcpy(p + OFF_HH, w->lstm_w_hh, 512 * 128 * sizeof(float));
    sections<SchemeB3>(p + OFF_QHH, 8, 4, 4, hh_view, hmax);
    sections<SchemeH2>(p + OFF_HHH, 8, 4, 4, hh_view, hmax);
    memcpy(p + OFF_B2, w->enc_b[1], 64 * sizeof(float));
    memcpy(p + OFF_B3, w->enc_b[2], 64 * sizeof(float));
    memcpy(p + OFF_B4, w->enc_b[3], 128 * sizeof(float));
    for (int r = 0; r < 512; ++r) p[OFF_BG + r] = w->lstm_b_ih[r] + w->lstm_b_hh[r];
    memcpy(p + OFF_DW, w->dec_w, 128 * sizeof(float));
    p[OFF_DB] = w->dec_b[0];
}

// c1_in = conv1's input channels: 129 (16 kHz: 256-point STFT) or 65 (8 kHz: 128-point STFT); who = the entry point, for its messages
int pack_blob(const char *who, int c1_in, const vadx_silero_weights_host *w_in, float *p) {
    VADX_REQUIRE(w_in && p, "%s: NULL argument", who);
    VADX_REQUIRE(w_in->stft_basis && w_in->lstm_w_ih && w_in->lstm_w_hh && w_in->lstm_b_ih && w_in->lstm_b_hh && w_in->dec_w && w_in->dec_b,
                 "%s: NULL weight pointer", who);
    for (int k = 0; k < 4; ++k) VADX_REQUIRE(w_in->enc_w[k] && w_in->enc_b[k], "%s: NULL encoder weight %d", who, k);
    memset(p, 0, sizeof(float) * PACKED_FLOATS);
    // conv1 -> ReLU -> conv2 -> ReLU -> conv3 -> ReLU -> conv4 -> ReLU -> W_ih is one chain of affine layers with only ReLU between them: exact
    // power-of-two rebalancing (csrc/rebalance.h) when a layer's weights sit outside [2^-10, 2^7); ordinary checkpoints pass through untouched.
    // gx (b_ih + b_hh, then the LSTM's non-linearities) stays at its true scale: W_ih is the segment's last layer.
    const size_t enc_nw[4] = {(size_t)128 * c1_in * 3, 64 * 128 * 3, 64 * 64 * 3, 128 * 64 * 3}, enc_nb[4] = {128, 64, 64, 128};
    std::vector<float> rw[5], rb[4];
    for (int k = 0; k < 4; ++k) { rw[k].assign(w_in->enc_w[k], w_in->enc_w[k] + enc_nw[k]); rb[k].assign(w_in->enc_b[k], w_in->enc_b[k] + enc_nb[k]); }
    rw[4].assign(w_in->lstm_w_ih, w_in->lstm_w_ih + 512 * 128);
    int reb_min = 1000;
    vadx::rebalance_chain({{&rw[0], &rb[0]}, {&rw[1], &rb[1]}, {&rw[2], &rb[2]}, {&rw[3], &rb[3]}, {&rw[4], nullptr}}, &reb_min);
    vadx_silero_weights_host w = *w_in;
    for (int k = 0; k < 4; ++k) { w.enc_w[k] = rw[k].data(); w.enc_b[k] = rb[k].data(); }
    w.lstm_w_ih = rw[4].data();
    {   // W_hh stands outside the chain; its exponent counts for the refusal below all the same
        const int e = vadx::reb_exponent(std::vector<float>(w.lstm_w_hh, w.lstm_w_hh + 512 * 128));
        if (e > -100000 && e < reb_min) reb_min = e;
    }
    float hmax = 0.f;       // largest |weight| handed to the fp16 x 2 fragments
    const bool is_16k = c1_in == 129;
    if (is_16k) pack_front_16k(&w, p, hmax);
    else pack_front_8k(&w, p, hmax);
    memcpy(p + OFF_B1, w.enc_b[0], 128 * sizeof(float));
    pack_shared(&w, p, hmax);
    // the fp16 x 2 kernels may run on this blob when every weight is inside the fp16 range, no weight tensor lies wholly below the smallest
    // normal fp16 once the chain is rebalanced (csrc/rebalance.h), and -- at 16 kHz, whose fp16 x 2 STFT is the folded pass only (the 8 kHz
    // one is dense) -- the folded basis is valid
    p[OFF_HFLAG] = ((!is_16k || p[OFF_FOLD] != 0.f) && hmax <= vadx::H_MAX && reb_min >= vadx::REB_REFUSE) ? 1.f : 0.f;
    return VADX_OK;
}

}  // namespace

extern "C" size_t vadx_silero_packed_floats(void) { return (size_t)PACKED_FLOATS; }

extern "C" size_t vadx_silero_packed_floats_sr(int sample_rate) {
    return (sample_rate == 16000 || sample_rate == 8000) ? (size_t)PACKED_FLOATS : 0;
}

extern "C" int vadx_silero_pack_host(const vadx_silero_weights_host *w, float *p) { return pack_blob("vadx_silero_pack_host", 129, w, p); }

extern "C" int vadx_silero_pack_host_sr(int sample_rate, const vadx_silero_weights_host *w, float *p) {
    if (sample_rate == 16000) return vadx_silero_pack_host(w, p);
    VADX_REQUIRE(sample_rate == 8000, "vadx_silero_pack_host_sr: sample_rate=%d is not 16000 or 8000", sample_rate);
    return pack_blob("vadx_silero_pack_host_sr", 65, w, p);
}
