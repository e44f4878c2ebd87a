// silero_stream.hip -- streaming Silero: S live streams advance by k windows per call, every stream's context, LSTM state and VADIterator
// machine held in a device record (include/vadx.h: vadx_silero_stream_run).  One tick = four stream-ordered launches:
//   silero_stream_stage_kernel<SampleT, CW, WW>: staged f32 rows [context(64) | k*512 samples] (32 | k*256 at 8 kHz) in the workspace, the initial LSTM state (zeros for a
//       reset stream), NaN pre-filled into probs and state_out's h/c (a launch that writes nothing leaves NaN, never stale numbers);
//   the tuned encoder over the staged rows (origin 0, as vadx_silero_step runs it) and the recurrent launch, unchanged (csrc/silero.hip);
//   silero_stream_iter_kernel: VADIterator's machine (utils_vad.py:535-586), one stream per thread, then the record's context.
// Staging the context in front of the new samples is what makes a tick's scores bit for bit those of vadx_silero_clips over the
// concatenated audio: window t of a staged row is the same 576 samples, and an encoder window's result does not depend on the tile slot
// that takes it.
#include "silero_common.h"

#include <math.h>

namespace vadx {
namespace silero {

constexpr int CTX = 64, WIN = 512;
constexpr int MAX_WINDOWS = 1 << 16;      // windows per tick (the staging grid's y extent stays below 65536)

// ---- the record (vadx_silero_stream_state_bytes): structure of arrays, every field zero in the reset state ----------------------------
//   [2][S][128] f32  LSTM h, c (the documented part)      [S][64] f32  context: the last 64 samples the stream was fed
//   [S] i64  current_sample    [S] i64  temp_end    [S] i32  triggered
struct StreamRecord {
    float *hc, *ctx;
    long long *cur, *temp_end;
    int *trig;
};
__host__ __device__ inline size_t record_bytes(long long S) { return ((size_t)S * (2 * 128 + CTX) * 4 + (size_t)S * 20 + 15) & ~(size_t)15; }
__host__ __device__ inline StreamRecord record_at(void *base, long long S) {
    char *p = static_cast<char *>(base);
    StreamRecord r;
    r.hc = reinterpret_cast<float *>(p);
    r.ctx = r.hc + S * 2 * 128;
    r.cur = reinterpret_cast<long long *>(r.ctx + S * CTX);       // S * 1280 B from the base: 8-byte aligned
    r.temp_end = r.cur + S;
    r.trig = reinterpret_cast<int *>(r.temp_end + S);
    return r;
}

// ---- workspace: staged rows [S][64 + k*512] f32 | state0 [2][S][128] f32 | gx (vadx_silero_workspace_bytes(S, k)), 256-B aligned each
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t staged_bytes(long long S, int k) { return align256((size_t)S * (CTX + (size_t)k * WIN) * 4); }
inline size_t state0_bytes(long long S) { return align256((size_t)S * 2 * 128 * 4); }

constexpr int STAGE_THREADS = 256, STAGE_PER_BLOCK = 4 * STAGE_THREADS;      // floats of one staged row per block

// CW / WW: the network's context and window (64 / 512 at 16 kHz, 32 / 256 at 8 kHz); the record keeps CTX floats of context per stream
// either way (an 8 kHz stream uses the first 32)
template <typename SampleT, int CW, int WW>
__global__ __launch_bounds__(STAGE_THREADS) void silero_stream_stage_kernel(
    const SampleT *__restrict__ samples, float scale, long long row_stride, int S, int k, const unsigned char *__restrict__ reset,
    const unsigned char *__restrict__ active, const float *__restrict__ hc_in, const float *__restrict__ ctx_in, float *__restrict__ hc_out,
    float *__restrict__ staged, float *__restrict__ state0, float *__restrict__ probs) {
    const long long s = blockIdx.x;
    const int tid = threadIdx.x;
    const bool act = active == nullptr || active[s] != 0;
    const bool fresh = !act || (reset != nullptr && reset[s] != 0);     // inactive rows run on zeros: their results are discarded, and
    const long long L = CW + (long long)k * WW;                        // garbage there must not raise the fp16 range flag
    float *row = staged + s * L;
    const long long i0 = (long long)blockIdx.y * STAGE_PER_BLOCK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = i0 + tid + j * STAGE_THREADS;
        if (i >= L) break;
        float v = 0.f;
        if (i < CW) {
            if (!fresh) v = ctx_in[s * CTX + i];
        } else if (act) {
            v = SampleIO<SampleT>::load1(samples + s * row_stride + (i - CW), scale);
        }
        row[i] = v;
    }
    if (blockIdx.y != 0) return;
    for (int u = tid; u < 2 * 128; u += STAGE_THREADS) {            // u = 128 * (h | c) + unit
        const long long off = ((long long)(u >> 7) * S + s) * 128 + (u & 127);
        state0[off] = fresh ? 0.f : hc_in[off];
        hc_out[off] = __builtin_nanf("");
    }
    for (int t = tid; t < k; t += STAGE_THREADS) probs[s * k + t] = __builtin_nanf("");
}

// One stream per thread (the machine diverges per stream; 64 streams per wave), then the block's streams' context / record copies with
// every lane on one stream's row at a time.
constexpr int ITER_THREADS = 64;
struct IterConsts {
    double thr, neg, pad, min_sil;
};

template <int CW, int WW>
__global__ __launch_bounds__(ITER_THREADS) void silero_stream_iter_kernel(
    IterConsts q, int S, int k, const unsigned char *__restrict__ reset, const unsigned char *__restrict__ active, StreamRecord in,
    StreamRecord out, const float *__restrict__ staged, float *__restrict__ probs, signed char *__restrict__ kind,
    double *__restrict__ value) {
    __shared__ unsigned char what[ITER_THREADS];           // 0 active, 1 active and poisoned this tick, 2 inactive
    const int tid = threadIdx.x;
    const long long s0 = (long long)blockIdx.x * ITER_THREADS;
    const long long s = s0 + tid;
    if (s < S) {
        const bool act = active == nullptr || active[s] != 0;
        signed char *ks = kind + s * k;
        double *vs = value + s * k;
        if (!act) {
            for (int t = 0; t < k; ++t) { ks[t] = 0; vs[t] = 0.0; probs[s * k + t] = __builtin_nanf(""); }
            out.cur[s] = in.cur[s];
            out.temp_end[s] = in.temp_end[s];
            out.trig[s] = in.trig[s];
            what[tid] = 2;
        } else {
            const bool fresh = reset != nullptr && reset[s] != 0;
            long long cur = fresh ? 0 : in.cur[s], temp_end = fresh ? 0 : in.temp_end[s];
            bool trig = fresh ? false : in.trig[s] != 0, poison = false;
            // VADIterator.__call__ (utils_vad.py:561-585) per window of W = 512 samples, in double, each expression left to right as the
            // Python evaluates it.  `neg` is literally threshold - 0.15 (VADIterator has no max(., 0.01)).
            for (int t = 0; t < k; ++t) {
                const float p = probs[s * k + t];
                signed char e = 0;
                double v = 0.0;
                cur += WW;
                if (!isfinite(p)) {                // NaN score: "invalid", and the stream stays so until reset (its h is poisoned below)
                    e = -1;
                    poison = true;
                } else if ((double)p >= q.thr) {
                    if (temp_end) temp_end = 0;
                    if (!trig) {
                        trig = true;
                        e = 1;
                        const double x = ((double)cur - q.pad) - (double)WW;
                        v = x > 0.0 ? x : 0.0;                   // max(0, x): the int 0 unless x is larger
                    }
                } else if ((double)p < q.neg && trig) {
                    if (!temp_end) temp_end = cur;
                    if ((double)(cur - temp_end) >= q.min_sil) {
                        e = 2;
                        v = ((double)temp_end + q.pad) - (double)WW;
                        temp_end = 0;
                        trig = false;
                    }
                }
                ks[t] = e;
                vs[t] = v;
            }
            out.cur[s] = cur;
            out.temp_end[s] = temp_end;
            out.trig[s] = trig ? 1 : 0;
            what[tid] = poison ? 1 : 0;
        }
    }
    __syncthreads();
    const long long L = CW + (long long)k * WW;
    const int n = S - s0 < ITER_THREADS ? (int)(S - s0) : ITER_THREADS;
    for (int i = 0; i < n; ++i) {
        const long long r = s0 + i;
        const unsigned char w = what[i];
        out.ctx[r * CTX + tid] = w == 2 ? in.ctx[r * CTX + tid] : (tid < CW ? staged[r * L + L - CW + tid] : 0.f);
        if (w == 2) {
            for (int u = tid; u < 2 * 128; u += ITER_THREADS) {
                const long long off = ((long long)(u >> 7) * S + r) * 128 + (u & 127);
                out.hc[off] = in.hc[off];
            }
        } else if (w == 1) {
            for (int u = tid; u < 128; u += ITER_THREADS) out.hc[r * 128 + u] = __builtin_nanf("");
        }
    }
}

}  // namespace silero
}  // namespace vadx

using namespace vadx::silero;

extern "C" size_t vadx_silero_stream_state_bytes(int streams) { return streams > 0 ? record_bytes(streams) : 0; }

extern "C" size_t vadx_silero_stream_workspace_bytes(int streams, int windows) {
    if (streams <= 0 || windows <= 0 || windows > MAX_WINDOWS) return 0;
    return staged_bytes(streams, windows) + state0_bytes(streams) + align256(vadx_silero_workspace_bytes(streams, windows));
}

extern "C" int vadx_silero_stream_run(const float *packed, const vadx_silero_iter_params *prm, const void *samples, int samples_int16,
                                      float scale, int64_t row_stride, int streams, int windows, const uint8_t *reset,
                                      const uint8_t *active, const void *state_in, void *state_out, float *probs, int8_t *event_kind,
                                      double *event_value, void *workspace, size_t workspace_bytes, void *stream,
                                      const vadx_silero_cfg *cfg) {
    VADX_REQUIRE(packed && prm && samples && state_in && state_out && probs && event_kind && event_value && workspace,
                 "vadx_silero_stream_run: NULL pointer argument");
    const int rate = (cfg == nullptr || cfg->ext.sample_rate == 0) ? 16000 : cfg->ext.sample_rate;
    VADX_REQUIRE(rate == 16000 || rate == 8000, "vadx_silero_stream_run: cfg->ext.sample_rate=%d is not 16000 or 8000 (0 = 16000)", rate);
    VADX_REQUIRE(prm->sampling_rate == rate,
                 "sr=%d: the cfg selects the %d kHz sub-graph of the Silero network (vadx_silero_cfg.ext.sample_rate and the blob must be "
                 "packed for the same rate)", (int)prm->sampling_rate, rate / 1000);
    const int win = rate == 8000 ? 256 : WIN, cw = win / 8;
    VADX_REQUIRE(streams > 0 && windows > 0 && windows <= MAX_WINDOWS, "vadx_silero_stream_run: streams=%d windows=%d", streams, windows);
    VADX_REQUIRE(row_stride >= (int64_t)windows * win, "vadx_silero_stream_run: row_stride=%lld < windows * %d = %lld",
                 (long long)row_stride, win, (long long)windows * win);
    const int a = cfg ? cfg->arithmetic : VADX_ARITH_AUTO;
    VADX_REQUIRE(a >= VADX_ARITH_AUTO && a <= VADX_ARITH_F16X2, "vadx_silero_stream_run: cfg->arithmetic=%d is not one of VADX_ARITH_*", a);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, record_bytes(streams)), "vadx_silero_stream_run: state_in and state_out overlap");
    const size_t need = vadx_silero_stream_workspace_bytes(streams, windows);
    if (workspace_bytes < need) {
        vadx::set_error("vadx_silero_stream_run: workspace %zu B < required %zu B", workspace_bytes, need);
        return VADX_ENOSPACE;
    }
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) &
                  15) == 0, "vadx_silero_stream_run: workspace and records must be 16-byte aligned");

    char *ws = static_cast<char *>(workspace);
    float *staged = reinterpret_cast<float *>(ws);
    float *state0 = reinterpret_cast<float *>(ws + staged_bytes(streams, windows));
    char *gx = ws + staged_bytes(streams, windows) + state0_bytes(streams);
    const size_t gx_bytes = workspace_bytes - (size_t)(gx - ws);
    const StreamRecord rin = record_at(const_cast<void *>(state_in), streams), rout = record_at(state_out, streams);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long L = cw + (long long)windows * win;      // (the workspace is laid out for the 16 kHz geometry, an upper bound)

    const dim3 sgrid((unsigned)streams, (unsigned)((L + STAGE_PER_BLOCK - 1) / STAGE_PER_BLOCK));
    if (win == 256) {
        if (samples_int16)
            hipLaunchKernelGGL((silero_stream_stage_kernel<int16_t, 32, 256>), sgrid, dim3(STAGE_THREADS), 0, st,
                               static_cast<const int16_t *>(samples), scale, (long long)row_stride, streams, windows, reset, active, rin.hc,
                               rin.ctx, rout.hc, staged, state0, probs);
        else
            hipLaunchKernelGGL((silero_stream_stage_kernel<float, 32, 256>), sgrid, dim3(STAGE_THREADS), 0, st,
                               static_cast<const float *>(samples), 1.0f, (long long)row_stride, streams, windows, reset, active, rin.hc,
                               rin.ctx, rout.hc, staged, state0, probs);
    } else {
        if (samples_int16)
            hipLaunchKernelGGL((silero_stream_stage_kernel<int16_t, CTX, WIN>), sgrid, dim3(STAGE_THREADS), 0, st,
                               static_cast<const int16_t *>(samples), scale, (long long)row_stride, streams, windows, reset, active, rin.hc,
                               rin.ctx, rout.hc, staged, state0, probs);
        else
            hipLaunchKernelGGL((silero_stream_stage_kernel<float, CTX, WIN>), sgrid, dim3(STAGE_THREADS), 0, st,
                               static_cast<const float *>(samples), 1.0f, (long long)row_stride, streams, windows, reset, active, rin.hc,
                               rin.ctx, rout.hc, staged, state0, probs);
    }
    VADX_HIP_TRY(hipGetLastError());

    int rc = silero_encode_launch<float>(packed, staged, 1.0f, L, L, 0, streams, windows, gx, gx_bytes, stream, cfg);
    if (rc != VADX_OK) return rc;
    rc = silero_recur_launch(packed, gx, gx_bytes, streams, windows, state0, probs, windows, rout.hc, stream, cfg);
    if (rc != VADX_OK) return rc;

    IterConsts q;
    const double sr = (double)prm->sampling_rate;
    q.thr = prm->threshold;
    q.neg = prm->threshold - 0.15;
    q.pad = sr * prm->speech_pad_ms / 1000.0;
    q.min_sil = sr * prm->min_silence_duration_ms / 1000.0;
    const dim3 igrid((unsigned)((streams + ITER_THREADS - 1) / ITER_THREADS));
    if (win == 256)
        hipLaunchKernelGGL((silero_stream_iter_kernel<32, 256>), igrid, dim3(ITER_THREADS), 0, st, q, streams, windows, reset, active, rin,
                           rout, staged, probs, reinterpret_cast<signed char *>(event_kind), event_value);
    else
        hipLaunchKernelGGL((silero_stream_iter_kernel<CTX, WIN>), igrid, dim3(ITER_THREADS), 0, st, q, streams, windows, reset, active, rin,
                           rout, staged, probs, reinterpret_cast<signed char *>(event_kind), event_value);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
