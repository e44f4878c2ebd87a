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

// VADIterator.__call__ (utils_vad.py:561-585) for one window of WW samples with score p, in double, each expression left to right as the
// Python evaluates it -> the window's event (e, v).  `neg` is literally threshold - 0.15 (VADIterator has no max(., 0.01)).  Shared by the
// rectangular and the ragged tick: one machine.
template <int WW>
__device__ __forceinline__ void iter_step(const IterConsts &q, float p, long long &cur, long long &temp_end, bool &trig, bool &poison,
                                          signed char &e_out, double &v_out) {
    signed char e = 0;
    double v = 0.0;
    cur += WW;
    if (!isfinite(p)) {                // NaN score: "invalid", and the stream stays so until reset (its h is poisoned by the caller)
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
    e_out = e;
    v_out = v;
}

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
            for (int t = 0; t < k; ++t) iter_step<WW>(q, probs[s * k + t], cur, temp_end, trig, poison, ks[t], vs[t]);
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

// ---- ragged ticks (include/vadx.h: vadx_silero_stream_run_ragged): stream s delivers n_s windows, 0 <= n_s <= max_windows ------------------
// A tick is a ragged batch (silero_common.h) over the staged rows [context | n_s windows] of the streams with n_s > 0: origin 0, the record's
// h / c as state0, clips = S.  The per-stream tables come from the device planner below; n_s is read from probs_first everywhere.
constexpr int RAGGED_MAX_WINDOWS = 256;
constexpr int PLAN_THREADS = 1024, PLAN_WAVES = PLAN_THREADS / 64, PLAN_KEYS = RAGGED_MAX_WINDOWS + 1;

// plan scratch: block_sum i64 [blocks] | key histograms i32 [blocks][max_windows + 1] (turned into their exclusive prefix over the blocks)
inline long long plan_blocks(long long S) { return (S + PLAN_THREADS - 1) / PLAN_THREADS; }
inline size_t plan_bytes(long long S, int mw) { return align256((size_t)plan_blocks(S) * (8 + (size_t)(mw + 1) * 4)); }

// The counting sort's block step, the same in both planner kernels: this thread's stream s = block * 1024 + tid has key n_s (0 for a stream
// behind S or a count outside [0, mw]: `bad`); rank = streams of the same key before it in its WAVE (nine ballots: the lanes that agree in
// every key bit); wh [16][K] = every wave's key histogram, written by each key's first lane -- no atomic, nothing depends on arrival order.
__device__ __forceinline__ void plan_block(const int *__restrict__ counts, long long S, int mw, int K, int *wh, int &key, int &rank,
                                           bool &valid, bool &bad) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = (long long)blockIdx.x * PLAN_THREADS + tid;
    for (int i = tid; i < PLAN_WAVES * K; i += PLAN_THREADS) wh[i] = 0;
    __syncthreads();
    valid = s < S;
    const int c = valid ? counts[s] : 0;
    bad = (unsigned)c > (unsigned)mw;
    key = bad ? 0 : c;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 9; ++bit) {
        const bool on = (key >> bit) & 1;
        const unsigned long long b = __ballot(on);
        same &= on ? b : ~b;
    }
    rank = __popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wh[wave * K + key] = __popcll(same);
    __syncthreads();
}

// pass 1: per block the key histogram and the sum of its counts
__global__ __launch_bounds__(PLAN_THREADS) void silero_stream_plan_hist_kernel(const int *__restrict__ counts, int S, int mw,
                                                                               long long *__restrict__ block_sum, int *__restrict__ block_hist) {
    __shared__ int wh[PLAN_WAVES * PLAN_KEYS];
    __shared__ int total;
    const int K = mw + 1, tid = threadIdx.x;
    int key, rank;
    bool valid, bad;
    if (tid == 0) total = 0;
    plan_block(counts, S, mw, K, wh, key, rank, valid, bad);
    if (tid < K) {
        int h = 0;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) h += wh[w * K + tid];
        block_hist[(long long)blockIdx.x * K + tid] = h;
        atomicAdd(&total, h * tid);              // an integer sum: the same whatever the order
    }
    __syncthreads();
    if (tid == 0) block_sum[blockIdx.x] = total;
}

// pass 2: exclusive prefix over the blocks, per key (one thread each) and of the block sums (thread K)
__global__ __launch_bounds__(320) void silero_stream_plan_scan_kernel(int blocks, int mw, long long *__restrict__ block_sum,
                                                                      int *__restrict__ block_hist) {
    const int K = mw + 1, tid = threadIdx.x;
    if (tid < K) {
        int run = 0;
        for (int b = 0; b < blocks; ++b) {
            const int h = block_hist[(long long)b * K + tid];
            block_hist[(long long)b * K + tid] = run;
            run += h;
        }
    } else if (tid == K) {
        long long run = 0;
        for (int b = 0; b < blocks; ++b) {
            const long long h = block_sum[b];
            block_sum[b] = run;
            run += h;
        }
    }
}

// pass 3: stream s with n_s > 0 goes to slot bucket_first[n_s] + (streams of the same count before it) -- descending by count, stable; the
// slots behind the last active stream are emptied; probs_first = exclusive prefix of the counts in stream order.  A position outside the
// 16 * groups slots (tables that contradict the counts) is not written and raises bit 1 of *status, as a count outside [0, mw] does.
__global__ __launch_bounds__(PLAN_THREADS) void silero_stream_plan_scatter_kernel(
    const int *__restrict__ counts, const int *__restrict__ bucket_first, int S, int mw, int win, int groups,
    const long long *__restrict__ block_sum, const int *__restrict__ block_hist, long long *__restrict__ probs_first,
    long long *__restrict__ slot_off, int *__restrict__ slot_len, int *__restrict__ slot_clip, unsigned *__restrict__ status) {
    __shared__ int wh[PLAN_WAVES * PLAN_KEYS];
    __shared__ int wsum[PLAN_WAVES];
    const int K = mw + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long s = (long long)blockIdx.x * PLAN_THREADS + tid;
    const long long slots = 16LL * groups;
    const int cw = win / 8;
    int key, rank;
    bool valid, bad;
    plan_block(counts, S, mw, K, wh, key, rank, valid, bad);
    if (bad && valid) atomicOr(status, 2u);
    if (valid && key > 0) {
        int before = rank;
        for (int w = 0; w < wave; ++w) before += wh[w * K + key];
        const long long pos = (long long)bucket_first[key] + block_hist[(long long)blockIdx.x * K + key] + before;
        if (pos >= 0 && pos < slots) {
            slot_clip[pos] = (int)s;
            slot_off[pos] = s * (cw + (long long)mw * win);
            slot_len[pos] = cw + key * win;
        } else {
            atomicOr(status, 2u);
        }
    }
    {   // the empty slots [active, 16 groups): fewer than sixteen when the tables agree
        const long long e = (long long)bucket_first[0] + s;
        if (bucket_first[0] >= 0 && e < slots) {
            slot_clip[e] = -1;
            slot_off[e] = 0;
            slot_len[e] = 0;
        }
    }
    // exclusive prefix of the keys in stream order: wave scan, wave totals, block base
    int incl = key;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    long long base = block_sum[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wsum[w];
    if (valid) {
        probs_first[s] = base + incl - key;
        if (s == S - 1) probs_first[S] = base + incl;
    }
}

// n_s as every kernel of the tick takes it: from probs_first, held to [0, mw] (a row has room for mw windows)
__device__ __forceinline__ int ragged_count(const long long *__restrict__ probs_first, long long s, int mw) {
    const long long n = probs_first[s + 1] - probs_first[s];
    return n < 0 ? 0 : (n > mw ? mw : (int)n);
}

// silero_stream_stage_kernel for a ragged tick: of a stream with n_s > 0 the cw + n_s * win floats of its row (row length L = cw + mw * win),
// its state0, NaN into its n_s scores and its h / c of state_out; nothing at all for an idle stream.
template <typename SampleT, int CW, int WW>
__global__ __launch_bounds__(STAGE_THREADS) void silero_stream_stage_ragged_kernel(
    const SampleT *__restrict__ samples, float scale, long long row_stride, int S, int mw, const long long *__restrict__ probs_first,
    const unsigned char *__restrict__ reset, const float *__restrict__ hc_in, const float *__restrict__ ctx_in, float *__restrict__ hc_out,
    float *__restrict__ staged, float *__restrict__ state0, float *__restrict__ probs) {
    const long long s = blockIdx.x;
    const int tid = threadIdx.x;
    const int n = ragged_count(probs_first, s, mw);
    if (n == 0) return;
    const bool fresh = reset != nullptr && reset[s] != 0;
    const long long L = CW + (long long)mw * WW, len = CW + (long long)n * WW;
    float *row = staged + s * L;
    const long long i0 = (long long)blockIdx.y * STAGE_PER_BLOCK;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long i = i0 + tid + j * STAGE_THREADS;
        if (i >= len) break;
        float v;
        if (i < CW) v = fresh ? 0.f : ctx_in[s * CTX + i];
        else v = SampleIO<SampleT>::load1(samples + s * row_stride + (i - CW), scale);
        row[i] = v;
    }
    if (blockIdx.y != 0) return;
    for (int u = tid; u < 2 * 128; u += STAGE_THREADS) {            // u = 128 * (h | c) + unit
        const long long off = ((long long)(u >> 7) * S + s) * 128 + (u & 127);
        state0[off] = fresh ? 0.f : hc_in[off];
        hc_out[off] = __builtin_nanf("");
    }
    float *prow = probs + probs_first[s];
    for (int t = tid; t < n; t += STAGE_THREADS) prow[t] = __builtin_nanf("");
}

// silero_stream_iter_kernel for a ragged tick: n_s steps of the same machine (iter_step) over the stream's packed scores; the new context is
// the last CW samples of the stream's OWN n_s windows; an idle stream's record is copied bit for bit.
template <int CW, int WW>
__global__ __launch_bounds__(ITER_THREADS) void silero_stream_iter_ragged_kernel(
    IterConsts q, int S, int mw, const long long *__restrict__ probs_first, const unsigned char *__restrict__ reset, StreamRecord in,
    StreamRecord out, const float *__restrict__ staged, const float *__restrict__ probs, signed char *__restrict__ kind,
    double *__restrict__ value) {
    __shared__ unsigned char what[ITER_THREADS];           // 0 active, 1 active and poisoned this tick, 2 idle
    __shared__ int cnt[ITER_THREADS];
    const int tid = threadIdx.x;
    const long long s0 = (long long)blockIdx.x * ITER_THREADS;
    const long long s = s0 + tid;
    if (s < S) {
        const int n = ragged_count(probs_first, s, mw);
        cnt[tid] = n;
        if (n == 0) {
            out.cur[s] = in.cur[s];
            out.temp_end[s] = in.temp_end[s];
            out.trig[s] = in.trig[s];
            what[tid] = 2;
        } else {
            const long long first = probs_first[s];
            const bool fresh = reset != nullptr && reset[s] != 0;
            long long cur = fresh ? 0 : in.cur[s], temp_end = fresh ? 0 : in.temp_end[s];
            bool trig = fresh ? false : in.trig[s] != 0, poison = false;
            for (int t = 0; t < n; ++t) iter_step<WW>(q, probs[first + t], cur, temp_end, trig, poison, kind[first + t], value[first + t]);
            out.cur[s] = cur;
            out.temp_end[s] = temp_end;
            out.trig[s] = trig ? 1 : 0;
            what[tid] = poison ? 1 : 0;
        }
    }
    __syncthreads();
    const long long L = CW + (long long)mw * WW;
    const int m = S - s0 < ITER_THREADS ? (int)(S - s0) : ITER_THREADS;
    for (int i = 0; i < m; ++i) {
        const long long r = s0 + i;
        const unsigned char w = what[i];
        out.ctx[r * CTX + tid] = w == 2 ? in.ctx[r * CTX + tid] : (tid < CW ? staged[r * L + (long long)cnt[i] * WW + tid] : 0.f);
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

// ---- ragged ticks: the planner and the tick ----------------------------------------------------------------------------------------------
extern "C" int vadx_silero_stream_ragged_max_windows(void) { return RAGGED_MAX_WINDOWS; }

extern "C" size_t vadx_silero_stream_plan_bytes(int streams, int max_windows) {
    if (streams <= 0 || max_windows <= 0 || max_windows > RAGGED_MAX_WINDOWS) return 0;
    return plan_bytes(streams, max_windows);
}

// plan scratch | staged rows [S][64 + max_windows * 512] f32 | state0 [2][S][128] f32 | gx, tiles x 32 KB
extern "C" size_t vadx_silero_stream_ragged_workspace_bytes(int streams, int max_windows, int64_t tiles) {
    if (streams <= 0 || max_windows <= 0 || max_windows > RAGGED_MAX_WINDOWS || tiles <= 0) return 0;
    return plan_bytes(streams, max_windows) + staged_bytes(streams, max_windows) + state0_bytes(streams) +
           align256(vadx_silero_ragged_workspace_bytes(tiles));
}

extern "C" int vadx_silero_stream_plan(const int32_t *counts, const int32_t *bucket_first, int streams, int max_windows, int window,
                                       int groups, int64_t *probs_first, int64_t *slot_off, int32_t *slot_len, int32_t *slot_clip,
                                       uint32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    VADX_REQUIRE(counts && bucket_first && probs_first && slot_off && slot_len && slot_clip && status && workspace,
                 "vadx_silero_stream_plan: NULL pointer argument");
    VADX_REQUIRE(streams > 0 && max_windows > 0 && max_windows <= RAGGED_MAX_WINDOWS,
                 "vadx_silero_stream_plan: streams=%d max_windows=%d (1 .. %d: vadx_silero_stream_ragged_max_windows)", streams, max_windows,
                 RAGGED_MAX_WINDOWS);
    VADX_REQUIRE(window == 512 || window == 256, "vadx_silero_stream_plan: window=%d is not 512 (16 kHz) or 256 (8 kHz)", window);
    VADX_REQUIRE(groups >= 1 && groups <= (streams + 15) / 16, "vadx_silero_stream_plan: groups=%d for %d streams", groups, streams);
    if (workspace_bytes < plan_bytes(streams, max_windows)) {
        vadx::set_error("vadx_silero_stream_plan: workspace %zu B < required %zu B", workspace_bytes, plan_bytes(streams, max_windows));
        return VADX_ENOSPACE;
    }
    VADX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "vadx_silero_stream_plan: workspace must be 16-byte aligned");
    const int blocks = (int)plan_blocks(streams);
    long long *block_sum = static_cast<long long *>(workspace);
    int *block_hist = reinterpret_cast<int *>(block_sum + blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(silero_stream_plan_hist_kernel, dim3(blocks), dim3(PLAN_THREADS), 0, st, counts, streams, max_windows, block_sum,
                       block_hist);
    hipLaunchKernelGGL(silero_stream_plan_scan_kernel, dim3(1), dim3(320), 0, st, blocks, max_windows, block_sum, block_hist);
    hipLaunchKernelGGL(silero_stream_plan_scatter_kernel, dim3(blocks), dim3(PLAN_THREADS), 0, st, counts, bucket_first, streams, max_windows,
                       window, groups, block_sum, block_hist, reinterpret_cast<long long *>(probs_first),
                       reinterpret_cast<long long *>(slot_off), slot_len, slot_clip, status);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

template <typename SampleT, int CW, int WW>
static void stage_ragged_launch(dim3 grid, hipStream_t st, const void *samples, float scale, long long row_stride, int S, int mw,
                                const long long *probs_first, const uint8_t *reset, const StreamRecord &rin, const StreamRecord &rout,
                                float *staged, float *state0, float *probs) {
    hipLaunchKernelGGL((silero_stream_stage_ragged_kernel<SampleT, CW, WW>), grid, dim3(STAGE_THREADS), 0, st,
                       static_cast<const SampleT *>(samples), scale, row_stride, S, mw, probs_first, reset, rin.hc, rin.ctx, rout.hc, staged,
                       state0, probs);
}

extern "C" int vadx_silero_stream_run_ragged(const float *packed, const vadx_silero_iter_params *prm, const void *samples, int samples_int16,
                                             float scale, int64_t row_stride, int streams, int max_windows, const vadx_silero_ragged *rg,
                                             const uint8_t *reset, const void *state_in, void *state_out, float *probs, int8_t *event_kind,
                                             double *event_value, void *workspace, size_t workspace_bytes, void *stream,
                                             const vadx_silero_cfg *cfg) {
    const char *who = "vadx_silero_stream_run_ragged";
    VADX_REQUIRE(packed && prm && samples && rg && state_in && state_out && probs && event_kind && event_value && workspace,
                 "%s: NULL pointer argument", who);
    VADX_REQUIRE(rg->slot_off && rg->slot_len && rg->slot_clip && rg->gx_first && rg->grp_min_len && rg->wg_tab && rg->probs_first && rg->status,
                 "%s: NULL table in vadx_silero_ragged", who);
    const int rate = (cfg == nullptr || cfg->ext.sample_rate == 0) ? 16000 : cfg->ext.sample_rate;
    VADX_REQUIRE(rate == 16000 || rate == 8000, "%s: cfg->ext.sample_rate=%d is not 16000 or 8000 (0 = 16000)", who, rate);
    VADX_REQUIRE(prm->sampling_rate == rate,
                 "sr=%d: the cfg selects the %d kHz sub-graph of the Silero network (vadx_silero_cfg.ext.sample_rate and the blob must be "
                 "packed for the same rate)", (int)prm->sampling_rate, rate / 1000);
    const int win = rate == 8000 ? 256 : WIN, cw = win / 8;
    VADX_REQUIRE(streams > 0 && max_windows > 0 && max_windows <= RAGGED_MAX_WINDOWS,
                 "%s: streams=%d max_windows=%d (1 .. %d: vadx_silero_stream_ragged_max_windows)", who, streams, max_windows, RAGGED_MAX_WINDOWS);
    VADX_REQUIRE(row_stride >= (int64_t)max_windows * win, "%s: row_stride=%lld < max_windows * %d = %lld", who, (long long)row_stride, win,
                 (long long)max_windows * win);
    VADX_REQUIRE(rg->clips == streams && rg->groups >= 1 && rg->groups <= (streams + 15) / 16 && rg->tiles >= rg->groups &&
                     (long long)rg->tiles <= (long long)rg->groups * max_windows && rg->n_runs >= rg->groups &&
                     (long long)rg->n_runs * RG_RUN < (1LL << 31) && (long long)rg->n_runs * RG_RUN >= rg->tiles,
                 "%s: clips=%d groups=%d n_runs=%d tiles=%d are not the counts of one tick of %d streams x at most %d windows", who, rg->clips,
                 rg->groups, rg->n_runs, rg->tiles, streams, max_windows);
    const int a = cfg ? cfg->arithmetic : VADX_ARITH_AUTO;
    VADX_REQUIRE(a >= VADX_ARITH_AUTO && a <= VADX_ARITH_F16X2, "%s: cfg->arithmetic=%d is not one of VADX_ARITH_*", who, a);
    VADX_REQUIRE(!vadx::records_overlap(state_in, state_out, record_bytes(streams)), "%s: state_in and state_out overlap", who);
    const size_t need = vadx_silero_stream_ragged_workspace_bytes(streams, max_windows, rg->tiles);
    if (workspace_bytes < need) {
        vadx::set_error("%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
        return VADX_ENOSPACE;
    }
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out) |
                   reinterpret_cast<uintptr_t>(packed)) & 15) == 0, "%s: packed weights, workspace and records must be 16-byte aligned", who);

    char *ws = static_cast<char *>(workspace) + plan_bytes(streams, max_windows);
    float *staged = reinterpret_cast<float *>(ws);
    float *state0 = reinterpret_cast<float *>(ws + staged_bytes(streams, max_windows));
    float *gx = reinterpret_cast<float *>(ws + staged_bytes(streams, max_windows) + state0_bytes(streams));
    const StreamRecord rin = record_at(const_cast<void *>(state_in), streams), rout = record_at(state_out, streams);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long L = cw + (long long)max_windows * win;      // (the workspace is laid out for the 16 kHz geometry, an upper bound)
    const long long *first = reinterpret_cast<const long long *>(rg->probs_first);

    const dim3 sgrid((unsigned)streams, (unsigned)((L + STAGE_PER_BLOCK - 1) / STAGE_PER_BLOCK));
    if (win == 256) {
        if (samples_int16) stage_ragged_launch<int16_t, 32, 256>(sgrid, st, samples, scale, row_stride, streams, max_windows, first, reset, rin, rout, staged, state0, probs);
        else stage_ragged_launch<float, 32, 256>(sgrid, st, samples, 1.0f, row_stride, streams, max_windows, first, reset, rin, rout, staged, state0, probs);
    } else {
        if (samples_int16) stage_ragged_launch<int16_t, CTX, WIN>(sgrid, st, samples, scale, row_stride, streams, max_windows, first, reset, rin, rout, staged, state0, probs);
        else stage_ragged_launch<float, CTX, WIN>(sgrid, st, samples, 1.0f, row_stride, streams, max_windows, first, reset, rin, rout, staged, state0, probs);
    }
    VADX_HIP_TRY(hipGetLastError());

    RgArg<true> arg;
    arg.t = *rg;
    arg.n_src = (long long)streams * L;
    int rc = silero_encode_ragged_launch<float>(rate, cfg, packed, staged, 1.0f, arg, gx, stream, 0LL);
    if (rc != VADX_OK) return rc;
    rc = silero_recur_ragged_launch(cfg, packed, gx, arg, probs, rout.hc, stream, state0);
    if (rc != VADX_OK) return rc;

    IterConsts q;
    const double sr = (double)prm->sampling_rate;
    q.thr = prm->threshold;
    q.neg = prm->threshold - 0.15;
    q.pad = sr * prm->speech_pad_ms / 1000.0;
    q.min_sil = sr * prm->min_silence_duration_ms / 1000.0;
    const dim3 igrid((unsigned)((streams + ITER_THREADS - 1) / ITER_THREADS));
    if (win == 256)
        hipLaunchKernelGGL((silero_stream_iter_ragged_kernel<32, 256>), igrid, dim3(ITER_THREADS), 0, st, q, streams, max_windows, first, reset,
                           rin, rout, staged, probs, reinterpret_cast<signed char *>(event_kind), event_value);
    else
        hipLaunchKernelGGL((silero_stream_iter_ragged_kernel<CTX, WIN>), igrid, dim3(ITER_THREADS), 0, st, q, streams, max_windows, first, reset,
                           rin, rout, staged, probs, reinterpret_cast<signed char *>(event_kind), event_value);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
