// timestamps.hip -- per-frame decisions / segment tables -> timestamps in seconds and in samples, for every clip of a resident batch
// (include/vadx.h, "Timestamps").  The host code this replaces, bit for bit:
//   FLAGS    vad_to_timestamps + process_timestamps (FSMN/Inference_FSMN_VAD_ONNX.py:102-141) over silence flags;
//   FRAMES   the float32 seconds + round(, 3) tail of decision_to_segment (FireRedVAD/Inference_FireRed_ONNX.py:169-179);
//   SAMPLES  round(x / sampling_rate, 1) with its clamps (Silero/modeling_modified/utils_vad.py:478-482).
// One WAVE per clip, four per workgroup: lanes are frames (FLAGS) or table rows, a ballot gives the mask of a step, a popcount of the
// lower lanes a row's slot.  Every kind feeds ONE back half, `Fuse::rows`: the duration filter, the fuse rule, seconds -> sample rows.
//
// Everything here is double arithmetic that Python does one operation at a time, so NOTHING may be contracted: `b * fd + fd` as an FMA
// rounds once where Python rounds twice, and moves an end by an ulp -- across a threshold.  hipcc contracts device code by default and
// its __dmul_rn / __dadd_rn are plain operators here, so contraction is switched off for the whole file; the one fused operation that is
// wanted (the exact residual of round1) is spelled fma().
#pragma clang fp contract(off)
#include "common.h"

namespace vadx {
namespace tstable {

typedef unsigned long long u64;

__device__ __forceinline__ u64 lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int top_bit(u64 m) { return 63 - __clzll((long long)m); }       // m != 0

// One clip's output rows.  `put` writes one number: the seconds as they are, the sample index by the caller's rule --
// NEAREST int(round(s * sr)) (Python's round of a double to an int: half to even = rint), TRUNC int(s * sr).
struct Out {
    double *sec;
    long long *smp;
    int cap, rule;
    double sr;
    __device__ __forceinline__ void put(int idx, int which, double v) const {
        sec[2 * (long long)idx + which] = v;
        const double x = v * sr;
        smp[2 * (long long)idx + which] = rule == VADX_TS_NEAREST ? (long long)rint(x) : (long long)x;
    }
};

// THE back half, once for the three kinds: process_timestamps over rows that arrive 64 at a time, in order.
//   filter   a row is kept when (e - s) >= min_duration;
//   fuse     the reference appends to `merged` or extends merged[-1], whose end is then always the previous KEPT row's end: row k opens
//            a segment exactly when there is no kept row before it or not (s_k - e_prev <= fusion_threshold) -- no serial walk.  Its
//            second pass compares the same s_k and e_prev across every boundary the first pass left, and so changes nothing: one pass.
//   process == 0: every row is kept and opens a segment (the table goes through as it is).
// A segment's ordinal is the number of openers before it.  An opener writes its own start and the END of the segment before it (the
// previous kept row's end, which it holds anyway); `finish` writes the last end.  Carried between steps: the last kept end, whether
// there is one, the openers so far.  Nothing is written at an ordinal >= cap; `opened` goes on counting (the true count).
struct Fuse {
    double last_end;
    int have, opened;
    __device__ __forceinline__ void rows(bool valid, double s, double e, const vadx_ts_params &p, int lane, const Out &o) {
        const bool keep = valid && (!p.process || (e - s) >= p.min_duration);
        const u64 K = __ballot(keep);
        const u64 kb = K & lanes_below(lane);
        const double e_lane = __shfl(e, kb ? top_bit(kb) : 0, 64);
        const double e_prev = kb ? e_lane : last_end;
        const bool has_prev = kb ? true : have != 0;
        const bool opens = keep && (!p.process || !has_prev || !((s - e_prev) <= p.fusion_threshold));
        const u64 O = __ballot(opens);
        if (opens) {
            const int idx = opened + __popcll(O & lanes_below(lane));
            if (idx < o.cap) o.put(idx, 0, s);
            if (idx >= 1 && idx - 1 < o.cap) o.put(idx - 1, 1, e_prev);
        }
        if (K) {                                           // uniform: K is a ballot
            last_end = __shfl(e, top_bit(K), 64);
            have = 1;
        }
        opened += __popcll(O);
    }
    __device__ __forceinline__ void finish(int lane, const Out &o) const {
        if (lane == 0 && opened >= 1 && opened - 1 < o.cap) o.put(opened - 1, 1, last_end);
    }
};

// head: int32 status (VADX_TS_ST_*), int32 largest count, 8 bytes of zeros; zeroed by the entry point before the launch
__device__ __forceinline__ void report(int *head, int32_t *counts, long long b, int lane, int count, int cap, bool refused) {
    if (lane != 0) return;
    counts[b] = refused ? 0 : count;
    if (refused) atomicOr(head, VADX_TS_ST_BAD_CLIP);
    else {
        if (count > cap) atomicOr(head, VADX_TS_ST_OVERFLOW);
        if (count > 0) atomicMax(head + 1, count);
    }
}

struct Outs {
    double *seconds;
    long long *samples;
    int32_t *counts;
    int *head;
    int cap;
};

__device__ __forceinline__ Out out_of(const Outs &o, long long b, const vadx_ts_params &p) {
    return Out{o.seconds + b * 2 * (long long)o.cap, o.samples + b * 2 * (long long)o.cap, o.cap, p.sample_rule, (double)p.sampling_rate};
}

// FLAGS: speech = flag 0 at a position < n (so the 255 filler of a ragged row is silence, as astype(bool) makes it).  The wave walks
// positions 0 .. n INCLUSIVE, 64 at a time, position n being silence: a run that reaches n then ends there like any other.  With m the
// step's speech mask and one carried bit, the edges are m ^ (m << 1 | carry); a falling edge at position b closes the run [a, b) whose
// start a is the last rising edge below it -- in this step, or the carried one.  start = a * fd; end = n * fd when b == n, otherwise
// b * fd + fd (timestamps.vad_to_timestamps).  The runs are never stored: each step's closed runs go straight into the back half.
__global__ __launch_bounds__(256) void flags_kernel(vadx_ts_params p, const uint8_t *__restrict__ flags, long long stride,
                                                    const int32_t *__restrict__ n_flags, int B, Outs o) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long n = n_flags[b];
    if (n < 0 || n > stride) {
        report(o.head, o.counts, b, lane, 0, o.cap, true);
        return;
    }
    const uint8_t *row = flags + b * stride;
    const Out out = out_of(o, b, p);
    const double fd = p.frame_s, end_n = (double)n * fd;
    Fuse f{0.0, 0, 0};
    u64 carry = 0;
    long long open_start = 0;
    for (long long base = 0; base <= n; base += 64) {
        const long long pos = base + lane;
        const u64 m = __ballot(pos < n && row[pos] == 0);
        const u64 edges = m ^ ((m << 1) | carry), rise = edges & m, fall = edges & ~m;
        const bool closes = (fall >> lane) & 1;
        const u64 rb = rise & lanes_below(lane);
        const long long a = rb ? base + top_bit(rb) : open_start;
        const double s = (double)a * fd;
        const double e = pos == n ? end_n : (double)pos * fd + fd;
        f.rows(closes, s, e, p, lane, out);
        if (rise) open_start = base + top_bit(rise);
        carry = m >> 63;
    }
    f.finish(lane, out);
    report(o.head, o.counts, b, lane, f.opened, o.cap, false);
}

// round(x, 3) for a float32-valued x: x * 1000.0 is exact in double (24 + 10 bits), so the nearest integer, ties to even, divided by
// 1000.0 is the correctly rounded decimal Python's round gives.
__device__ __forceinline__ double round3(float x) { return rint((double)x * 1000.0) / 1000.0; }

// FRAMES: VadPostprocessor.segments_to_seconds.  float32 frame * frame_shift; when the LAST row ends at n the end is n * frame_shift
// (+ frame_length), capped by the clip's duration when there is one (NaN: none), stored as float32; then round(, 3).
__global__ __launch_bounds__(256) void frames_kernel(vadx_ts_params p, const int32_t *__restrict__ segs, const int32_t *__restrict__ counts_in,
                                                     int cap_in, const int32_t *__restrict__ n_frames, const double *__restrict__ wav_dur, int B,
                                                     Outs o) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int cnt = counts_in[b], n = n_frames[b];
    if (cnt < 0 || cnt > cap_in || n < 0) {
        report(o.head, o.counts, b, lane, 0, o.cap, true);
        return;
    }
    const int32_t *row = segs + b * 2 * (long long)cap_in;
    const Out out = out_of(o, b, p);
    const double dur = wav_dur[b];
    Fuse f{0.0, 0, 0};
    const int rows = n == 0 ? 0 : cnt;                      // a clip without a frame has no segment
    for (int base = 0; base < rows; base += 64) {
        const int k = base + lane;
        const bool valid = k < rows;
        float s = 0.f, e = 0.f;
        if (valid) {
            const int f0 = row[2 * k], f1 = row[2 * k + 1];
            s = (float)f0 * p.frame_shift;
            e = (float)f1 * p.frame_shift;
            if (k == rows - 1 && f1 == n) {
                float end_t = (float)n * p.frame_shift;
                if (p.use_frame_length) end_t = end_t + p.frame_length;
                if (dur < (double)end_t) end_t = (float)dur;           // false for NaN
                e = end_t;
            }
        }
        f.rows(valid, round3(s), round3(e), p, lane, out);
    }
    f.finish(lane, out);
    report(o.head, o.counts, b, lane, f.opened, o.cap, false);
}

// round(x / sr, 1) for an integer x, sr = 16000 or 8000 (|x| < 2^53).  step = sr / 10 samples are one tenth; (m, r) = divmod(|x|, step).
// Off a tie the quotient's rounding error cannot reach the tie: m + (r > step / 2) tenths.  On a tie Python rounds the DOUBLE q = x / sr,
// which lies above, below or on the decimal tie: the sign of the exact residual q * sr - x says which; on it, the even tenth.
__device__ __forceinline__ double round1(long long x, int sr) {
    const bool neg = x < 0;
    const u64 ax = neg ? 0ull - (u64)x : (u64)x;
    const u64 step = (u64)(sr / 10), half = step / 2;
    const u64 m = ax / step, r = ax - m * step;
    u64 k;
    if (r != half) {
        k = m + (r > half);
    } else {
        const double xd = (double)ax, q = xd / (double)sr;
        const double res = fma(q, (double)sr, -xd);
        k = res > 0.0 ? m + 1 : (res < 0.0 ? m : m + (m & 1));
    }
    const double v = (double)k / 10.0;
    return neg ? -v : v;
}

// SAMPLES: the return_seconds branch of get_speech_timestamps with time_resolution = 1:
// start = max(round1(s), 0), end = min(round1(e), len / sr), Python's max / min (the first argument unless the second is strictly beyond).
__global__ __launch_bounds__(256) void samples_kernel(vadx_ts_params p, const long long *__restrict__ segs, const int32_t *__restrict__ counts_in,
                                                      int cap_in, const long long *__restrict__ clip_len, int B, Outs o) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int cnt = counts_in[b];
    const long long len = clip_len[b];
    if (cnt < 0 || cnt > cap_in || len < 0) {
        report(o.head, o.counts, b, lane, 0, o.cap, true);
        return;
    }
    const long long *row = segs + b * 2 * (long long)cap_in;
    const Out out = out_of(o, b, p);
    const double dur = (double)len / (double)p.sampling_rate;
    Fuse f{0.0, 0, 0};
    for (int base = 0; base < cnt; base += 64) {
        const int k = base + lane;
        const bool valid = k < cnt;
        double s = 0.0, e = 0.0;
        if (valid) {
            s = round1(row[2 * k], p.sampling_rate);
            e = round1(row[2 * k + 1], p.sampling_rate);
            if (0.0 > s) s = 0.0;
            if (dur < e) e = dur;
        }
        f.rows(valid, s, e, p, lane, out);
    }
    f.finish(lane, out);
    report(o.head, o.counts, b, lane, f.opened, o.cap, false);
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what every entry point checks of its parameters and outputs, before any HIP call
inline int check_common(const char *who, const vadx_ts_params *p, int batch, const double *seconds, const int64_t *samples, const int32_t *counts,
                        int cap, const void *head) {
    VADX_REQUIRE(p, "%s: params is NULL", who);
    VADX_REQUIRE(seconds && samples && counts && head, "%s: seconds, samples, counts and head must not be NULL", who);
    VADX_REQUIRE(batch >= 1, "%s: batch=%d must be positive", who, batch);
    VADX_REQUIRE(cap >= 1 && cap <= (1 << 30), "%s: cap=%d must be in [1, 2^30]", who, cap);
    VADX_REQUIRE(p->sampling_rate >= 1, "%s: sampling_rate=%d must be positive", who, p->sampling_rate);
    VADX_REQUIRE(p->sample_rule == VADX_TS_NEAREST || p->sample_rule == VADX_TS_TRUNC, "%s: sample_rule=%d must be VADX_TS_NEAREST or VADX_TS_TRUNC", who,
                 p->sample_rule);
    VADX_REQUIRE(p->process == 0 || p->process == 1, "%s: process=%d must be 0 or 1", who, p->process);
    VADX_REQUIRE(!p->process || (p->fusion_threshold == p->fusion_threshold && p->min_duration == p->min_duration),
                 "%s: fusion_threshold and min_duration must not be NaN", who);
    VADX_REQUIRE(aligned(seconds, 8) && aligned(samples, 8) && aligned(counts, 4) && aligned(head, 4),
                 "%s: seconds and samples must be 8-byte aligned, counts and head 4-byte", who);
    return VADX_OK;
}

}  // namespace tstable
}  // namespace vadx

using namespace vadx::tstable;

#define VADX_TS_LAUNCH(kernel, ...)                                                                                          \
    do {                                                                                                                     \
        hipStream_t s_ = static_cast<hipStream_t>(stream);                                                                   \
        const Outs o_{seconds, reinterpret_cast<long long *>(samples), counts, static_cast<int *>(head), cap};               \
        VADX_HIP_TRY(hipMemsetAsync(head, 0, 16, s_));                                                                       \
        hipLaunchKernelGGL(kernel, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s_, *prm, __VA_ARGS__, batch, o_);        \
        VADX_HIP_TRY(hipGetLastError());                                                                                     \
        return VADX_OK;                                                                                                      \
    } while (0)

extern "C" int vadx_timestamps_flags(const vadx_ts_params *prm, const uint8_t *flags, int64_t stride, const int32_t *n_flags, int batch,
                                     double *seconds, int64_t *samples, int32_t *counts, int cap, void *head, void *stream) {
    const int rc = check_common("vadx_timestamps_flags", prm, batch, seconds, samples, counts, cap, head);
    if (rc != VADX_OK) return rc;
    VADX_REQUIRE(flags && n_flags, "vadx_timestamps_flags: flags and n_flags must not be NULL");
    VADX_REQUIRE(stride >= 0, "vadx_timestamps_flags: stride=%lld must not be negative", (long long)stride);
    VADX_REQUIRE(prm->frame_s > 0 && prm->frame_s < 1e300, "vadx_timestamps_flags: frame_s=%g must be positive and finite", prm->frame_s);
    VADX_REQUIRE(aligned(n_flags, 4), "vadx_timestamps_flags: n_flags must be 4-byte aligned");
    VADX_TS_LAUNCH(flags_kernel, flags, (long long)stride, n_flags);
}

extern "C" int vadx_timestamps_frames(const vadx_ts_params *prm, const int32_t *segments, const int32_t *counts_in, int cap_in,
                                      const int32_t *n_frames, const double *wav_dur, int batch, double *seconds, int64_t *samples,
                                      int32_t *counts, int cap, void *head, void *stream) {
    const int rc = check_common("vadx_timestamps_frames", prm, batch, seconds, samples, counts, cap, head);
    if (rc != VADX_OK) return rc;
    VADX_REQUIRE(segments && counts_in && n_frames && wav_dur, "vadx_timestamps_frames: segments, counts_in, n_frames and wav_dur must not be NULL");
    VADX_REQUIRE(cap_in >= 1, "vadx_timestamps_frames: cap_in=%d must be positive", cap_in);
    VADX_REQUIRE(prm->frame_shift > 0 && prm->frame_shift < 1e30f, "vadx_timestamps_frames: frame_shift=%g must be positive and finite", prm->frame_shift);
    VADX_REQUIRE(prm->use_frame_length == 0 || (prm->use_frame_length == 1 && prm->frame_length == prm->frame_length),
                 "vadx_timestamps_frames: use_frame_length must be 0 or 1, frame_length not NaN");
    VADX_REQUIRE(aligned(segments, 4) && aligned(counts_in, 4) && aligned(n_frames, 4) && aligned(wav_dur, 8),
                 "vadx_timestamps_frames: segments, counts_in and n_frames must be 4-byte aligned, wav_dur 8-byte");
    VADX_TS_LAUNCH(frames_kernel, segments, counts_in, cap_in, n_frames, wav_dur);
}

extern "C" int vadx_timestamps_samples(const vadx_ts_params *prm, const int64_t *segments, const int32_t *counts_in, int cap_in,
                                       const int64_t *clip_len, int batch, double *seconds, int64_t *samples, int32_t *counts, int cap,
                                       void *head, void *stream) {
    const int rc = check_common("vadx_timestamps_samples", prm, batch, seconds, samples, counts, cap, head);
    if (rc != VADX_OK) return rc;
    VADX_REQUIRE(segments && counts_in && clip_len, "vadx_timestamps_samples: segments, counts_in and clip_len must not be NULL");
    VADX_REQUIRE(cap_in >= 1, "vadx_timestamps_samples: cap_in=%d must be positive", cap_in);
    VADX_REQUIRE(prm->sampling_rate == 16000 || prm->sampling_rate == 8000,
                 "vadx_timestamps_samples: sampling_rate=%d must be 16000 or 8000 (the tie rule of round(x / sr, 1) is derived for these)", prm->sampling_rate);
    VADX_REQUIRE(aligned(segments, 8) && aligned(counts_in, 4) && aligned(clip_len, 8),
                 "vadx_timestamps_samples: segments and clip_len must be 8-byte aligned, counts_in 4-byte");
    VADX_TS_LAUNCH(samples_kernel, reinterpret_cast<const long long *>(segments), counts_in, cap_in, reinterpret_cast<const long long *>(clip_len));
}
