// ragged.hip -- the copies around a RAGGED batch (clips of any lengths packed into one int16 vector, include/vadx.h "Ragged batches"):
//   vadx_windows_gather   packed PCM + one source offset per analysis window -> window_buf int16 [n_windows][window_len], the layout the
//                         front-end entry points take with batch = n_windows, windows_per_clip = 1 (the slicing of
//                         FSMN/Inference_FSMN_VAD_ONNX.py:162-167 and FireRedVAD/Inference_FireRed_ONNX.py:560-566 for every clip at once);
//   vadx_windows_gather_any  the same rows for a window / stride that is no multiple of 8 samples (DFSMN, Inference_DFSMN_VAD_ONNX.py:221-229),
//                         once per channel;
//   vadx_tracks_gather    per-window scores [n_windows][win_floats] -> one zero-filled track row per clip, what vadx_vadpost takes
//                         (the np.concatenate + [:num_valid_frames] of Inference_FireRed_ONNX.py:574-579).
// All are pure copies: HBM-bound, no arithmetic.
#include "common.h"

namespace vadx {
namespace ragged {

typedef short s16x8 __attribute__((ext_vector_type(8)));

// One workgroup per window, 16-byte runs (window_len and every offset are multiples of 8 samples, both buffers 16-byte aligned).  An
// offset that is negative, not a multiple of 8 or whose window would end past pcm_len reads nothing: that window is zeros.
__global__ __launch_bounds__(256) void windows_gather_kernel(const int16_t *__restrict__ pcm, long long pcm_len, const long long *__restrict__ win_src,
                                                             int window_len, int16_t *__restrict__ wbuf) {
    const long long w = blockIdx.x, src = win_src[w];
    const int nl = window_len / 8, tid = threadIdx.x;
    s16x8 *win = reinterpret_cast<s16x8 *>(wbuf + w * window_len);
    const bool inside = src >= 0 && (src & 7) == 0 && pcm_len >= window_len && src <= pcm_len - window_len;
    if (!inside) {
        for (int v = tid; v < nl; v += 256) win[v] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    const s16x8 *from = reinterpret_cast<const s16x8 *>(pcm + src);
    for (int v = tid; v < nl; v += 256) win[v] = from[v];
}

// The same copy for a grid that is not made of 16-byte runs (DFSMN: 16 001 samples every 10 881): one workgroup per window, one int16 per
// access, any offset >= 0 and any window_len >= 1.  A window whose source range leaves [0, pcm_len) reads nothing: it is zeros.
__global__ __launch_bounds__(256) void windows_gather_any_kernel(const int16_t *__restrict__ pcm, long long pcm_len, const long long *__restrict__ win_src,
                                                                 int window_len, int16_t *__restrict__ wbuf) {
    const long long w = blockIdx.x, src = win_src[w];
    int16_t *win = wbuf + w * window_len;
    const bool inside = src >= 0 && pcm_len >= window_len && src <= pcm_len - window_len;
    const int16_t *from = pcm + (inside ? src : 0);
    for (int i = threadIdx.x; i < window_len; i += 256) win[i] = inside ? from[i] : (int16_t)0;
}

// tracks[b][j] = probs[win_first[b] + j / fpw][chan_offset + j % fpw] for j < min(n_frames[b], W_b * fpw), 0 up to track_stride
__global__ __launch_bounds__(256) void tracks_gather_kernel(const float *__restrict__ probs, long long win_floats, int chan_offset, int fpw,
                                                            const int *__restrict__ win_first, const int *__restrict__ n_frames,
                                                            float *__restrict__ tracks, int track_stride) {
    const int nchunk = (track_stride + 255) / 256, b = blockIdx.x / nchunk, j = (blockIdx.x - b * nchunk) * 256 + threadIdx.x;
    if (j >= track_stride) return;
    const int first = win_first[b], W = win_first[b + 1] - first;
    long long n = n_frames[b];
    if (first < 0 || W < 0) n = 0;
    else if (n > (long long)W * fpw) n = (long long)W * fpw;
    float v = 0.f;
    if (j < n) {
        const int k = j / fpw, t = j - k * fpw;
        v = probs[((long long)first + k) * win_floats + chan_offset + t];
    }
    tracks[(long long)b * track_stride + j] = v;
}

}  // namespace ragged
}  // namespace vadx

using namespace vadx::ragged;

extern "C" int vadx_windows_gather(const int16_t *pcm, int64_t pcm_len, const int64_t *win_src, int n_windows, int window_len,
                                   int16_t *window_buf, void *stream) {
    VADX_REQUIRE(pcm && win_src && window_buf, "vadx_windows_gather: NULL argument");
    VADX_REQUIRE(n_windows >= 1 && pcm_len >= 1, "vadx_windows_gather: n_windows=%d pcm_len=%lld must be positive", n_windows, (long long)pcm_len);
    VADX_REQUIRE(window_len >= 8 && window_len % 8 == 0, "vadx_windows_gather: window_len=%d must be a positive multiple of 8", window_len);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(pcm) | reinterpret_cast<uintptr_t>(window_buf)) & 15) == 0 && (reinterpret_cast<uintptr_t>(win_src) & 7) == 0,
                 "vadx_windows_gather: pcm and window_buf must be 16-byte aligned, win_src 8-byte aligned");
    hipLaunchKernelGGL(windows_gather_kernel, dim3((unsigned)n_windows), dim3(256), 0, static_cast<hipStream_t>(stream), pcm, (long long)pcm_len,
                       reinterpret_cast<const long long *>(win_src), window_len, window_buf);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_windows_gather_any(const int16_t *pcm, int64_t pcm_len, const int64_t *win_src, int n_windows, int window_len,
                                       int16_t *window_buf, void *stream) {
    VADX_REQUIRE(pcm && win_src && window_buf, "vadx_windows_gather_any: NULL argument (pcm, win_src, window_buf)");
    VADX_REQUIRE(n_windows >= 1, "vadx_windows_gather_any: n_windows=%d must be positive", n_windows);
    VADX_REQUIRE(pcm_len >= 1, "vadx_windows_gather_any: pcm_len=%lld must be positive", (long long)pcm_len);
    VADX_REQUIRE(window_len >= 1, "vadx_windows_gather_any: window_len=%d must be positive", window_len);
    VADX_REQUIRE(((reinterpret_cast<uintptr_t>(pcm) | reinterpret_cast<uintptr_t>(window_buf)) & 1) == 0 && (reinterpret_cast<uintptr_t>(win_src) & 7) == 0,
                 "vadx_windows_gather_any: pcm and window_buf must be 2-byte aligned, win_src 8-byte aligned");
    hipLaunchKernelGGL(windows_gather_any_kernel, dim3((unsigned)n_windows), dim3(256), 0, static_cast<hipStream_t>(stream), pcm, (long long)pcm_len,
                       reinterpret_cast<const long long *>(win_src), window_len, window_buf);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}

extern "C" int vadx_tracks_gather(const float *probs, int64_t win_floats, int chan_offset, int frames_per_window, const int32_t *win_first,
                                  const int32_t *n_frames, int batch, float *tracks, int track_stride, void *stream) {
    VADX_REQUIRE(probs && win_first && n_frames && tracks, "vadx_tracks_gather: NULL argument");
    VADX_REQUIRE(batch >= 1 && track_stride >= 1 && (long long)batch * ((track_stride + 255) / 256) < (1ll << 31),
                 "vadx_tracks_gather: batch=%d track_stride=%d must be positive (and batch * ceil(track_stride / 256) < 2^31)", batch, track_stride);
    VADX_REQUIRE(frames_per_window >= 1 && chan_offset >= 0 && (int64_t)chan_offset + frames_per_window <= win_floats,
                 "vadx_tracks_gather: chan_offset=%d + frames_per_window=%d must lie inside a window's win_floats=%lld scores", chan_offset,
                 frames_per_window, (long long)win_floats);
    hipLaunchKernelGGL(tracks_gather_kernel, dim3((unsigned)(batch * ((track_stride + 255) / 256))), dim3(256), 0,
                       static_cast<hipStream_t>(stream), probs, (long long)win_floats, chan_offset, frames_per_window, win_first, n_frames, tracks,
                       track_stride);
    VADX_HIP_TRY(hipGetLastError());
    return VADX_OK;
}
