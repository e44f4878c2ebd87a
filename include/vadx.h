/* vadx.h -- C ABI of the MI355X-native batched VAD engine (libvadx.so).
 *
 * The reference (DakeQQ/Voice-Activity-Detection-VAD-ONNX) has no native FFI: its drop-in seam is
 * the ONNX-Runtime Python session object (`session.run(output_names, feeds)`), plus for Silero the
 * `OnnxWrapper` object.  Each entry point below is what a binding for that seam calls; the
 * comment on each names the reference interface it replaces (file:line under the reference root).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / hip types in signatures (`stream` is a hipStream_t
 *     passed as void*; NULL = the default stream);
 *   - all data pointers are DEVICE pointers unless the name ends in `_host`;
 *   - caller-owned buffers, no hidden allocation, stream-ordered (no device sync inside);
 *   - return 0 on success, a negative VADX_E* code otherwise; `vadx_last_error()` gives the text.
 */
#ifndef VADX_H
#define VADX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VADX_OK          0
#define VADX_EINVAL     -1   /* bad argument (shape, NULL pointer, unsupported sample rate ...) */
#define VADX_ENOSPACE   -2   /* workspace / output capacity too small */
#define VADX_EHIP       -3   /* a HIP runtime call failed */

/* THE ABI number: the library (csrc/capi.hip), the ctypes binding (vadx._lib.ABI_VERSION, parsed from this line),
 * the C client (tests/c/cabi_silero.c) and __graft_entry__.build() all read it from here and nowhere else.
 * 3: vadx_frontend_cfg grew `fold`; vadx_frontend_fold_kind, vadx_dfsmn_cfb_*, _lstm_t_ex, _ft_repack (round 3).
 * 4: vadx_silero_encoder_mode, vadx_gemm_mode; the Silero / FSMN packed blobs grew the bf16 x 3 weight fragments (round 4).
 * 5: vadx_dfsmn_cfb_weights grew fwd_tbl_q / inv_tbl_q (the struct must be zero-initialised at its ABI-5 size: an ABI-4 caller's shorter
 *    struct would have the new pointers read past its end -- the version check is the guard); vadx_stream_vadpost* (round 4).
 * 6: the arithmetic of an entry point comes WITH THE CALL (VADX_ARITH_* in a cfg / dims struct) instead of process-wide switches:
 *    vadx_silero_encoder_mode and vadx_gemm_mode are gone, every Silero launch takes a trailing `const vadx_silero_cfg *`;
 *    VADX_ARITH_F16X2 (fp16 x 2 split products) + vadx_silero_range_flag; the Silero packed blob grew the fp16 fragments;
 *    vadx_sepconv_block / vadx_marblenet_block2 / vadx_marblenet_tail take a trailing `const vadx_marblenet_cfg *` (NULL = float32 MFMAs),
 *    vadx_frag_h2_host / vadx_frag_h2_floats; vadx_dfsmn_lstm_f and vadx_dfsmn_lstm_t_ex take (arithmetic, range_flag) (round 5).
 * 7: no signature changed; three behaviours did (round 6).  (a) VADX_ARITH_AUTO of vadx_fsmn_dims / vadx_firered_cfg is BF16X3 (float32's
 *    exponent range: nothing for the caller to check); F16X2 is an explicit request there, by callers that read the range flag.  Silero's AUTO
 *    stays F16X2, and (b) a Silero workgroup whose activations left the fp16 range writes NaN instead of its gate pre-activations, so that the
 *    scores of those clips are NaN for a caller that never reads vadx_silero_range_flag (tests/c/cabi_silero.c reads it).  (c) The pack_host
 *    functions rebalance chains of affine layers by exact powers of two when a weight tensor sits outside [2^-10, 2^7) (csrc/rebalance.h) and
 *    refuse F16X2 for a blob that keeps a weight tensor wholly below 2^-14.
 * 8: new entry points only, no existing signature or behaviour changed: the Silero stream path vadx_silero_iter_params,
 *    vadx_silero_stream_state_bytes, vadx_silero_stream_workspace_bytes, vadx_silero_stream_run.
 * 9: additive: vadx_silero_cfg's reserved words became `ext` {sample_rate, reserved1, reserved2} (same size; 0 = 16000, as before), 8000 selects the 8 kHz
 *    network on every Silero launch; vadx_silero_packed_floats_sr, vadx_silero_pack_host_sr pack the 8 kHz blob.
 * 10: new entry points only: the FSMN stream path vadx_fsmn_stream_state_bytes, vadx_fsmn_stream_windows, vadx_fsmn_stream_run.
 *     Later additions under the SAME number (additive again: nothing an ABI-10 caller links against moved, and the suite's pin of this
 *     number, tests/test_fsmn_stream_cpu.py, stays as it is): the ragged-batch entry points vadx_windows_gather, vadx_fsmn_clips_ragged,
 *     vadx_tracks_gather; then MarbleNet over ragged batches: vadx_marblenet_ragged, vadx_frontend_logmel_ragged, vadx_sepconv_block_ragged,
 *     vadx_marblenet_block2_ragged, vadx_marblenet_tail_ragged; then FireRed Stream-VAD over live streams: vadx_firered_stream_state_bytes,
 *     vadx_firered_stream_group_max, vadx_firered_stream_tick; then FSMN windows of any length: vadx_fsmn_long_workspace_bytes,
 *     vadx_fsmn_window_stats_long, vadx_fsmn_run_long, vadx_fsmn_clips_long; then DFSMN over ragged batches and live streams:
 *     vadx_windows_gather_any, vadx_dfsmn_vote_ragged, vadx_dfsmn_stream_state_bytes, vadx_dfsmn_stream_windows, vadx_dfsmn_stream_vote; then
 *     MarbleNet over live streams: vadx_marblenet_stream_weights, vadx_marblenet_stream_max_frames, vadx_marblenet_stream_cap,
 *     vadx_marblenet_stream_state_bytes, vadx_marblenet_stream_workspace_bytes, vadx_marblenet_stream_tick, vadx_frontend_logmel_stream; then
 *     cutting the speech out on the device: vadx_chunks_plan_bytes, vadx_chunks_plan, vadx_chunks_copy; then timestamps on the device:
 *     vadx_timestamps_flags, vadx_timestamps_frames, vadx_timestamps_samples; then preparing a ragged batch on the device:
 *     vadx_ingest_pcm16_ragged, vadx_prepare_workspace_bytes, vadx_prepare_stats, vadx_prepare_scale, vadx_prepare_write; then Silero over
 *     ragged batches: vadx_silero_ragged, vadx_silero_ragged_workspace_bytes, vadx_silero_encode_ragged, vadx_silero_encode_ragged_pcm16,
 *     vadx_silero_recur_ragged, vadx_silero_clips_ragged, vadx_silero_segments_ragged; then the 8 kHz network over ragged batches:
 *     vadx_silero_encode_ragged_8k, vadx_silero_encode_ragged_8k_pcm16, vadx_silero_recur_ragged_8k, vadx_silero_clips_ragged_8k
 *     (and two relaxations: vadx_silero_segments_ragged takes sampling_rate 8000, a vadx_silero_ragged may describe a run of groups); then
 *     ragged ticks of the Silero streams: vadx_silero_stream_ragged_max_windows, vadx_silero_stream_plan_bytes,
 *     vadx_silero_stream_ragged_workspace_bytes, vadx_silero_stream_plan, vadx_silero_stream_run_ragged; then ragged ticks of the FSMN
 *     streams: vadx_fsmn_stream_ragged_max_windows, vadx_fsmn_stream_windows_ragged, vadx_fsmn_stream_run_ragged; then ragged ticks of the FireRed
 *     streams: vadx_firered_stream_tick_ragged; then FireRed windows of any length: vadx_firered_long_tables,
 *     vadx_firered_long_workspace_bytes, vadx_firered_run_long, vadx_frontend_logmel_ragged_snip.
 *     A caller that needs them checks for the symbols (dlsym), not for a number. */
#define VADX_ABI_VERSION 10

/* Arithmetic of the products whose one operand is a constant (every weight matrix, every DFT table) -- float32 RESULTS in all of them:
 *   F32     v_mfma_f32_16x16x4_f32 on the float32 operands themselves;
 *   BF16X3  operands split EXACTLY into three bf16 terms, six v_mfma_f32_16x16x32_bf16 per K = 32 step (csrc/split3.h): float32-class
 *           accuracy at 6/16 of the matrix time, float32's exponent range;
 *   F16X2   operands represented to one float32 ulp by two round-to-nearest fp16 terms, three v_mfma_f32_16x16x32_f16 per K = 32 step
 *           (csrc/split2.h): float32-class accuracy at 3/16 of the matrix time; activations must stay inside the fp16 range (|x| <= 65504),
 *           which the kernels check (vadx_silero_range_flag / vadx_fsmn_range_flag / vadx_firered_range_flag: the caller reads the flag with
 *           the results and recomputes a flagged batch on BF16X3 -- the RANGE PROTOCOL; tests/c/cabi_silero.c shows it);
 *   AUTO    the library's default for the entry point (what a zero-initialised cfg selects). */
#define VADX_ARITH_AUTO   0
#define VADX_ARITH_F32    1
#define VADX_ARITH_BF16X3 2
#define VADX_ARITH_F16X2  3

int         vadx_abi_version(void);      /* == VADX_ABI_VERSION of the header the library was built from */
const char *vadx_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Silero
 * ------------------------------------------------------------------------------------------- */

/* Original-layout float32 weights on the HOST (same tensors as the ONNX initialisers):
 * stft_basis [258][256]; enc_w[i] [c_out][c_in][3], enc_b[i] [c_out] for the four encoder convs
 * (129->128 s1, 128->64 s2, 64->64 s2, 64->128 s1); LSTM cell [512][128] x2 + biases [512] x2 in
 * torch gate order (i,f,g,o); decoder conv [128] + bias [1].
 * The 8 kHz network (vadx_silero_pack_host_sr(8000, ...)) has the same tensors except stft_basis [130][128] (65 bins re, then im;
 * stride 64) and enc_w[0] [128][65][3]. */
typedef struct vadx_silero_weights_host {
    const float *stft_basis;
    const float *enc_w[4];
    const float *enc_b[4];
    const float *lstm_w_ih, *lstm_w_hh, *lstm_b_ih, *lstm_b_hh;
    const float *dec_w, *dec_b;
} vadx_silero_weights_host;

/* Per-call configuration of the Silero launches; NULL = all defaults.  Zero-initialise it. */
typedef struct vadx_silero_cfg {
    int32_t arithmetic;     /* VADX_ARITH_*: AUTO = F16X2 (run the range protocol: vadx_silero_range_flag below).  The three kernel sets read the same packed blob and write the same workspace, so the
                             * encoder and recurrent launches of one batch may even differ.  Replaces nothing in the reference: onnxruntime has
                             * one CPU kernel set. */
    struct {                /* ABI 9: formerly int32_t reserved[3] -- same size, and `{arithmetic, {0, 0, 0}}` initialisers still compile */
        int32_t sample_rate;    /* 0 or 16000 = the 16 kHz network (windows of 512 samples, 64 of context), 8000 = the 8 kHz network (256,
                                 * 32); anything else is VADX_EINVAL.  `packed` must be the blob packed for this rate */
        int32_t reserved1, reserved2;    /* must be zero */
    } ext;
} vadx_silero_cfg;

/* Number of floats of the packed (kernel-layout) weight blob. */
size_t vadx_silero_packed_floats(void);
/* Repack on the host (init time only); the caller uploads `packed_host` to the device once.
 * Replaces: onnxruntime.InferenceSession(path) construction, Silero/modeling_modified/utils_vad.py:39. */
int vadx_silero_pack_host(const vadx_silero_weights_host *w, float *packed_host);
/* The same for either network: sample_rate 16000 is vadx_silero_pack_host, 8000 packs the 8 kHz network (its tensors' shapes above) into a
 * blob of the same size, tagged: an 8 kHz launch on a blob without the tag (a 16 kHz blob) writes NaN gate pre-activations and raises bit 2
 * (value 4) of vadx_silero_range_flag, it never scores.  A 16 kHz launch must be given a 16 kHz blob -- the caller's contract, as
 * vadx_fsmn_dims' "pass the same dims": an 8 kHz blob there is not detected.  vadx_silero_packed_floats_sr returns 0 for another rate. */
size_t vadx_silero_packed_floats_sr(int sample_rate);
int vadx_silero_pack_host_sr(int sample_rate, const vadx_silero_weights_host *w, float *packed_host);

/* Scratch needed by the two calls below, in bytes. `steps` = windows per clip (1 for vadx_silero_step). */
size_t vadx_silero_workspace_bytes(int batch, int steps);

/* One ORT-boundary call, batched:
 *   feeds  {'input': f32 [B,576], 'state': f32 [2,B,128], 'sr': int64 scalar}
 *   fetches(out f32 [B,1], stateN f32 [2,B,128])
 * Replaces: self.session.run(None, ort_inputs), Silero/modeling_modified/utils_vad.py:116-119.
 * sr must equal the cfg's sample_rate (16000 by default; the reference model's sr input, utils_vad.py:62-67); at 8000 the input is [B,288]
 * (32 context + 256 samples). */
int vadx_silero_step(const float *packed, const float *input, const float *state, int64_t sr,
                     int batch, float *out, float *state_n,
                     void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);

/* Whole clips, batched: audio f32 [B][row_stride] (first n_samples valid per row, +-1 scale),
 * zero state and zero context at t=0, last window zero-padded; probs f32 [B][T], T = ceil(n/512) (ceil(n/256) at 8 kHz: every launch
 * below takes the window of the cfg's sample_rate).
 * state_n (optional, may be NULL) receives the final [2,B,128].
 * Replaces the window loop of get_speech_timestamps, utils_vad.py:350,359-372, and
 * OnnxWrapper.audio_forward, utils_vad.py:130-146 (context carry :111-114,:123 is done in-kernel). */
int vadx_silero_clips(const float *packed, const float *audio, int batch, int64_t n_samples,
                      int64_t row_stride, float *probs, float *state_n,
                      void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);

/* The two halves of vadx_silero_clips as separate launches (same buffers, same results), so a
 * harness can time the state-independent encoder (STFT conv + conv stack + W_ih, the dominant
 * kernel) and the recurrent kernel separately.  `steps` = ceil(n_samples/512) (/256 at 8 kHz). */
int vadx_silero_encode(const float *packed, const float *audio, int batch, int64_t n_samples,
                       int64_t row_stride, void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
/* The same encoder fed int16 PCM: sample = (float)pcm * scale in one f32 rounding -- with scale = 0.000030517578f exactly the
 * float32 array the reference script builds on the host (Silero/Inference_Silero_VAD_ONNX.py:83), so results are
 * bit-identical to vadx_silero_encode on that array while the upload and the HBM read are half the bytes. */
int vadx_silero_encode_pcm16(const float *packed, const int16_t *audio, float scale, int batch, int64_t n_samples,
                             int64_t row_stride, void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
/* A slice of the batch: clips [first_clip, first_clip + batch) of a workspace laid out for total_batch clips (first_clip a
 * multiple of 16).  Lets the encoder of one uploaded chunk run while the next chunk is still crossing PCIe (bench.py's
 * feed-inclusive mode, SURVEY 8e "pinned-host staging double-buffered per GPU"); one vadx_silero_recur over total_batch
 * follows.  Results are identical to a single vadx_silero_encode_pcm16 over the whole batch. */
int vadx_silero_encode_pcm16_part(const float *packed, const int16_t *audio, float scale, int batch, int64_t n_samples,
                                  int64_t row_stride, int first_clip, int total_batch, void *workspace,
                                  size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_recur(const float *packed, const void *workspace, size_t workspace_bytes, int batch,
                      int steps, const float *state0, float *probs, float *state_n, void *stream, const vadx_silero_cfg *cfg);

/* The same two launches over a SPAN of windows [first_step, first_step + n_steps) of the clips, for recordings whose
 * whole-clip workspace (32 KB per 16-clip group and window) is too large: the caller walks the spans in order on one
 * stream with one span-sized workspace (vadx_silero_workspace_bytes(batch, n_steps)), as
 * vadx.silero.SileroEngine.clips_spanned does.  encode_span reads the clip rows with the usual zero context before
 * sample 0 and zero padding after n_samples.  recur_span: `probs` points at column first_step of the [B][probs_stride]
 * table, state0 (NULL = zeros) / state_n (may alias state0) carry [2,B,128] between spans.  Results are identical to
 * the single launches (same kernels, same arithmetic order).  (Running span k's recurrence on a second stream under
 * span k+1's encoder was measured and gains nothing: both kernels are matrix-pipe-bound) */
int vadx_silero_encode_span(const float *packed, const float *audio, int batch, int64_t n_samples,
                            int64_t row_stride, int first_step, int n_steps, void *workspace,
                            size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_recur_span(const float *packed, const void *workspace, size_t workspace_bytes, int batch,
                           int n_steps, const float *state0, float *probs, int64_t probs_stride,
                           float *state_n, void *stream, const vadx_silero_cfg *cfg);

/* Parameters of the segmenter; defaults of get_speech_timestamps (utils_vad.py:248-263). */
typedef struct vadx_silero_seg_params {
    double threshold;                 /* 0.5 */
    double neg_threshold;             /* <0 => max(threshold-0.15, 0.01) */
    int    sampling_rate;             /* 16000 */
    double min_speech_duration_ms;    /* 250 */
    double max_speech_duration_s;     /* inf */
    double min_silence_duration_ms;   /* 100 */
    double speech_pad_ms;             /* 30 */
    double min_silence_at_max_speech; /* 98 */
    int    use_max_poss_sil_at_max_speech; /* 1 */
} vadx_silero_seg_params;

/* Device-side dual-threshold segmenter, one clip per thread: probs f32 [B][T] -> padded sample
 * index pairs int64 [B][cap][2] + counts int32 [B] (count > cap => truncated, VADX_ENOSPACE is NOT
 * raised on device; the host checks counts).  n_samples int64 [B] = true clip lengths.
 * Replaces: the state machine + padding of get_speech_timestamps, utils_vad.py:374-476
 * (the seconds rounding :478-482 stays on the host: it is Python round()).  On the device, from this call's table:
 * vadx_timestamps_samples, section "Timestamps". */
int vadx_silero_segments(const float *probs, int batch, int steps, const int64_t *n_samples,
                         const vadx_silero_seg_params *params, int64_t *segments, int32_t *counts,
                         int cap, void *stream);

/* VADX_ARITH_F16X2 (csrc/split2.h: every product, the STFT included, as three v_mfma_f32_16x16x32_f16 per K = 32 step on operands
 * represented to one float32 ulp by two round-to-nearest fp16 terms).  fp16 terms do not have float32's exponent range: the F16X2
 * kernels keep the largest |activation| they split and raise a sticky flag inside the packed blob when one left the fp16
 * range (|x| > 65504), or when the blob cannot run in this mode at all (a weight outside the range, an STFT basis without the DFT
 * symmetries).  This call copies the flag (0 = every result since the last reset is valid) and, when non-zero, the largest magnitude
 * seen to the host (it synchronises `stream`); reset != 0 clears it.  A flagged batch must be recomputed with VADX_ARITH_BF16X3, whose
 * bf16 terms have float32's range (vadx.silero.SileroEngine and tests/c/cabi_silero.c do so).  A caller that skips this does not read
 * plausible numbers: a flagged workgroup hands the recurrent kernel NaN, and the scores of its clips are NaN from that window on (ABI 7).
 * The underflow side needs no protocol: pack_host rebalances layers whose weights sit outside [2^-10, 2^7) by exact powers of two
 * (csrc/rebalance.h) and marks a blob with a weight tensor wholly below 2^-14 as unusable for this arithmetic (flag bit 1 on a launch). */
int vadx_silero_range_flag(const float *packed, int reset, uint32_t *flag_host, float *amax_host, void *stream);

/* Silero over a RAGGED batch: clips of any lengths in ONE packed source vector (float32 on the +-1 scale, or int16 PCM
 * scaled while staging as vadx_silero_encode_pcm16 does), scored in one encoder and one recurrent launch whose work follows the clips'
 * own window counts T_b = ceil(len_b / 512) instead of batch x the longest clip's.  (The 16 kHz network is described; the 8 kHz one,
 * windows of 256 samples, has the _8k entry points below and is otherwise the same.)  The host sorts the clips by T_b (descending, stable)
 * and takes sixteen at a time -- one MFMA column tile -- as a GROUP; slot s = 16 g + i is column i of group g.  A group runs T_g = the
 * window count of its first slot; its gx tiles (32 KB each) lie CONSECUTIVELY in the workspace from tile gx_first[g] (the rectangular
 * layout is window-major).  The encoder's workgroups find their work in wg_tab: one entry per (group, run of VADX_SILERO_RAGGED_RUN
 * consecutive windows), ordered run-major over the groups that still have that run, read with uniform loads -- no search.
 * Per slot the window is read as the rectangular kernel reads a clip of n_samples = slot_len: zero beyond the clip's own end, reflect
 * pad over that; an empty slot (slot_clip = -1, behind the last clip of a partial group) stages zeros.  A slot may start at any element
 * of the source; one that does not start on a multiple of four elements is loaded element by element, with the same result.
 * Scores: one packed float32 vector [probs_first[clips]], clip b's T_b scores from probs_first[b] (the caller's clip order); a clip's
 * LSTM state stops changing behind its own last window, so state_n [2][clips][128] holds every clip's state after its last window.
 * The device trusts no slot: one whose [slot_off, slot_off + slot_len) leaves [0, n_src) is not read at all, its scores are NaN,
 * bit 0 of *status is raised (the caller zeroes the word), and no other clip's result changes.  The remaining tables are functions of
 * the lengths (vadx.ragged.RaggedClips._set_tables writes them) and are the caller's contract, as a rectangular call's batch and steps.
 * A table set may describe a RUN OF A BATCH'S GROUPS, 1 <= groups <= ceil(clips / 16): slot_*, grp_min_len start at the run's first group,
 * gx_first is rebased to the run (gx_first[0] = 0, tiles = gx_first[groups]), wg_tab numbers the run's groups from 0, while clips,
 * slot_clip, probs_first, probs and state_n stay the whole batch's -- the launch writes the scores and states of the run's clips to their
 * places and nothing else.  Groups are independent workgroups, so a batch whose workspace would be too large runs as consecutive such
 * launches on one smaller workspace, in stream order, with the results of the single launch (vadx.ragged.RaggedClips.parts). */
#define VADX_SILERO_RAGGED_RUN 4                /* windows per wg_tab entry = the fp16 x 2 encoder's tiles per workgroup (H2_NSUB) */
typedef struct vadx_silero_ragged {             /* every pointer: device memory */
    const int64_t *slot_off;                    /* [16 groups] first element of the slot's clip in the source vector (0: empty slot) */
    const int32_t *slot_len;                    /* [16 groups] its samples (0: empty slot) */
    const int32_t *slot_clip;                   /* [16 groups] the caller's clip index, -1: empty slot */
    const int32_t *gx_first;                    /* [groups + 1] prefix of T_g, in gx tiles */
    const int32_t *grp_min_len;                 /* [groups] the shortest slot_len of a full group, 0 for a partial one: windows that end below it
                                                   are covered by every clip of the group (the encoder's vector staging; the device takes
                                                   the smaller of this and what its own slot checks leave) */
    const int32_t *wg_tab;                      /* [n_runs][2] (group, run) */
    const int64_t *probs_first;                 /* [clips + 1] prefix of T_b in the caller's clip order */
    uint32_t *status;                           /* [1] bit 0: a slot lay outside the source vector (bit 1: vadx_silero_stream_plan) */
    int32_t clips, groups, n_runs, tiles;       /* tiles = gx_first[groups] */
} vadx_silero_ragged;
size_t vadx_silero_ragged_workspace_bytes(int64_t tiles);          /* tiles x 32 KB */
/* The halves of vadx_silero_clips_ragged (no range protocol of their own, as vadx_silero_encode / _recur).  n_src = elements of `src`.
 * cfg->ext.sample_rate = 8000 is refused by these four: a table set carries no window length, so the network comes with the entry point
 * (the _8k calls below), not with a switch that tables built for the other rate would pass silently.  A workspace below
 * vadx_silero_ragged_workspace_bytes(rg->tiles) returns VADX_ENOSPACE. */
int vadx_silero_encode_ragged(const float *packed, const float *src, int64_t n_src, const vadx_silero_ragged *rg,
                              void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_encode_ragged_pcm16(const float *packed, const int16_t *src, float scale, int64_t n_src, const vadx_silero_ragged *rg,
                                    void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_recur_ragged(const float *packed, const void *workspace, size_t workspace_bytes, int64_t n_src,
                             const vadx_silero_ragged *rg, float *probs, float *state_n, void *stream, const vadx_silero_cfg *cfg);
/* encode then recur; src_int16 != 0: `src` is int16 PCM scaled by `scale`, otherwise float32 (scale ignored).  state_n may be NULL. */
int vadx_silero_clips_ragged(const float *packed, const void *src, int src_int16, float scale, int64_t n_src,
                             const vadx_silero_ragged *rg, float *probs, float *state_n, void *workspace, size_t workspace_bytes,
                             void *stream, const vadx_silero_cfg *cfg);
/* The 8 kHz network (the blob of vadx_silero_pack_host_sr(8000, ...)) over a ragged batch whose tables count windows of 256 samples,
 * T_b = ceil(len_b / 256): arguments, layouts, device checks and results as the namesakes above; cfg must be given with
 * ext.sample_rate = 8000 (anything else: VADX_EINVAL).  The encoder stages 32 samples of context + 256 + a reflect pad of 32 per slot and
 * runs one tile per workgroup; the recurrent kernels are the 16 kHz calls' own.  A 16 kHz blob gives NaN scores and range-flag bit 2. */
int vadx_silero_encode_ragged_8k(const float *packed, const float *src, int64_t n_src, const vadx_silero_ragged *rg,
                                 void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_encode_ragged_8k_pcm16(const float *packed, const int16_t *src, float scale, int64_t n_src, const vadx_silero_ragged *rg,
                                       void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_recur_ragged_8k(const float *packed, const void *workspace, size_t workspace_bytes, int64_t n_src,
                                const vadx_silero_ragged *rg, float *probs, float *state_n, void *stream, const vadx_silero_cfg *cfg);
int vadx_silero_clips_ragged_8k(const float *packed, const void *src, int src_int16, float scale, int64_t n_src,
                                const vadx_silero_ragged *rg, float *probs, float *state_n, void *workspace, size_t workspace_bytes,
                                void *stream, const vadx_silero_cfg *cfg);
/* vadx_silero_segments on the packed scores: clip b's row starts at probs_first[b] and has probs_first[b + 1] - probs_first[b] windows
 * (of which ceil(n_samples[b] / window) are read at most; params->sampling_rate 16000 or 8000 gives the window).  Same tables out. */
int vadx_silero_segments_ragged(const float *probs, const int64_t *probs_first, int batch, const int64_t *n_samples,
                                const vadx_silero_seg_params *params, int64_t *segments, int32_t *counts, int cap, void *stream);

/* Streaming Silero: S live streams advance by `windows` 512-sample windows per call (256 at 8 kHz), each stream's context, LSTM state and VADIterator
 * machine kept in a device RECORD (vadx_silero_stream_state_bytes(S) bytes).  The record is opaque except that
 *   - its first 2*S*128 floats are the LSTM state [2][S][128] (h, then c), laid out as state_n of every other Silero call;
 *   - a record of all zero bytes is S streams in their reset state (no init call).
 * samples: [S][row_stride], windows*512 (windows*256) valid per row; f32 on the +-1 scale (samples_int16 = 0), or int16 PCM (samples_int16 != 0) scaled
 * by `scale` in one f32 rounding as vadx_silero_encode_pcm16 does.  reset (NULL or uint8 [S]): != 0 = reset_states() before this tick.
 * active (NULL or uint8 [S]): 0 = no audio for this stream this tick -- its state_out record is a bitwise copy of state_in (a reset
 * request on an inactive stream is ignored), its events are 0 and its probs NaN.  state_in is never written (a tick can be recomputed
 * from it, which the range protocol needs); state_in and state_out must not overlap.  Per window: probs f32, event_kind int8 (0 none,
 * 1 start, 2 end, -1 the window's score is not finite) and event_value f64 [S][windows], the value VADIterator computes BEFORE int()
 * (the host applies int(v) or round(v / sampling_rate, time_resolution), utils_vad.py:571-584).  A NaN score poisons the stream's
 * LSTM state in state_out, so its later windows stay -1 until it is reset: with F16X2 and no range-flag read, a flagged stream reads
 * "invalid", never a plausible silence.  One arithmetic per call for the encoder and the recurrence (AUTO = F16X2: read
 * vadx_silero_range_flag after the call and, when it is raised, recompute the tick on BF16X3 from the same state_in into the same
 * state_out).  Scores are bit for bit those of vadx_silero_clips over the concatenated audio, and so is the LSTM state.  windows <= 65536;
 * records and workspace (vadx_silero_stream_workspace_bytes) 16-byte aligned.
 * Replaces VADIterator.__init__ / reset_states / __call__, Silero/modeling_modified/utils_vad.py:494-586, one object per stream
 * (each call an OnnxWrapper call, utils_vad.py:93-128). */
typedef struct vadx_silero_iter_params {   /* VADIterator.__init__, utils_vad.py:494-533 */
    double  threshold;                     /* 0.5 */
    int32_t sampling_rate;                 /* must equal the cfg's sample_rate (16000 by default; 8000 with the 8 kHz blob and cfg) */
    double  min_silence_duration_ms;       /* 100 */
    double  speech_pad_ms;                 /* 30 */
} vadx_silero_iter_params;

size_t vadx_silero_stream_state_bytes(int streams);
size_t vadx_silero_stream_workspace_bytes(int streams, int windows);
int vadx_silero_stream_run(const float *packed, const vadx_silero_iter_params *prm,
                           const void *samples, int samples_int16, float scale, int64_t row_stride,
                           int streams, int windows, const uint8_t *reset, const uint8_t *active,
                           const void *state_in, void *state_out,
                           float *probs, int8_t *event_kind, double *event_value,
                           void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);

/* RAGGED ticks: stream s delivers n_s windows this tick, 0 <= n_s <= max_windows <= vadx_silero_stream_ragged_max_windows() = 256 (longer
 * catch-ups go through vadx_silero_stream_run); n_s = 0 is "no audio" and costs nothing.  A tick is a ragged Silero batch ("Silero over a
 * RAGGED batch" above) over the staged rows [context | n_s windows] of the streams with n_s > 0, read from origin 0 with the record's h / c
 * as the initial state: Sum T_g tiles of encoder and recurrent work instead of ceil(S / 16) * max n_s.  Its table set has clips = streams
 * and two halves:
 *   the group tables gx_first, grp_min_len (cw + window * the smallest count of a full group, 0 for a partial one; cw = window / 8),
 *   wg_tab and the counts groups = ceil(active / 16), n_runs, tiles are functions of the HISTOGRAM of the counts and come from the host
 *   (vadx.ragged.stream_plan: one bincount, no sort), as does bucket_first int32 [max_windows + 2], bucket_first[c] = the number of
 *   streams with a count above c = the first sorted position of count c;
 *   the per-stream tables are written on the device by vadx_silero_stream_plan from counts int32 [S] and bucket_first: probs_first
 *   int64 [S + 1], the exclusive prefix of the counts in stream order, and over the 16 * groups slots slot_clip = the streams with n_s > 0
 *   sorted by count, descending and stable -- exactly numpy's argsort(-counts, kind="stable") restricted to them; -1 in the empty slots --,
 *   slot_off = stream * L with L = cw + max_windows * window (the staged row), slot_len = cw + n_s * window.  A counting sort (ranks of
 *   equal keys from wave ballots, per-block key histograms, a prefix over the blocks) whose result does not depend on the order in which
 *   anything executes: which stream sits in which slot decides who shares a poisoned fp16 x 2 workgroup.  A count outside
 *   [0, max_windows] is taken as 0 and bit 1 of *status is raised; so is a slot position outside the tables, which is not written.
 *   Scratch: vadx_silero_stream_plan_bytes(S, max_windows), the FIRST bytes of the tick workspace
 *   (vadx_silero_stream_ragged_workspace_bytes(S, max_windows, tiles) = that + the staged rows + the initial states + tiles x 32 KB), so
 *   the plan and the tick take the same workspace pointer; the plan alone needs only its own part.  window: 512 or 256.
 * vadx_silero_stream_run_ragged: arguments as vadx_silero_stream_run, except samples [S][row_stride] with n_s * window valid per row
 * (row_stride >= max_windows * window), max_windows and the table set in place of `windows`, no `active`.  probs, event_kind and
 * event_value are PACKED vectors [probs_first[S]], stream s owns probs_first[s] .. probs_first[s + 1].  A reset applies to a stream with
 * n_s > 0 only; an idle stream's state_out record is a bitwise copy of state_in and nothing else of it is touched or computed.  The new
 * context is the last cw samples of the stream's own n_s windows.  Record format, NaN poisoning and the range protocol are
 * vadx_silero_stream_run's: a record written by either call continues under the other, and per stream the scores are bit for bit those
 * of vadx_silero_clips over the concatenated audio.  A workspace below vadx_silero_stream_ragged_workspace_bytes(S, max_windows,
 * rg->tiles) returns VADX_ENOSPACE (a tick is not run in parts).  Stream-ordered after the plan: stage, encode, recur, events. */
int    vadx_silero_stream_ragged_max_windows(void);                                   /* 256 */
size_t vadx_silero_stream_plan_bytes(int streams, int max_windows);                  /* 0 for arguments out of range */
size_t vadx_silero_stream_ragged_workspace_bytes(int streams, int max_windows, int64_t tiles);
int vadx_silero_stream_plan(const int32_t *counts, const int32_t *bucket_first, int streams, int max_windows, int window, int groups,
                            int64_t *probs_first, int64_t *slot_off, int32_t *slot_len, int32_t *slot_clip, uint32_t *status,
                            void *workspace, size_t workspace_bytes, void *stream);
int vadx_silero_stream_run_ragged(const float *packed, const vadx_silero_iter_params *prm,
                                  const void *samples, int samples_int16, float scale, int64_t row_stride,
                                  int streams, int max_windows, const vadx_silero_ragged *rg, const uint8_t *reset,
                                  const void *state_in, void *state_out,
                                  float *probs, int8_t *event_kind, double *event_value,
                                  void *workspace, size_t workspace_bytes, void *stream, const vadx_silero_cfg *cfg);

/* ---------------------------------------------------------------------------------------------
 * Fused signal front-end: int16 PCM -> prep -> framed windowed DFT against the
 * reference's own float32 table -> |.|^2 -> mel -> log.
 * Replaces the graph prefix every exported model starts with:
 *   FSMN      FSMN/Export_FSMN_VAD.py:76-81      + FSMN/STFT_Process.py:144-157
 *   MarbleNet Export_NVIDIA_MarbleNet_VAD.py:236-262 + NVIDIA_.../STFT_Process.py:265-279
 *   FireRed   FireRedVAD/Export_FireRedVAD.py:428-461 + FireRedVAD/STFT_Process.py (same class)
 *   DFSMN     DFSMN/.../Export_DFSMN_VAD.py:318-325,342-348 + DFSMN/.../STFT_Process.py:154-172
 * ------------------------------------------------------------------------------------------- */
typedef struct vadx_frontend_cfg {
    int   prep;        /* 0: x-mean(window), then y[n]=a[n]-0.97*a[n-1], y[0]=a[0]        (FSMN)
                          1: y[n]=k0*x[n-1]+k1*x[n], x[-1]=0                             (MarbleNet, FireRed)
                          2: y = k1*x - mean(k1*x)                                       (DFSMN STFT-B)
                          3/4/5: DFSMN feature streams, see vadx_frontend_logmel_ex
                          6: linear resample (in_window_len -> window_len samples), THEN prep 1   (IN_SAMPLE_RATE > 16000)
                          7: prep 1 at the input rate, THEN linear resample                    (IN_SAMPLE_RATE < 16000)
                             = F.interpolate(mode='linear', align_corners=False) of the exports built for another input
                             rate (Export_NVIDIA_MarbleNet_VAD.py:237-254, FireRedVAD/Export_FireRedVAD.py:431-449) */
    float k0, k1;
    int   center_pad;  /* zeros on each side of the window (n_fft/2, or 0 for snip-edges) */
    int   tap0, taps;  /* non-zero span of the centre-padded analysis window inside n_fft */
    int   hop;         /* multiple of 16, <= 320, and taps <= 4 * hop (at most four hops per analysis window): any other geometry is REFUSED
                          (vadx_frontend_packed_floats returns 0, the other entry points VADX_EINVAL) -- there is no slower generic path */
    int   n_bins;      /* n_fft/2+1 */
    int   n_mels;      /* multiple of 16 */
    int   log_mode;    /* 0: log(max(x,floor))   1: log(x+floor) */
    float log_floor;
    int   frames;      /* frames per window */
    int   window_len;  /* samples per window (at 16 kHz, i.e. after the in-graph resample of prep 6 / 7) */
    int   in_window_len; /* prep 6 / 7: samples per window in the audio buffer (input rate); 0 otherwise */
    float rs_scale;    /* prep 6 / 7: source samples per output sample, float32(1 / scale_factor) as torch computes it */
    int   fold;        /* the DFT product of vadx_frontend_logmel / _logmel_means, one of VADX_FE_KIND_* below; set it before
                          vadx_frontend_packed_floats / _pack_host (the blob's layout depends on it).  _logmel_ex and _stft_ft ignore
                          it: they run the dense kernels on the dense tables, which every blob carries */
} vadx_frontend_cfg;

/* vadx_frontend_cfg.fold.  A geometry a kind does not take is refused like any other (packed_floats 0, VADX_EINVAL); a TABLE a fold
 * does not admit is refused by _pack_host. */
#define VADX_FE_KIND_DENSE    0   /* float32 product: any geometry the front-end takes */
#define VADX_FE_KIND_FOLD_SYM 1   /* mirror fold: taps paired about the window centre + an f16 residual, same table bits, half the f32 */
#define VADX_FE_KIND_FOLD_PER 2   /* MFMAs; centre of a symmetric (1) / periodic (2) window.  Preps 0 - 2, 6, 7; <= 257 bins; hop >= 32.
                                     Use the one vadx_frontend_fold_kind answers for the table */
#define VADX_FE_KIND_FOLD_TF  3   /* opt-in: periodic windows centred on n_fft/2 only (FSMN), time x frequency fold, a quarter of the dense
                                     MACs, noisier on bands far below the frame's peak (csrc/frontend.hip "kind 3") */
#define VADX_FE_KIND_SPLIT_B3 4   /* dense product of the reference table itself on bf16 x 3 exactly split operands (csrc/split3.h: six
                                     bf16 MFMAs per 32 taps, float32-class accuracy, no symmetry assumption); hop 160, preps 0 - 2,
                                     taps <= 512, <= 272 bins */
#define VADX_FE_KIND_SPLIT_H2 5   /* the same on fp16 x 2 split operands (csrc/split2.h; the samples are pre-scaled exactly into the
                                     fp16 range; _pack_host refuses a table entry outside it) -- the Python front-end's default where
                                     it applies */

/* Which mirror fold the reference's windowed DFT table admits for this geometry -- VADX_FE_KIND_FOLD_SYM, _FOLD_PER, or 0 for neither:
 * the table must equal, about the window centre, an even real / odd imaginary pair to within what the f16 residual carries (1.5e-4 of
 * the table scale). */
int vadx_frontend_fold_kind(const vadx_frontend_cfg *cfg, const float *cos_tab, const float *sin_tab, int n_fft);


size_t vadx_frontend_packed_floats(const vadx_frontend_cfg *cfg);
/* Host repack of the reference tables (cos/sin [n_bins][n_fft] windowed, fbank [n_mels][n_bins]);
 * mel_kb receives 2*n_mels/16 ints (banded mel ranges) that vadx_frontend_logmel wants back. */
int vadx_frontend_pack_host(const vadx_frontend_cfg *cfg, const float *cos_tab, const float *sin_tab,
                            int n_fft, const float *fbank, float *packed_host, int32_t *mel_kb);
/* audio int16 [batch][row_stride]; window w of clip b starts at b*row_stride + w*win_stride;
 * out f32 [batch*windows_per_clip][frames][n_mels]; means_ws: batch*windows floats (prep 0/2). */
int vadx_frontend_logmel(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host,
                         const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch,
                         int windows_per_clip, float *means_ws, float *out, void *stream);
/* vadx_frontend_logmel with the window means (prep 0 / 2) GIVEN by the caller instead of computed into a workspace, and the kernel that
 * computes them (mean of scale * x over each window: exact integer sum, one float32 rounding). */
int vadx_frontend_logmel_means(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host,
                               const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch,
                               int windows_per_clip, const float *means, float *out, void *stream);
int vadx_frontend_window_means(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                               int window_len, float scale, float *means, void *stream);

/* DFSMN variants of the fused front-end (DFSMN/.../Export_DFSMN_VAD.py:322-325, 338-348):
 *   prep 3: near stream  a = k1*x - mean, pre-emphasis 0.97 keeping a[0]        (int16 source + means)
 *   prep 4: AEC stream   pre-emphasis of the float waveform `faux` [windows][window_len]
 *   prep 5: echo stream  near_pe - k0 * aec_pe                                  (both sources)
 * Each call writes n_mels columns at `out_off` of rows of `out_stride` floats (3 calls fill the 240-dim row). */
int vadx_frontend_logmel_ex(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host,
                            const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch,
                            int windows_per_clip, const float *means, const float *faux, int out_stride,
                            int out_off, float *out, void *stream);
/* Raw complex STFT (prep 2) into a frame-tiled tensor [window*ceil(frames/16) + t/16][c_total][n_bins][16]:
 * real part at channel c_off, imaginary at c_off+1 (the two-stream STFT-B of DFSMN_VAD.forward :322-325). */
int vadx_frontend_stft_ft(const vadx_frontend_cfg *cfg, const float *packed, const int16_t *audio,
                          int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                          float *means_ws, float *ft_out, int c_total, int c_off, void *stream);

/* ---------------------------------------------------------------------------------------------
 * FSMN-VAD
 * ------------------------------------------------------------------------------------------- */
typedef struct vadx_fsmn_dims {          /* FunASR FSMN(input 400, proj 128, lorder 20, 4 layers pinned in-tree) */
    int   input_affine_dim, linear_dim, output_affine_dim, output_dim;   /* external config: 140/250/140/248 */
    int   frames;                         /* T = window_len // 160 + 1 (101); vadx_fsmn_run takes T <= 128 (window_len <= 20479), the clips, ragged
                                           * and stream entry points T <= 112 (window_len <= 17919); more is VADX_EINVAL there.  The *_long
                                           * entry points take T <= VADX_FSMN_LONG_MAX_FRAMES */
    float speech_2_noise_ratio;           /* FSMN/Export_FSMN_VAD.py:34,87-92 */
    int   arithmetic;                     /* VADX_ARITH_* of the dense layers (0 = AUTO = BF16X3: float32's exponent range, nothing to check; F16X2
                                           * is for callers that read vadx_fsmn_range_flag with the results and recompute a flagged batch on
                                           * BF16X3, as vadx.fsmn.FsmnEngine does).  The packed blob carries the weight fragments of THIS
                                           * arithmetic only: pass the same dims to vadx_fsmn_pack_host and to every launch.  pack_host refuses
                                           * F16X2 when a weight lies outside the fp16 range (pack BF16X3 then). */
} vadx_fsmn_dims;

typedef struct vadx_fsmn_weights_host {  /* torch layouts: Linear weight [out][in]; conv_left [128][20] */
    const float *in1_w, *in1_b, *in2_w, *in2_b;
    const float *lin_w[4], *fir_w[4], *aff_w[4], *aff_b[4];
    const float *out1_w, *out1_b, *out2_w, *out2_b;
    const float *cmvn_means, *cmvn_vars;  /* [400] each, (x + means) * vars */
} vadx_fsmn_weights_host;

size_t vadx_fsmn_packed_floats(const vadx_fsmn_dims *dims);
/* The F16X2 kernels' sticky range flag, as vadx_silero_range_flag: flag != 0 = an activation of some launch since the last reset left the
 * fp16 range and that launch's results must be recomputed with a BF16X3 blob.  Synchronises `stream`. */
int vadx_fsmn_range_flag(const vadx_fsmn_dims *dims, const float *packed, int reset, uint32_t *flag_host, float *amax_host, void *stream);
int vadx_fsmn_pack_host(const vadx_fsmn_dims *dims, const vadx_fsmn_weights_host *w, float *packed_host);

/* Per-frame energy term of the score gate: log10(sum_512 (y/(sqrt(L)*2e-5))^2 + 2e-5) of the prepped
 * window, 97 real frames + last value repeated to `frames`; means = per-window DC (from
 * vadx_frontend_logmel's means workspace).  Replaces FSMN/Export_FSMN_VAD.py:93-97. */
int vadx_fsmn_energy(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch,
                     int windows_per_clip, int window_len, int frames, const float *means, float *db,
                     void *stream);
/* The window means (prep 0: exact integer sum / window_len, what vadx_frontend_logmel computes into its workspace) AND the energy term above
 * in ONE pass over the PCM: means f32 [batch*windows_per_clip], db f32 [batch*windows_per_clip][frames].  Feed the means to
 * vadx_frontend_logmel_means.  (Windows that do not start on 16-byte boundaries or whose length is not a multiple of 32 take the two
 * separate kernels.)  Replaces nothing more than vadx_fsmn_energy does: FSMN/Export_FSMN_VAD.py:76-79, 93-97. */
int vadx_fsmn_window_stats(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                           int window_len, int frames, float *means, float *db, void *stream);

/* One ORT-boundary call for `batch` independent streams, after the front-end:
 *   feeds   audio -> (logmel [B][T][80], db [B][T]); cache_0..3 f32 [B][128][19];
 *           one_minus_speech_threshold f32 [B]; noise_average_dB f32 [B]
 *   fetches score u8 [B][T]; cache_0..3; noisy_dB f32 [B]      (+ optional P(silence) f32 [B][T])
 * dims->frames <= 128: the kernel keeps a window's scores in a 128-entry LDS array; a longer window returns VADX_EINVAL before any device call.
 * Replaces ort_session_A.run(...), FSMN/Inference_FSMN_VAD_ONNX.py:177-187 (graph :75-101). */
int vadx_fsmn_run(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                  const float *const cache_in[4], float *const cache_out[4], const float *thr,
                  const float *noise_db, int batch, uint8_t *score, float *noisy_db, float *psil,
                  void *stream);

typedef struct vadx_fsmn_loop_params {   /* FSMN/Inference_FSMN_VAD_ONNX.py:16-23,79-81,159-171 */
    int    look_backward;                 /* frames: int(LOOK_BACKWARD*16000 // 160) = 30; 0 is allowed and means what it
                                           * means in the reference: slide_range = T, one-frame vote, empty tail */
    float  one_minus_speech_threshold;    /* 1.0 */
    float  noise_db_init;                 /* (BACKGROUND_NOISE_dB_INIT + SNR_THRESHOLD) * 0.1 */
    float  snr_threshold;                 /* SNR_THRESHOLD * 0.1 */
    double speaking_score, silence_score; /* 0.5, 0.5 */
} vadx_fsmn_loop_params;

/* Whole clips: every clip's windows in order with cache + noise-floor carry and the look-ahead
 * vote; flags u8 [B][W*(T-lb) + lb] = the reference's `saved` list (1 = silence).
 * cache_ws: scratch of B*4*128*19 floats.  noise_trace (optional) [B][W] = noise floor after each window.
 * Replaces the while-loop + tail, FSMN/Inference_FSMN_VAD_ONNX.py:176-234. */
int vadx_fsmn_clips(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                    int batch, int windows_per_clip, const vadx_fsmn_loop_params *lp, float *cache_ws,
                    uint8_t *flags, float *noise_trace, void *stream);

/* Streaming FSMN (ABI 10): S live streams advance by `windows` analysis windows per tick; what the reference loop carries from window to
 * window -- the four FIR caches, the noise floor it feeds back, the vote's `silence` and the (look_backward + 1) * 160 samples two
 * consecutive windows share -- lives in a device RECORD of vadx_fsmn_stream_state_bytes(S, look_backward) bytes.  The record is opaque
 * except that
 *   - its first S*4*128*19 floats are the caches [S][4][128][19] (cache_0..3 of vadx_fsmn_run, per stream);
 *   - a record of all zero bytes is S streams in their reset state (no init call);
 *   - its size is a multiple of 16 bytes; records are 16-byte aligned.
 * It also carries a 64-bit count of the windows each stream has done since its reset (the host turns flag positions into times with it).
 * One tick is four calls on one HIP stream, the middle two unchanged:
 *   vadx_fsmn_stream_windows   samples + carry -> window_buf int16 [S*windows][window_len], the new carry
 *   vadx_fsmn_window_stats     on window_buf with batch = S, windows_per_clip = windows, row_stride = windows * window_len, win_stride = window_len
 *   vadx_frontend_logmel_means the same arguments
 *   vadx_fsmn_stream_run       the window loop -> flags, tail, the rest of the record
 * Both stream calls of a tick take the SAME state_in, state_out, reset and active.  state_in is never written (a tick can be recomputed
 * from it, which the range protocol needs); state_in and state_out must not overlap.  vadx_fsmn_stream_windows writes only the carry and
 * the "has a carry" word of state_out, vadx_fsmn_stream_run everything else.
 * reset (NULL or uint8 [S]): != 0 = back to the reset state before this tick.  active (NULL or uint8 [S]): 0 = no audio for this stream
 * this tick -- its record in state_out is a bitwise copy of state_in's (a reset request on an inactive stream is ignored), its flags and
 * tail are 255 and its noise_trace NaN.
 * Range protocol per tick: with VADX_ARITH_F16X2 dims read vadx_fsmn_range_flag after vadx_fsmn_stream_run and, when it is raised, call
 * vadx_fsmn_stream_run again with the BF16X3 dims and blob on the same arguments (same state_in, same state_out, same logmel / db):
 * every byte the first call wrote is written again.  The window and front-end calls do not depend on the arithmetic.
 * The flags are bit for bit those of vadx_fsmn_clips over the concatenated audio. */

/* Bytes of the record of `streams` streams (0 for streams <= 0 or look_backward < 0). */
size_t vadx_fsmn_stream_state_bytes(int streams, int look_backward);

/* Window assembly.  stride = window_len - (look_backward + 1) * 160.  samples int16 [S][row_stride] holds each stream's NEW samples from
 * column 0: windows * stride of them for a stream that has a carry, window_len + (windows - 1) * stride for one that has none (zero
 * record, or reset this tick) -- the caller sizes every row for the streams it knows to be in that state; row_stride >= windows * stride
 * is all this call can check.  Window j of a stream is [j * stride, j * stride + window_len) of (carry ++ new samples); the last
 * (look_backward + 1) * 160 samples become the carry in state_out.  An inactive stream's windows are zeros.  samples, window_buf and the
 * records 16-byte aligned, row_stride a multiple of 8.  Returns VADX_EINVAL for a NULL pointer, windows < 1, look_backward outside
 * [0, window_len / 160 + 1) or leaving no stride, or overlapping records.
 * Replaces the slicing `audio[..., slice_start:slice_end]` + `slice_start += stride_step` of FSMN/Inference_FSMN_VAD_ONNX.py:162-167,
 * 176-234 for audio that arrives in pieces. */
int vadx_fsmn_stream_windows(const int16_t *samples, int64_t row_stride, int streams, int windows, int window_len,
                             int look_backward, const uint8_t *reset, const uint8_t *active,
                             const void *state_in, void *state_out, int16_t *window_buf, void *stream);

/* The window loop of one tick, one workgroup per stream: logmel [S*windows][T][80] and db [S*windows][T] are the front-end over
 * window_buf.  flags u8 [S][windows * (T - look_backward)]: the voted silence flags of this tick's windows (1 = silence), the next
 * entries of the reference's `saved` list.  tail u8 [S][look_backward] (may be NULL when look_backward = 0): what the plain rule appends
 * if the stream ENDS with this tick; it does not touch the carried vote state, so the stream can go on.  noise_trace (optional)
 * [S][windows] = noise floor after each window.  lp as for vadx_fsmn_clips; 0 <= look_backward < T - 2.  Returns VADX_EINVAL for a NULL
 * pointer, windows < 1, look_backward out of range, or overlapping records.
 * Replaces the while-loop body + tail, FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234, for S streams that arrive in pieces. */
int vadx_fsmn_stream_run(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                         int streams, int windows, const vadx_fsmn_loop_params *lp,
                         const uint8_t *reset, const uint8_t *active, const void *state_in, void *state_out,
                         uint8_t *flags, uint8_t *tail, float *noise_trace, void *stream);

/* RAGGED ticks of the FSMN streams: stream s advances by counts[s] windows this tick, 0 <= counts[s] <= max_windows <=
 * vadx_fsmn_stream_ragged_max_windows() = 256 (no kernel resource depends on a count, so the cap is the Silero ragged tick's; longer
 * catch-ups go through vadx_fsmn_stream_run).  The work is sum(counts) windows, not S * k: a stream with count 0 owns no window row and
 * costs no front-end and no network time.  The RECORD is the one above -- same layout, same size, zero bytes = reset, state_in never
 * written, two records ping-ponged -- so the two tick forms interchange tick by tick.  The tick is the sequence above with two new ends:
 *   vadx_fsmn_stream_windows_ragged   samples + carries -> window_buf int16 [n_windows][window_len], the new carries
 *   vadx_fsmn_window_stats            batch = n_windows, windows_per_clip = 1, row_stride = win_stride = window_len
 *   vadx_frontend_logmel_means        the same arguments
 *   vadx_fsmn_stream_run_ragged       the window loop per stream -> flags, tails, the rest of the record
 * Both new calls take the same tables, reset, state_in, state_out and status:
 *   counts    int32 [S]       windows of each stream this tick; 0 = no audio (there is no `active` argument): the stream's record in
 *                             state_out is a bitwise copy of state_in's, a reset request for it is ignored, its tail reads 255;
 *   win_first int32 [S + 1]   prefix sum of counts; n_windows = win_first[S].  Window j of stream s is row win_first[s] + j of window_buf,
 *                             logmel, db, flags and noise_trace;
 *   status    uint32 [1]      zeroed by the caller.  The tables are device memory the library cannot read on the host: a stream whose
 *                             count lies outside [0, max_windows], or whose win_first entries do not span exactly its count inside
 *                             [0, n_windows], COUNTS AS 0 (record copied, no flags, tail 255) and raises bit 1 (value 2) of *status;
 *                             nothing is indexed out of bounds and no other stream changes.
 * Per-stream results depend on nothing but that stream's record and audio: not on `order`, S, its neighbours or where its rows lie.
 * Range protocol as for the rectangular tick: with F16X2 dims read vadx_fsmn_range_flag after vadx_fsmn_stream_run_ragged and, when it is
 * raised, call it again with the BF16X3 dims and blob on the same arguments; every byte the first call wrote is written again.
 * Both return VADX_EINVAL, with a message that names the argument and before any HIP call, for a NULL pointer (reset, order and
 * noise_trace may be NULL; tail when look_backward = 0), streams, n_windows or max_windows < 1, max_windows above the cap, a look_backward
 * that leaves no stride, a row_stride below max_windows * stride, and misaligned or overlapping records. */
int vadx_fsmn_stream_ragged_max_windows(void);                                          /* 256 */

/* Window assembly of a ragged tick.  samples int16 [S][row_stride] holds each stream's NEW samples from column 0: n_s * stride for a
 * stream with a carry, window_len + (n_s - 1) * stride for one without (zero record, or reset this tick) -- as for
 * vadx_fsmn_stream_windows the caller sizes the rows for the streams it knows to be in that state; row_stride >= max_windows * stride
 * is what this call can check.  A stream's timeline is its carry followed by its new samples; window j = timeline[j * stride, j * stride +
 * window_len) goes to row win_first[s] + j, and the new carry is the last (look_backward + 1) * 160 samples of THAT stream's timeline of
 * n_s windows.  A stream with count 0 keeps its carry and its "has a carry" word bit for bit.  win_stream int32 [n_windows] names the
 * stream of each window row (the counts repeated; the caller uploads it with them); a row whose entry does not agree with win_first is
 * left unwritten.  16-byte runs: samples, window_buf and the records 16-byte aligned, row_stride and window_len multiples of 8.
 * Replaces the slicing of FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234 for streams that deliver different amounts of audio. */
int vadx_fsmn_stream_windows_ragged(const int16_t *samples, int64_t row_stride, int streams, int n_windows, int max_windows,
                                    int window_len, int look_backward, const int32_t *counts, const int32_t *win_first,
                                    const int32_t *win_stream, const uint8_t *reset, const void *state_in, void *state_out,
                                    int16_t *window_buf, uint32_t *status, void *stream);

/* The window loop of a ragged tick, one workgroup per stream; workgroup i serves stream order[i] (int32 [S], optional: streams with
 * audio by count descending, idle streams last; NULL = identity).  An order entry outside [0, S) makes its workgroup return at once
 * (and raises bit 1 of *status); a stream no entry names is not served -- nothing of it is written by this call.  The workgroup of a
 * stream with n_s > 0 runs n_s iterations of exactly the loop body of vadx_fsmn_stream_run (one __device__ function, shared).
 * flags u8 [n_windows][T - look_backward]: stream s owns rows win_first[s] .. win_first[s+1] - 1.  tail u8 [S][look_backward] (may be
 * NULL when look_backward = 0): written on the stream's OWN last window of this tick; 255 for a stream without audio.  noise_trace
 * (optional) f32 [n_windows].  The windows-done word advances by n_s.
 * Replaces the while-loop body + tail, FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234, for streams that advance by different amounts. */
int vadx_fsmn_stream_run_ragged(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                                int streams, int n_windows, int max_windows, const vadx_fsmn_loop_params *lp,
                                const int32_t *counts, const int32_t *win_first, const int32_t *order, const uint8_t *reset,
                                const void *state_in, void *state_out, uint8_t *flags, uint8_t *tail, float *noise_trace,
                                uint32_t *status, void *stream);

/* Ragged batches (FSMN, FireRed): B clips of ANY lengths in one launch sequence, work proportional to the sum of their windows.
 * The caller pads every clip to its own window grid on the host (the reference's tail-noise rule, FSMN/Inference_FSMN_VAD_ONNX.py:88-99 /
 * FireRedVAD/Inference_FireRed_ONNX.py:546-558), lays the padded clips end to end in ONE int16 vector `pcm` -- every clip starting on a
 * multiple of 8 samples (16 bytes) -- and describes it with three tables (vadx.ragged.RaggedBatch builds all of this):
 *   win_first int32 [B+1]   prefix sum of W_b, the windows per clip: clip b owns windows win_first[b] .. win_first[b+1]-1 of every
 *                           per-window buffer below (n_windows = win_first[B]);
 *   win_src   int64 [n_windows]   sample offset of each window in pcm: clip_off[b] + k * stride (stride = window_len for FireRed);
 *   order     int32 [B]     clips by W_b descending: the launch order of the one-workgroup-per-clip FSMN kernel (optional).
 * The PCM crosses the host link once, without the overlap of the windows and without the padding a rectangular [B][max N] batch has.
 * FSMN sequence on one HIP stream:
 *   vadx_windows_gather        pcm, win_src -> window_buf int16 [n_windows][window_len]
 *   vadx_fsmn_window_stats     on window_buf with batch = n_windows, windows_per_clip = 1, row_stride = win_stride = window_len
 *   vadx_frontend_logmel_means the same arguments
 *   vadx_fsmn_clips_ragged     -> flags u8 [B][flag_stride]
 * FireRed sequence: vadx_windows_gather, vadx_frontend_logmel (batch = n_windows, windows_per_clip = 1), vadx_firered_run (windows =
 * n_windows), then per output channel vadx_tracks_gather + vadx_vadpost.  The front-end and network calls are the unchanged ones. */

/* window_buf int16 [n_windows][window_len]: row w = pcm[win_src[w], win_src[w] + window_len).  One workgroup per window, 16-byte runs:
 * window_len and every offset are multiples of 8 samples, pcm and window_buf 16-byte aligned.  A window whose source range leaves
 * [0, pcm_len) -- or whose offset is not a multiple of 8 -- is written as ZEROS; nothing outside pcm is ever read.  Returns VADX_EINVAL
 * for a NULL pointer, n_windows < 1, pcm_len < 1, a window_len that is not a positive multiple of 8, or misaligned buffers.
 * Replaces the slicing `audio[..., slice_start:slice_end]` of FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234 and of the chunk loop
 * FireRedVAD/Inference_FireRed_ONNX.py:560-579, for every window of every clip at once. */
int vadx_windows_gather(const int16_t *pcm, int64_t pcm_len, const int64_t *win_src, int n_windows, int window_len,
                        int16_t *window_buf, void *stream);

/* vadx_fsmn_clips over a ragged batch: the same window loop (one device function, shared), per-clip bounds.  Workgroup i serves clip
 * b = order[i] (order NULL = identity; order MUST be a permutation of 0 .. batch-1 -- documented, not checked: a clip named twice is
 * computed twice by racing workgroups, a clip never named keeps its 255 row).  logmel [n_windows][T][80], db [n_windows][T]: the
 * front-end over window_buf.  Row b of flags u8 [batch][flag_stride]: its first W_b * (T - look_backward) + look_backward entries are
 * the reference's `saved` list of clip b (1 = silence), bit for bit what vadx_fsmn_clips gives for that clip alone; every other entry
 * is 255, the stream API's "no flag" (the call fills flags with 255 first, on `stream`).  noise_trace (optional) f32 [n_windows] = noise
 * floor after each window.  cache_ws: scratch of batch*4*128*19 floats.  max_windows: the largest W_b the caller sized flag_stride for.
 * A table entry that does not describe windows inside the buffers -- W_b <= 0, W_b > max_windows, win_first[b] < 0, win_first[b+1] >
 * n_windows, order[i] outside [0, batch) -- makes that workgroup return at once: the row stays all 255, its noise_trace entries are
 * not written, nothing is indexed out of bounds.  Returns VADX_EINVAL, before any HIP call, for a NULL pointer (order and noise_trace
 * may be NULL), batch / n_windows / max_windows < 1, flag_stride < max_windows * (T - look_backward) + look_backward, or a
 * look_backward outside [0, T).  All three arithmetics; with F16X2 dims the range flag is raised as by vadx_fsmn_clips (range protocol:
 * read vadx_fsmn_range_flag, repeat this call with the BF16X3 dims and blob when it is raised).
 * Replaces the while-loop + tail, FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234, for B files of different lengths. */
int vadx_fsmn_clips_ragged(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int batch,
                           int n_windows, int max_windows, const int32_t *win_first, const int32_t *order,
                           const vadx_fsmn_loop_params *lp, float *cache_ws, uint8_t *flags, int64_t flag_stride, float *noise_trace,
                           void *stream);

/* Long windows (FSMN, opt-in): INPUT_AUDIO_LENGTH is a plain constant of FSMN/Export_FSMN_VAD.py which the driver reads back from the
 * session (FSMN/Inference_FSMN_VAD_ONNX.py:73-80); an export at 160 000 scores a 10 s clip as ONE window of 1 001 frames.  The entry
 * points above keep a window's scores in LDS and stop at 128 / 112 frames; the three below take any 1 <= frames <=
 * VADX_FSMN_LONG_MAX_FRAMES (a 10-minute window, window_len <= 9 600 000; longer audio goes on the window grid).  One workgroup still
 * walks a window tile by tile with the FIR caches carried from tile to tile; the window's P(silence) and gate bits live in `workspace`
 * rows (8 bytes per frame, read back by the workgroup that wrote them).  At frames <= 112 the results are bit for bit those of the
 * entry points above.  Same dims, blob, arithmetics and range protocol.  Each returns VADX_EINVAL with a message that names the
 * argument, before any HIP call, for a NULL pointer or workspace, frames out of range, or counts that do not fit each other.
 * Plain-C sequence for B padded clips of W windows: vadx_fsmn_window_stats_long, vadx_frontend_logmel_means (unchanged),
 * vadx_fsmn_clips_long with win_first = NULL. */
#define VADX_FSMN_LONG_MAX_FRAMES 60001
/* Bytes of `workspace` for vadx_fsmn_run_long (rows = batch) and vadx_fsmn_clips_long (rows = clips); 0 for rows < 1 or frames outside
 * [1, VADX_FSMN_LONG_MAX_FRAMES].  Contents need no initialisation and carry nothing between calls. */
size_t vadx_fsmn_long_workspace_bytes(int rows, int frames);
/* vadx_fsmn_window_stats for windows of any length >= 512 and any alignment, with a grid of (window, block of frames) so that a single
 * long window fills the chip (vadx_fsmn_window_stats gives a window above 16 384 samples to one workgroup, twice).  means: the exact
 * 64-bit integer sum, one float32 rounding -- bit for bit vadx_frontend_window_means; db: vadx_fsmn_energy's per-sample expression in
 * another summation order (float32 rounding apart).  workspace: 8 bytes per window, 8-byte aligned (vadx_fsmn_long_workspace_bytes(
 * batch * windows_per_clip, frames) is more than enough).  VADX_EINVAL also for a row_stride that does not hold the windows.
 * Replaces what vadx_fsmn_window_stats does, FSMN/Export_FSMN_VAD.py:76-79, 93-97, for the window of a long export. */
int vadx_fsmn_window_stats_long(const int16_t *audio, int64_t row_stride, int64_t win_stride, int batch, int windows_per_clip,
                                int window_len, int frames, float *means, float *db, void *workspace, void *stream);
/* vadx_fsmn_run for dims->frames up to VADX_FSMN_LONG_MAX_FRAMES: same feeds and fetches; with psil the window's P(silence) is written
 * straight to it.  workspace: vadx_fsmn_long_workspace_bytes(batch, dims->frames) bytes, 4-byte aligned.
 * Replaces ort_session_A.run(...), FSMN/Inference_FSMN_VAD_ONNX.py:177-187, for a long export. */
int vadx_fsmn_run_long(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db,
                       const float *const cache_in[4], float *const cache_out[4], const float *thr, const float *noise_db, int batch,
                       uint8_t *score, float *noisy_db, float *psil, void *workspace, void *stream);
/* vadx_fsmn_clips_ragged for dims->frames up to VADX_FSMN_LONG_MAX_FRAMES, and vadx_fsmn_clips too: win_first == NULL is the rectangular
 * batch, max_windows windows for every clip (n_windows = batch * max_windows, logmel / db / noise_trace [batch][max_windows], flags
 * [batch][flag_stride] with flag_stride >= max_windows * (T - look_backward) + look_backward).  With win_first the tables, the 255
 * fill and the guard are vadx_fsmn_clips_ragged's: a lying entry leaves its row of 255s and touches nothing; batch <= n_windows <=
 * batch * max_windows.  look_backward in [0, frames - 1): the windows of a grid must advance.  workspace:
 * vadx_fsmn_long_workspace_bytes(batch, dims->frames) bytes, 4-byte aligned.
 * Replaces the while-loop + tail, FSMN/Inference_FSMN_VAD_ONNX.py:176-234, for a long export. */
int vadx_fsmn_clips_long(const vadx_fsmn_dims *dims, const float *packed, const float *logmel, const float *db, int batch,
                         int n_windows, int max_windows, const int32_t *win_first, const int32_t *order,
                         const vadx_fsmn_loop_params *lp, float *cache_ws, uint8_t *flags, int64_t flag_stride, float *noise_trace,
                         void *workspace, void *stream);

/* Per-window scores -> one track per clip.  probs f32 [n_windows][win_floats]; a window's `frames_per_window` scores of interest start
 * at float `chan_offset` of its row (FireRed: probs [n_windows][odim][T], win_floats = odim * T, channel c = chan_offset / T).  Row b
 * of tracks f32 [batch][track_stride] receives the first min(n_frames[b], W_b * frames_per_window, track_stride) frames of clip b's
 * windows laid end to end (W_b = win_first[b+1] - win_first[b]; a negative win_first[b] or W_b counts as no frames), zeros after them:
 * the [B][stride] + n_frames[B] input of vadx_vadpost.  win_first must be the table probs was computed with -- this call does not know
 * n_windows.  Returns VADX_EINVAL for a NULL pointer, batch / track_stride / frames_per_window < 1 or a channel range outside
 * [0, win_floats).  Replaces np.concatenate(all_probs)[:num_valid_frames], FireRedVAD/Inference_FireRed_ONNX.py:560-579 (AED
 * :661-683), for a plain-C caller that has no tensor library to index with. */
int vadx_tracks_gather(const float *probs, int64_t win_floats, int chan_offset, int frames_per_window, const int32_t *win_first,
                       const int32_t *n_frames, int batch, float *tracks, int track_stride, void *stream);

/* ---------------------------------------------------------------------------------------------
 * FireRedVAD / FireRedAED DetectModel and VadPostprocessor (row a16)
 * ------------------------------------------------------------------------------------------- */
typedef struct vadx_firered_cfg {        /* checkpoint `args` (FireRedVAD/Export_FireRedVAD.py:336-337) */
    int idim, R, M, H, P, N1, S1, N2, S2, odim;
    int frames;                           /* frames per window: (L-400)//160+1 = 98 */
    /* Limits (a cfg outside them: vadx_firered_packed_floats returns 0, every other entry point VADX_EINVAL): idim = 80; 1 <= R <= 16; 1 <= M <= 4; 1 <= H <= 256;
     * 1 <= P <= 128; 1 <= N1 <= 32 and 0 <= N2 <= 32 taps at any dilation S1, S2 >= 1 (a filter may reach beyond the window);
     * 1 <= odim <= 4; 1 <= frames <= 112, for a window of vadx_firered_run and for a chunk of vadx_firered_stream_run alike (18 160
     * samples).  tests/test_gpu_firered_shapes.py runs the edges of each. */
    int arithmetic;                       /* VADX_ARITH_* of the point-wise layer pairs (0 = AUTO = BF16X3 where H = 256, P = 128; float32 MFMAs
                                           * elsewhere; F16X2 on request, with vadx_firered_range_flag).  As vadx_fsmn_dims.arithmetic: the blob
                                           * carries the fragments of this arithmetic only. */
} vadx_firered_cfg;

typedef struct vadx_firered_weights_host {   /* torch layouts, 1x1 convs as [out][in] */
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;          /* dfsmn.fc1 (CMVN already folded), dfsmn.fc2 */
    const float *fsmn_lb[16], *fsmn_la[16];              /* [P][N1], [P][N2] depthwise filters per FSMN */
    const float *blk_fc1_w[16], *blk_fc1_b[16], *blk_fc2_w[16];   /* DFSMNBlock r = 1..R-1 (index 0 unused) */
    const float *dnn_w[4], *dnn_b[4];
    const float *out_w, *out_b;
} vadx_firered_weights_host;

size_t vadx_firered_packed_floats(const vadx_firered_cfg *cfg);
/* The F16X2 kernel's sticky range flag, as vadx_silero_range_flag. */
int vadx_firered_range_flag(const vadx_firered_cfg *cfg, const float *packed, int reset, uint32_t *flag_host, float *amax_host, void *stream);
int vadx_firered_pack_host(const vadx_firered_cfg *cfg, const vadx_firered_weights_host *w, float *packed_host);
/* logmel f32 [windows][frames][80] (vadx_frontend_logmel, 'firered' geometry) -> probs f32 [windows][odim][frames].
 * Replaces ort_session_A.run([probs], {audio}), FireRedVAD/Inference_FireRed_ONNX.py:567-572
 * (graph: FireRedVAD/Export_FireRedVAD.py:420-467 after the front-end). */
int vadx_firered_run(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int windows,
                     float *probs, void *stream);

/* ---- FireRed windows of ANY length: the export at any INPUT_AUDIO_LENGTH or with DYNAMIC_AXES = True
 * (FireRedVAD/Export_FireRedVAD.py:29,48,785-807), which the reference's drivers run as ONE window per file
 * (INPUT_AUDIO_LENGTH_RUN = min(3600 s, audio_len): FireRedVAD/Inference_FireRed_ONNX.py:541-547 VAD, :644-650 AED).  A window of T
 * frames no longer lives in one workgroup: the activations live in a caller-owned workspace and the grid is (window, tile of 64
 * frames), R + 1 launches.  A long window is ANOTHER export than the 1 s one: every window edge zero-pads the look-ahead / look-back
 * filters of all R blocks, so fewer edges give other numbers -- not a faster way to the same ones.  Where both apply (T <= 112) the
 * probabilities are bit for bit those of vadx_firered_run. */
#define VADX_FIRERED_LONG_MAX_FRAMES 360000   /* frames of one window: covers 3600 s at 16 kHz (359 998 frames), the reference's cap (:541) */
#define VADX_FIRERED_LONG_TILE       64       /* frames per tile of the long launches and of the snip-edge ragged front-end */

/* The tables of a batch of windows of any lengths (device pointers), in the style of vadx_marblenet_ragged.  Window b (one clip in
 * the dynamic mode, one window of the grid in a static one; :541-547) has T_b = frame_first[b + 1] - frame_first[b] frames, 0 <= T_b <=
 * VADX_FIRERED_LONG_MAX_FRAMES (0: a clip under 400 samples, no frame and no tile), and ceil(T_b / 64) tiles.  A rectangular batch is the same tables
 * with equal counts. */
typedef struct vadx_firered_long_tables {
    const int32_t *frame_first;   /* [clips + 1], frame_first[clips] = frames_total */
    const int32_t *tile_first;    /* [clips + 1], tile_first[clips] = n_tiles */
    const int32_t *tile_clip;     /* [n_tiles]: the window of every tile */
    int32_t clips, n_tiles, frames_total;
} vadx_firered_long_tables;

/* Bytes of the workspace of vadx_firered_run_long: p (two planes) and mem (one), each f32 [P][frames_total] = 3 * P * frames_total
 * floats; 0 for a cfg outside vadx_firered_cfg's limits (cfg->frames aside) or frames_total outside [1, 2^31). */
size_t vadx_firered_long_workspace_bytes(const vadx_firered_cfg *cfg, int64_t frames_total);
/* logmel f32 [frames_total][80] (window b's rows from frame_first[b]: vadx_frontend_logmel at window_len = L for a rectangular batch,
 * vadx_frontend_logmel_ragged_snip for a ragged one) -> probs f32 [odim][frames_total]: output o of window b's frame t at
 * probs[o * frames_total + frame_first[b] + t] -- planes that suit vadx_tracks_gather(probs + o * frames_total, win_floats = 1,
 * frames_per_window = 1, win_first = frame_first), as MarbleNet's ragged scores.  Replaces ort_session_A.run([probs], {audio}) on a
 * dynamic or long export, FireRedVAD/Inference_FireRed_ONNX.py:567-572 (VAD), :668-673 (AED).  The blob is vadx_firered_pack_host's,
 * unchanged; cfg->frames only has to lie in [1, VADX_FIRERED_LONG_MAX_FRAMES] (T comes from the tables).  All three arithmetics under the range
 * protocol as it stands (an F16X2 call that raised vadx_firered_range_flag is repeated whole on BF16X3).  The look-ahead filter of a
 * one-frame window is skipped, as in the reference (Export_FireRedVAD.py:229).
 * Returns, before any HIP call: VADX_EINVAL naming the argument for a NULL pointer or table, cfg->frames outside its range, clips /
 * n_tiles / frames_total < 1, counts that do not fit each other (n_tiles <= frames_total <= 64 * n_tiles), an unsupported cfg;
 * VADX_ENOSPACE for workspace_bytes below vadx_firered_long_workspace_bytes.  Device-side guard of every launch: a workgroup whose table
 * entries name a clip outside [0, clips), a tile outside its clip's tiles, an empty or decreasing prefix range, a range beyond
 * frames_total, a window above the cap, or a tile count that disagrees with the frame count returns before its first read or write of
 * the buffers: its rows keep what they held. */
int vadx_firered_run_long(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, const vadx_firered_long_tables *tables,
                          float *probs, void *workspace, size_t workspace_bytes, void *stream);

/* Streaming variant (FireRed Stream-VAD): one chunk of cfg->frames frames for `streams`
 * independent streams; caches f32 [R][streams][P][(N1-1)*S1] in -> out (must not alias); cfg->N2 == 0.
 * Replaces ort_session_C.run([probs, caches_out], {audio, caches_in}), Inference_FireRed_ONNX.py:798-801
 * (graph FireRedVAD/Export_FireRedVAD.py:479-612, 656-749 after the front-end). */
int vadx_firered_stream_run(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams,
                            const float *caches_in, float *caches_out, float *probs, void *stream);

typedef struct vadx_vadpost_params {     /* VadPostprocessor.__init__, Inference_FireRed_ONNX.py:108-120 */
    int   smooth_window_size;
    float prob_threshold;
    int   min_speech_frame, max_speech_frame, min_silence_frame, merge_silence_frame, extend_speech_frame;
} vadx_vadpost_params;

size_t vadx_vadpost_workspace_bytes(int batch, int stride);
/* probs f32 [B][stride] (n_frames[b] valid) -> decisions i8 [B][stride] + (start_frame, end_frame)
 * int32 pairs [B][cap][2] + counts [B]; one clip per thread.
 * Replaces VadPostprocessor.process + the edge extraction of decision_to_segment
 * (Inference_FireRed_ONNX.py:122-168, 181-304; MarbleNet copy Inference_NVIDIA_...:160-353);
 * the float32 seconds arithmetic + round(,3) of decision_to_segment :169-179 stays on the host.  On the device, from this call's
 * table: vadx_timestamps_frames, section "Timestamps". */
int vadx_vadpost(const vadx_vadpost_params *prm, const float *probs, int stride, const int32_t *n_frames,
                 int batch, int8_t *decisions, int32_t *segments, int32_t *counts, int cap,
                 void *workspace, size_t workspace_bytes, void *stream);

typedef struct vadx_stream_vadpost_params {     /* StreamVadPostprocessor.__init__, FireRedVAD/Export_FireRedVAD.py:1161-1190 */
    int   smooth_window_size;                   /* <= 16 */
    float speech_threshold;
    int   pad_start_frame, min_speech_frame, max_speech_frame, min_silence_frame;
} vadx_stream_vadpost_params;

size_t vadx_stream_vadpost_state_bytes(int streams);
/* The streaming decision state machine for `streams` independent streams, one thread per stream: probs f32 [streams][probs_stride]
 * (`frames` new frames each) -> the segments that END inside this chunk as (start_frame, end_frame) int32 pairs [streams][cap][2]
 * (0-based frames: multiply by 1 / frames_per_second on the host) + counts [streams] (count > cap => truncated).  `state`
 * (vadx_stream_vadpost_state_bytes, device) carries the moving-average ring buffer and the machine between calls; reset != 0 starts
 * every stream from the reference's reset() state; flush != 0 also reports the segment still open after the last frame, as the
 * reference's process_batch does at the end of its input, without closing it.  Same float32 operations in the same order as the
 * reference's per-frame loop (its comparisons are float32 under NumPy 2).
 * Replaces StreamVadPostprocessor.process_batch, FireRedVAD/Export_FireRedVAD.py:1161-1339 (driver Inference_FireRed_ONNX.py:788-822). */
int vadx_stream_vadpost(const vadx_stream_vadpost_params *prm, const float *probs, int64_t probs_stride, int frames, int streams,
                        void *state, int reset, int flush, int32_t *segments, int32_t *counts, int cap, void *stream);

/* Streaming FireRed (Stream-VAD for S live streams): every tick advances each stream by `chunks` chunks of cfg->frames frames,
 * F = chunks * frames <= 112 frames in all.  What the reference's chunk loop carries -- the FIR caches it feeds back and the
 * StreamVadPostprocessor object -- lives in a device RECORD of vadx_firered_stream_state_bytes(cfg, S) bytes.  The record is opaque
 * except that
 *   - its first S*R*P*pad floats are the caches [S][R][P][pad], pad = (N1 - 1) * S1: per stream the caches_in / caches_out of
 *     vadx_firered_stream_run (there [R][streams][P][pad]);
 *   - behind them, on the next multiple of 16 bytes, come 128 bytes per stream: the decision machine (ring buffer, sum, counters,
 *     state) and, at byte 112 of those, a 64-bit count of the frames the stream has done since its reset;
 *   - a record of all zero bytes is S streams in their reset state (no init call);
 *   - its size is a multiple of 16 bytes; records are 16-byte aligned.
 * After the front-end a tick is ONE call.  logmel f32 [S * chunks][frames][80] is the unchanged vadx_frontend_logmel over S rows of
 * `chunks` chunks of n samples each (batch = S, windows_per_clip = chunks): every chunk's features are computed on its own, no sample is
 * carried between chunks, as in the reference.  The `chunks` chunks of a stream are F consecutive frames to the net, which carries its
 * caches across them: a look-back-only net over concatenated frames IS the chunked net.  cfg->N2 must be 0.
 * state_in is never written (a tick can be recomputed from it, which the range protocol needs); state_out must not overlap it.
 * reset (NULL or uint8 [S]): != 0 = back to the reset state before this tick.  active (NULL or uint8 [S]): 0 = no audio for this stream
 * this tick -- its record in state_out is a bitwise copy of state_in's, a reset request is ignored, its probs are NaN, its count 0 and
 * its open_start -1 (its logmel rows are not read).
 * Outputs: probs f32 [S][odim][F]; segments int32 [S][cap][2] + counts [S]: the segments of channel 0 that END in this tick as 0-based
 * (start_frame, end_frame) pairs counted from the stream's reset, exactly what vadx_stream_vadpost reports with flush = 0 (same float32
 * operations in the same order; a count above cap = truncated, the state still advances); open_start int32 [S]: the 0-based start frame
 * of the segment still open after the tick, or -1 -- with the frames done, (open_start, frames_done - 1) is what the reference's
 * end-of-input rule appends, and nothing is closed by reporting it.  post->smooth_window_size <= 16.
 * group: streams per workgroup, 1 <= group <= vadx_firered_stream_group_max(F) = 112 / F, or 0 = the library's choice.  The streams of a
 * workgroup lie side by side in its LDS rows behind one load of the weights; every output of a stream and its bytes of state_out are
 * bitwise independent of group, of S, of the other streams and of their masks.
 * All three arithmetics, with the blob vadx_firered_pack_host wrote for cfg->arithmetic (a split arithmetic on widths the split
 * kernels do not take is refused); on F32 the probabilities and caches are bitwise those of vadx_firered_stream_run.  Range protocol per
 * tick: with an F16X2 cfg read vadx_firered_range_flag after the call and, when it is raised, call vadx_firered_stream_tick again with
 * the BF16X3 cfg and blob on the same arguments: every byte the first call wrote is written again.
 * Returns VADX_EINVAL, before any HIP call, for a NULL pointer (reset and active may be NULL), streams / chunks / cap < 1, F > 112, a
 * group outside [0, 112 / F], N2 != 0, smooth_window_size > 16, or overlapping records.
 * Replaces the body of the chunk loop, FireRedVAD/Inference_FireRed_ONNX.py:788-822 (ort_session_C.run :798-801 with its caches fed back,
 * StreamVadPostprocessor.process_batch, FireRedVAD/Export_FireRedVAD.py:1205-1339), for S streams that arrive in pieces. */

/* Bytes of the record of `streams` streams (0 for streams <= 0 or a cfg outside the limits; cfg->frames is not looked at). */
size_t vadx_firered_stream_state_bytes(const vadx_firered_cfg *cfg, int streams);
/* The most streams one workgroup serves at F = frames_per_tick frames per stream: 112 / F, 0 for F outside 1 .. 112. */
int vadx_firered_stream_group_max(int frames_per_tick);
int vadx_firered_stream_tick(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams, int chunks, int group,
                             const vadx_stream_vadpost_params *post, const uint8_t *reset, const uint8_t *active,
                             const void *state_in, void *state_out, float *probs, int32_t *segments, int32_t *counts, int cap,
                             int32_t *open_start, void *stream);

/* A RAGGED tick of the same streams on the same record: stream s advances by counts[s] chunks of cfg->frames frames, 0 <= counts[s] <=
 * vadx_firered_stream_group_max(cfg->frames) = 112 / frames, and the work is sum(counts) chunks in ONE launch.  The record is the
 * unchanged one of vadx_firered_stream_tick, so the two calls interchange tick by tick.  All tables are int32 on the device:
 *   counts [S], row_first [S]: stream s owns the log-mel rows row_first[s] .. row_first[s] + counts[s] - 1 of
 *     logmel f32 [n_rows][frames][80] (vadx_frontend_logmel over n_rows rows of ONE chunk each) and the columns
 *     row_first[s] * frames .. (row_first[s] + counts[s]) * frames - 1 of every row of probs f32 [odim][n_rows * frames];
 *   slot_stream [wg_first[n_wg]] (at most S entries) and wg_first [n_wg + 1]: workgroup w lays the streams
 *     slot_stream[wg_first[w] .. wg_first[w + 1]) side by side, slot j with counts[s_j] * frames LDS columns behind those of the slots before
 *     it; a workgroup holds at most 112 columns.  Every stream with a count above 0 must be named in exactly one slot: a stream named twice,
 *     or one with audio named nowhere (its bytes of state_out are then not written), is the caller's fault and is not checked.
 * segments [S][cap][2], counts_out [S] and open_start [S] are indexed by stream and mean what they mean in vadx_firered_stream_tick.
 * A stream with count 0 owns no log-mel row and no probability column: its record in state_out is a bitwise copy of state_in's, a reset
 * request for it is ignored, its counts_out is 0 and its open_start -1 (workgroups behind the n_wg compute ones do this).
 * Tables that lie: a slot is SKIPPED -- no columns, no record write, no decision -- and bit 1 (value 2) of *status is raised when its
 * stream index is outside [0, S), its count outside [0, 112 / frames], its rows outside [0, n_rows), or its columns would pass 112 (then
 * every slot behind it in the workgroup is skipped too), and a workgroup whose wg_first entries are negative, decreasing, more than 112
 * apart or above S is skipped whole.  A stream whose count or rows lie is treated as one without audio.  Nothing is indexed out of
 * bounds.  *status (uint32, device) is only ever OR-ed into: the caller zeroes it.
 * All three arithmetics and the range protocol of vadx_firered_stream_tick: after an F16X2 tick that raised vadx_firered_range_flag,
 * call again with the BF16X3 cfg and blob, the same state_in and the same tables; every byte the first call wrote is written again.
 * Every output of a stream and its bytes of state_out are bitwise what vadx_firered_stream_tick gives that stream with chunks =
 * counts[s], whatever the plan.
 * Returns VADX_EINVAL, before any HIP call and naming the argument, for a NULL pointer (reset may be NULL), streams / n_rows / n_wg /
 * cap < 1, frames > 112, N2 != 0, smooth_window_size > 16, overlapping or misaligned records.
 * Replaces the body of the chunk loop, FireRedVAD/Inference_FireRed_ONNX.py:788-822, for S streams that deliver different numbers of
 * chunks per tick. */
int vadx_firered_stream_tick_ragged(const vadx_firered_cfg *cfg, const float *packed, const float *logmel, int streams, int n_rows,
                                    const int32_t *counts, const int32_t *row_first, const int32_t *slot_stream, const int32_t *wg_first,
                                    int n_wg, const vadx_stream_vadpost_params *post, const uint8_t *reset, const void *state_in,
                                    void *state_out, float *probs, int32_t *segments, int32_t *counts_out, int cap, int32_t *open_start,
                                    uint32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * MarbleNet building blocks: one fused launch per Jasper sub-block
 * (depthwise conv -> pointwise 1x1 + folded BatchNorm [-> + residual 1x1] -> ReLU) and the frame
 * classifier head.  Replaces the encoder/decoder calls of NVIDIA_VAD_Optimized.forward,
 * Export_NVIDIA_MarbleNet_VAD.py:265-274 (BatchNorm folded on the host as in :58-151).
 * ------------------------------------------------------------------------------------------- */
typedef struct vadx_sepconv_cfg {
    int cin, cout;            /* <= 128 */
    int kernel, stride, dilation;   /* 'same' padding = dilation*(kernel-1)/2 */
    int depthwise;            /* 0: plain 1x1 conv (kernel must be 1) */
    int residual_cin;         /* 0: no residual branch; else channels of the block input */
    int relu;
} vadx_sepconv_cfg;
/* Limits, refused with VADX_EINVAL before any device call: channels in [1, 128]; a 32-frame tile's receptive field
 * 31 * stride + (kernel - 1) * dilation + 1 <= 100; and the residual contract -- the block input xres is read with this sub-block's
 * OUTPUT frame index and row length, so residual_cin > 0 needs stride == 1 and t_in == t_out (an odd kernel), and every earlier
 * sub-block of the same Jasper block must have kept the frame count too (the caller's side: MarbleNetEngine refuses such a layout). */

/* x: element (b, c, t) at x[b*xs_b + c*xs_c + t*xs_t] (lets the first block read the time-major
 * log-mel directly); xres [B][residual_cin][t_out]; y [B][cout][t_out].  Weights on the device:
 * dw_w [cin][kernel]; pw_w [cout_pad16][cin_pad16], pw_b [cout_pad16]; res_w [cout_pad16][rescin_pad16]. */
struct vadx_marblenet_cfg;   /* below: arithmetic of the launch + the fp16 x 2 range flag words; NULL = float32 MFMAs */
int vadx_sepconv_block(const vadx_sepconv_cfg *cfg, const float *dw_w, const float *pw_w, const float *pw_b,
                       const float *res_w, const float *res_b, const float *x, int64_t xs_b, int64_t xs_c,
                       int64_t xs_t, int t_in, const float *xres, float *y, int batch, int t_out, void *stream,
                       const struct vadx_marblenet_cfg *mcfg);
/* Fused forms for the published MarbleNet 3x2x64 layout (what MarbleNetEngine launches; the per-sub-block entry above stays
 * for other Jasper stacks).  block2: one residual Jasper block = two separable sub-blocks (depthwise `kernel`, stride 1,
 * 64 filters each) + the residual 1x1 branch of the block input, x [B][cin][T] -> y [B][64][T]; weights as for
 * vadx_sepconv_block (dw [c][kernel]; pw / res fragment-major, BatchNorm folded; biases padded to 16).
 * tail: block 5 (depthwise k 29, dilation 2, 64 -> 128) -> block 6 (plain 1x1, 128 -> 128) -> Linear(128 -> 2) -> softmax,
 * x [B][64][T] -> score0 / score1 [B][T] (dec_w [2][128], dec_b [2]); the 128-channel tensors never reach HBM. */
/* cfg (may be NULL = float32 MFMAs): `arithmetic` VADX_ARITH_AUTO / VADX_ARITH_F32 -- pw0 / pw1 / res_w are fragment-major float32
 * (vadx_frag_major_host); VADX_ARITH_F16X2 -- they are fp16 x 2 fragments (vadx_frag_h2_host: K_QUARTER for block2 with cin = 128, K_PLAIN for block2 with cin = 64 and for tail's pw / w6) and the 1x1 convs run as split
 * products on the fp16 pipe (float32-class results, csrc/split2.h); `range_flag` then points at two device words {sticky flag, bits of the
 * largest |operand|} that a launch raises when an activation left the fp16 range -- the caller reads them with the results and recomputes
 * that batch on VADX_ARITH_F32 (MarbleNetEngine does).  VADX_ARITH_BF16X3 is refused (no such form of these kernels). */
typedef struct vadx_marblenet_cfg {
    int32_t arithmetic;       /* VADX_ARITH_* */
    int32_t reserved;
    void *range_flag;         /* device uint32_t[2], zeroed by the caller; required for VADX_ARITH_F16X2 */
} vadx_marblenet_cfg;
int vadx_marblenet_block2(int cin, int kernel, const float *dw0, const float *pw0, const float *b0, const float *dw1,
                          const float *pw1, const float *b1, const float *res_w, const float *res_b, const float *x,
                          float *y, int batch, int frames, void *stream, const vadx_marblenet_cfg *cfg);
int vadx_marblenet_tail(const float *dw, const float *pw, const float *pb, const float *w6, const float *b6,
                        const float *dec_w, const float *dec_b, const float *x, float *score0, float *score1,
                        int batch, int frames, void *stream, const vadx_marblenet_cfg *cfg);
/* ---- MarbleNet over a RAGGED batch: B clips of ANY lengths in one launch sequence, dynamic-axis mode (one window = one whole clip, so a
 * clip's length sets its own frame count: NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-135).  The clips lie end to end in ONE
 * int16 vector `pcm`, NO padding and no alignment between them (the front-end reads samples as single int16 loads from clamped indices).
 * Per clip b of n_b samples: F_b = n_b / 160 + 1 log-mel frames (the centre-padded preset) and T1_b = (F_b - 1) / 2 + 1 encoder frames
 * (the stride-2, k 11 prologue).  Tables, all on the device (vadx.ragged.RaggedFrames builds them; every sum is checked against int32 there):
 *   clip_off  int64 [B]      first sample of clip b in pcm           clip_len  int32 [B]   n_b
 *   mel_first int32 [B+1]    prefix sum of F_b: clip b owns rows mel_first[b] .. of the log-mel buffer f32 [sum F][n_mels]
 *   enc_first int32 [B+1]    prefix sum of T1_b: clip b's activations are [C][T1_b] at FLOAT offset C * enc_first[b] of every buffer
 *                            between the launches, its scores s0 / s1 [enc_first[b] .. enc_first[b+1])
 *   tile tables              the front-end works in 64-frame tiles, the encoder in 32-frame tiles; each has tile_first int32 [B+1] (prefix
 *                            sum of ceil(F_b / 64) resp. ceil(T1_b / 32)) and tile_clip int32 [n_tiles] (the clip of every tile): a
 *                            workgroup finds (clip, tile) with two uniform loads -- no search, one int per tile.
 * Sequence on one HIP stream (a plain-C caller: INTEGRATION.md section 7):
 *   vadx_frontend_logmel_ragged    pcm + tables -> logmel f32 [sum F][80]
 *   vadx_sepconv_block_ragged      -> a0 f32, sum T1 * 128 floats         (block 1: the prologue)
 *   vadx_marblenet_block2_ragged   x 3 (kernel 13, 15, 17; cin 128, 64, 64) -> sum T1 * 64 floats each
 *   vadx_marblenet_tail_ragged     -> score0, score1 f32 [sum T1]
 *   vadx_tracks_gather (win_floats = 1, frames_per_window = 1, win_first = enc_first) + vadx_vadpost as for any ragged batch.
 * Every workgroup computes the very tile the rectangular launches compute for that clip alone (one device function per kernel, shared),
 * so clip b's slice of every output is bit for bit what the one-clip call gives.  Device-side guard of all four launches: a workgroup
 * whose table entries name a clip outside [0, B), a tile outside its clip's tiles, a negative, empty or decreasing prefix range, a range
 * beyond the totals passed by value, or tables that disagree about the clip (tile count against frame count; T1 against F; F against
 * clip_len) returns before its first read or write of the buffers: its rows keep what they held.  The arithmetic and the range-flag
 * protocol are vadx_marblenet_cfg's (F16X2 raised flag: repeat the whole sequence from vadx_sepconv_block_ragged on VADX_ARITH_F32). */

/* Log-mel of every clip of a ragged batch in one launch; replaces the per-file front-end of the dynamic-axis session call,
 * NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-147, 369-402, for B files of different lengths.  cfg / packed / mel_kb_host as
 * for vadx_frontend_logmel (nothing in the blob depends on a window length: one blob serves every clip; cfg->frames and cfg->window_len
 * only have to be valid).  tile_first / tile_clip: the 64-frame tile tables.  out f32 [mel_total][n_mels].  Built for cfg->fold
 * VADX_FE_KIND_SPLIT_H2 / VADX_FE_KIND_SPLIT_B3 and the two-tap prep 1 of a centre-padded preset, no in-graph resampling.  Returns
 * VADX_EINVAL, before any HIP call, for a NULL pointer, any other kind or prep (the message names it), clips / n_tiles / mel_total /
 * pcm_len < 1, or counts that do not fit each other (clips <= n_tiles <= mel_total <= 64 * n_tiles). */
int vadx_frontend_logmel_ragged(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host, const int16_t *pcm,
                                int64_t pcm_len, const int64_t *clip_off, const int32_t *clip_len, const int32_t *mel_first,
                                const int32_t *tile_first, const int32_t *tile_clip, int clips, int n_tiles, int mel_total,
                                float *out, void *stream);

/* The same launch for a SNIP-EDGE preset (no centre pad: the FireRed front-end, FireRedVAD/Export_FireRedVAD.py:396-418, 428-461): clip b
 * has (clip_len[b] - n_fft) / hop + 1 frames, n_fft = taps + 2 * tap0 -- none when it is shorter than n_fft samples, and then no tile
 * and no row.  It is the front-end of the dynamic-axis FireRed call on B files of different lengths (one window per file,
 * FireRedVAD/Inference_FireRed_ONNX.py:541-547, :644-650); mel_first / tile_first / tile_clip are vadx_firered_long_tables' frame_first /
 * tile_first / tile_clip.  Arguments and refusals as above, with cfg->center_pad == 0 required instead and n_tiles <= mel_total <= 64 *
 * n_tiles (clips may exceed n_tiles: a clip may have no frame).  vadx_frontend_logmel_ragged itself keeps refusing a centre pad of 0. */
int vadx_frontend_logmel_ragged_snip(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host, const int16_t *pcm,
                                     int64_t pcm_len, const int64_t *clip_off, const int32_t *clip_len, const int32_t *mel_first,
                                     const int32_t *tile_first, const int32_t *tile_clip, int clips, int n_tiles, int mel_total,
                                     float *out, void *stream);

/* The encoder's tables (device pointers): the 32-frame tile tables, frame_first = enc_first, src_first = mel_first (read by
 * vadx_sepconv_block_ragged only; the other two ignore src_first / src_total). */
typedef struct vadx_marblenet_ragged {
    const int32_t *tile_first;    /* [clips + 1] */
    const int32_t *tile_clip;     /* [n_tiles] */
    const int32_t *frame_first;   /* [clips + 1], frame_first[clips] = frames_total */
    const int32_t *src_first;     /* [clips + 1], src_first[clips] = src_total */
    int32_t clips, n_tiles, frames_total, src_total;
} vadx_marblenet_ragged;
/* Ragged forms of vadx_sepconv_block (the prologue of the published layout only: depthwise k 11, stride 2, no residual; x = the
 * time-major log-mel rows, row stride xs_t floats, channel stride 1), vadx_marblenet_block2 and vadx_marblenet_tail: the same weights,
 * the same arithmetics, `batch` and `frames` replaced by the tables.  They replace the per-file session calls of
 * NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-147, 369-402 for B files of different lengths.  Each returns VADX_EINVAL,
 * before any HIP call, for a NULL pointer or table, clips / n_tiles / frames_total < 1, counts that do not fit each other (clips <=
 * n_tiles <= frames_total <= 32 * n_tiles; the prologue also frames_total <= src_total <= 2 * frames_total), an arithmetic other than
 * AUTO / F32 / F16X2 (named in the message), F16X2 without range_flag, or a layer shape outside the published layout. */
int vadx_sepconv_block_ragged(const vadx_sepconv_cfg *cfg, const float *dw_w, const float *pw_w, const float *pw_b, const float *x,
                              int64_t xs_t, float *y, const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *mcfg);
int vadx_marblenet_block2_ragged(int cin, int kernel, const float *dw0, const float *pw0, const float *b0, const float *dw1,
                                 const float *pw1, const float *b1, const float *res_w, const float *res_b, const float *x, float *y,
                                 const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *cfg);
int vadx_marblenet_tail_ragged(const float *dw, const float *pw, const float *pb, const float *w6, const float *b6,
                               const float *dec_w, const float *dec_b, const float *x, float *score0, float *score1,
                               const vadx_marblenet_ragged *rt, void *stream, const vadx_marblenet_cfg *cfg);

/* ---- MarbleNet over LIVE STREAMS: S streams, each the audio of one virtual clip arriving in pieces.  After a stream's last piece its
 * emitted scores, in order, are what the dynamic-axis call gives for the whole clip (n / 320 frames of n samples: the session's
 * signal_len - 1) -- bit for bit in every frame that reads none of the log-mel frames the whole-clip front-end computes in a TAIL tile (its
 * last F mod 64 frames when that is 1 .. 48, F = n / 160 + 1: that tile variant rounds |X|^2 with an FMA, the full tile does not, so the
 * whole-clip call's own bits depend on where the clip ends; a stream computes every frame in the full-tile form), and within one float32
 * ulp of the log-mel behind that.  Replaces, for a growing stream, re-running the session over a sliding buffer -- the seam is the window loop
 * and the dynamic-axis call of NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-135, 369-388.
 * Geometry (published 3x2x64 layout, masks off): score frame j reads encoder frames j - 70 .. j + 70 = log-mel frames 2j - 145 .. 2j +
 * 145 = samples up to 320 j + 23 456, so a stream emits every frame once, 73 frames (1.46 s) behind the audio it has been fed:
 *   after N = 320 J samples and no final tick   log-mel frames 0 .. 2J - 2 are complete, max(0, J - 73) score frames are out;
 *   a final tick at a total of n samples         brings the total to n / 320 and resets the stream.
 * RECORD: vadx_marblenet_stream_state_bytes(S) = S * 46 048 bytes on the device, 16-byte aligned, stream s at byte 46 048 s.  Per stream,
 * in 4-byte words (activations float32 on both arithmetics; J = samples fed / 320):
 *       0 ..   800  log-mel history [10 frames][80], frames 2J - 11 .. 2J - 2      800 ..  3872  prologue output [128][24], frames J - 27 .. J - 4
 *    3872 ..  5664  block 2 output [64][28], frames J - 43 .. J - 16              5664 ..  7712  block 3 output [64][32], frames J - 61 .. J - 30
 *    7712 .. 11296  block 4 output [64][56], frames J - 101 .. J - 46            11296 .. 11508  audio carry: 417 int16 (416 samples + the
 *   11508 .. 11510  samples fed since the reset (int64)                                           pre-emphasis tap in front), zero-padded
 *   11510 .. 11512  score frames emitted since the reset (int64)
 *   A frame index below 0 is a layer's zero padding and is held as zeros, so ALL-ZERO BYTES ARE A FRESH STREAM (no init call).
 * A TICK is one call: vadx_marblenet_stream_tick runs, on `stream`, an opening kernel (checks, plan, `carry || new` rows, histories into
 * the row buffers of the workspace), vadx_frontend_logmel_stream, the prologue, blocks 2 - 4 and the tail as stream instantiations of the
 * whole-clip kernels (a workgroup's tile is a tile of the virtual clip; its halo comes from the history columns; frames < 0, or >= the
 * clip's end on a final tick, are masked where the rectangular kernels mask them), and a closing kernel that writes state_out.
 * Inputs per tick: samples int16 [S][sample_stride >= 320 k]; n_samples int32 [S]: 0 = no audio this tick, a non-final stream a positive
 * multiple of 320 up to 320 k, a final stream anything in 0 .. 320 k; reset / final: NULL or uint8 [S] (reset applies before the audio;
 * final runs every stage out against zeros BEHIND THE CLIP'S LAST FRAME, stage by stage -- not "feed silence" -- emits the remaining
 * look-ahead and leaves the stream reset).  1 <= k <= vadx_marblenet_stream_max_frames() = 256 frames (5.12 s) per tick.
 * Outputs: score0 / score1 f32 [S][cap], cap = vadx_marblenet_stream_cap(k) = k + 73, the first n_out[s] entries = the stream's next
 * score frames, the rest NaN; n_out int32 [S].  state_in is never written and state_out is a second record (ping-pong): a tick whose
 * F16X2 range flag was raised is repeated on VADX_ARITH_F32 from the same state_in.  A stream with n_samples = 0 and not final costs no
 * tile, emits nothing and has its record copied bit for bit (zeroed when reset is set).  No result depends on k, on a stream's
 * neighbours or on the order of streams.
 * Device-side guard: a stream whose n_samples is negative, above 320 k, or no multiple of 320 while not final -- or whose record's
 * counters no tick could have written -- is skipped: its record in state_out, its score rows and its n_out keep what they held, and
 * nothing is indexed with its values.
 * VADX_EINVAL, before any HIP call: a NULL pointer (reset / final may be NULL), streams < 1, k outside [1, 256], sample_stride < 320 k,
 * state_out == state_in, an unaligned or short workspace, an arithmetic other than AUTO / F32 / F16X2 (named), F16X2 without range_flag,
 * a front-end cfg other than the MarbleNet preset at 16 kHz on VADX_FE_KIND_SPLIT_H2 / SPLIT_B3 (named: kind, prep, hop, in-graph
 * resampling).  Weights: those of vadx_sepconv_block / vadx_marblenet_block2 / vadx_marblenet_tail for the same arithmetic. */
typedef struct vadx_marblenet_stream_weights {
    const float *p_dw, *p_pw, *p_pb;                                   /* prologue (block 1) */
    const float *b_dw0[3], *b_pw0[3], *b_b0[3], *b_dw1[3], *b_pw1[3], *b_b1[3], *b_rw[3], *b_rb[3];   /* blocks 2, 3, 4 */
    const float *t_dw, *t_pw, *t_pb, *t_w6, *t_b6, *dec_w, *dec_b;     /* blocks 5 + 6 + decoder */
} vadx_marblenet_stream_weights;
int vadx_marblenet_stream_max_frames(void);
int vadx_marblenet_stream_cap(int k);                       /* k + 73; 0 for a k outside [1, 256] */
size_t vadx_marblenet_stream_state_bytes(int streams);
size_t vadx_marblenet_stream_workspace_bytes(int streams, int k);   /* scratch of one tick (nothing is carried in it); 0 = bad arguments */
int vadx_marblenet_stream_tick(const vadx_frontend_cfg *fe, const float *fe_packed, const int32_t *mel_kb_host,
                               const vadx_marblenet_stream_weights *w, const int16_t *samples, int64_t sample_stride,
                               const int32_t *n_samples, const uint8_t *reset, const uint8_t *final, int streams, int k,
                               const void *state_in, void *state_out, float *score0, float *score1, int32_t *n_out,
                               void *workspace, size_t workspace_bytes, void *stream, const vadx_marblenet_cfg *cfg);
/* The stream front-end on its own: stream s's row = rows + s * row_stride holds `carry || new` int16 samples with NO centre padding --
 * sample 0 is the pre-emphasis tap, frame i starts at row sample 1 + 160 i; samples at and behind row_len[s] read as zeros.  n_frames[s]
 * frames go to rows out_row0 .. of the stream's out_rows rows of out f32 [S][out_rows][n_mels]; row_len / n_frames are device int32 [S].
 * A frame is computed by the device functions of vadx_frontend_logmel in their full-tile (64-frame) form whatever n_frames is, so its bits
 * are those of the whole-clip call's full tiles and depend on no neighbour frame.  Device-side guard:
 * row_len outside [1, row_stride] or n_frames outside [1, max_frames] skips the stream.  VADX_EINVAL, before any HIP call: a NULL
 * pointer, a kind other than VADX_FE_KIND_SPLIT_H2 / SPLIT_B3, a prep other than 1, a hop other than 160 or in-graph resampling (each
 * named), streams / max_frames / row_stride < 1, or out_row0 + max_frames > out_rows. */
int vadx_frontend_logmel_stream(const vadx_frontend_cfg *cfg, const float *packed, const int32_t *mel_kb_host, const int16_t *rows,
                                int64_t row_stride, const int32_t *row_len, const int32_t *n_frames, int streams, int max_frames,
                                float *out, int out_rows, int out_row0, void *stream);

/* enc [B][C][T] -> softmax(Linear(C->2)) split into score0 / score1 [B][T]. */
int vadx_frame_classifier(const float *enc, const float *dec_w, const float *dec_b, int batch, int channels,
                          int frames, float *score0, float *score1, void *stream);

/* ---------------------------------------------------------------------------------------------
 * DFSMN near+far: ICCRN building blocks on frame-tiled ("FT") activations
 *   [tile = chunk*NT + t/16][C][F][16]  -- element (c,f,t) at ((tile*C + c)*F + f)*16 + t%16.
 * Reference: DFSMN/near_and_far_end_audio/Export_DFSMN_VAD.py (LayerNorm :157-167, CFB :76-93,
 * CepsUnit :96-154, CH_LSTM_F :270-284, CH_LSTM_T :252-267, NET :170-249, DFSMN_VAD :287-354).
 * ------------------------------------------------------------------------------------------- */
typedef struct vadx_ft_view { const float *ptr; int c_total, c_off, c; } vadx_ft_view;   /* channel slice */
typedef struct vadx_ft_ln { const float *stats, *w, *b; } vadx_ft_ln;                    /* LayerNorm on the fly */

/* stats[tile][16][2] = (mean, 1/(unbiased std + 1e-6)) over (C,F) of cat(a, b) per frame. */
int vadx_dfsmn_frame_stats(const vadx_ft_view *a, const vadx_ft_view *b, int F, int tiles, float *stats, void *stream);
/* Fused alternative: pw_conv and the forward dft_f can emit, per frame, the (count, mean, sum of squared deviations) of
 * what each workgroup wrote -- "partial statistics", float [tiles][VADX_DFSMN_STAT_PARTS][16][4], caller-owned --
 * and this merges the partials of one tensor (part_b NULL) or of the channel concatenation of two into the same
 * stats[tile][16][2] that frame_stats produces, without re-reading the tensors. */
#define VADX_DFSMN_STAT_PARTS 2
int vadx_dfsmn_stats_merge(const float *part_a, const float *part_b, int tiles, float *stats, void *stream);
/* Shapes are instantiated at compile time: (co, cin, kf, mode) in {(20,20,1,1), (20,40,1,1), (20,20,3,2), (20,24,1,0), (20,40,1,0),
 * (40,40,1,0), (2,60,1,0)} -- the ICCRN's seven; anything else returns VADX_EINVAL.
 * mode 0: out0 = act(conv(cat(a,b)) + bias)        (kf taps along F, weights [ceil16(co)][kf*cin])
 * mode 1: CFB front: g = sigmoid(convG(LN(x)) + bias); xi = convI(x) + bias2; out0 = g*xi; out1 = xi - g*xi
 * mode 2: CFB back : out0 = conv31(LN(x)) + bias + add
 * part0 / part1 (optional, may be NULL): partial statistics of out0 / out1 (mode 1) for vadx_dfsmn_stats_merge. */
int vadx_dfsmn_pw_conv(int mode, const vadx_ft_view *a, const vadx_ft_view *b, const vadx_ft_ln *ln,
                       const float *w, const float *bias, const float *w2, const float *bias2,
                       const vadx_ft_view *add, const vadx_ft_view *out0, const vadx_ft_view *out1,
                       int F, int co, int kf, int act, int tiles, float *part0, float *part1, void *stream);
/* CepsUnit's length-160 real DFT along F (inverse=0: in C ch x 160 -> out 2C ch x 81, LayerNorm on the
 * input) and its pinv-based inverse fused with the complex product (inverse=1: in = spectrum, lo = LSTM
 * output, both 2C ch x 81 -> out C ch x 160).  tbl = float [160][160] row-major:
 *   forward: rows = cos bins 0..80 | sin bins 1..79 (the sine rows of bins 0 and 80 vanish; those two outputs are written as 0);
 *   inverse: rows = output bin f, columns k = re 0..80 | im 1..79 of the pseudo-inverse basis (its im(0), im(80) columns are 0).
 * part (optional, forward only): partial statistics of out. */
int vadx_dfsmn_dft_f(int inverse, const vadx_ft_view *in, const vadx_ft_view *lo, const vadx_ft_ln *ln,
                     const float *tbl, const vadx_ft_view *out, int C, int tiles, float *part, void *stream);
/* bi-LSTM (hidden 20) along F with the tile's 16 frames as the batch; in->c = 4 or 40; out 40 ch.  arithmetic: VADX_ARITH_* of the
 * 40-channel (CepsUnit) form -- AUTO = BF16X3, F32 = the float32-MFMA kernel, F16X2 = fp16 x 2 split products with range_flag = two
 * zeroed device words {sticky flag, bits of the largest |operand|} (the caller recomputes a flagged batch on BF16X3 / F32); range_flag
 * may be NULL for the other arithmetics. */
int vadx_dfsmn_lstm_f(const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2],
                      const float *const w_hh[2], const float *const b_ih[2], const float *const b_hh[2],
                      const vadx_ft_view *out, int F, int tiles, void *stream, int arithmetic, void *range_flag);

/* One gated conv block (CFB :76-93 with its CepsUnit :96-154) as two streaming launches around vadx_dfsmn_lstm_f
 * (csrc/dfsmn_cfb.hip): the block's 20-channel intermediates gx, r, lo, ceps never reach memory.
 *   front: cat(a, b) (20 or 40 ch x 160, LN0 statistics stats0[tile][16][2] as frame_stats / stats_merge give them)
 *          -> y1 [tiles][20][160][16] = conv31(ln1_w * gx) WITHOUT LayerNorm 1's (mean, inv, bias) and the conv bias,
 *             stats1 [tile][16][2] = (mean, 1/(std + 1e-6)) of gx,
 *             li [tiles][40][81][16] = DFT_F(LN2(xi - gx)) (real | imaginary parts) and its statistics stats_li for the LSTM's LayerNorm;
 *   back:  hf (the LSTM output, [tiles][40][81][16]), li, y1, stats1 -> out (20-channel slice of an FT tensor)
 *          = conv31(LN1(gx)) + bias + ceps_unit(...), part (optional): its partial statistics for vadx_dfsmn_stats_merge.
 * All pointers are device pointers; the derived tables are built on the host (vadx/dfsmn.py: Iccrn._cfb_tables):
 *   ln0_w [cin][160]; gate_w / in_w [32][cin], in_b [32] (rows >= 20 zero); conv_w [32][60], column tap * 20 + ci;
 *   front_tab [160 bins][4][20 channels]: (conv_gate ln0_w, conv_gate ln0_b + gate bias, ln1_w, ln2_w) -- LayerNorm 0 is applied
 *           BEHIND the gate conv: pre-activation = inv0 * (Wg (ln0_w * x)) + front_tab[1] - mean0 * inv0 * front_tab[0];
 *   fwd_tbl [10 row tiles][40 k-steps][64 lanes]: lane (q, i) of fragment (m, s) = T[16 m + i][4 s + q], T = the 160 x 160 forward
 *           table of vadx_dfsmn_dft_f; fwd_fix [20 ch][10][64]: lane quarter q = 0 -> (T ln2_w[c])[16 m + i], q = 1 -> (T ln2_b[c])[..], else 0;
 *   lin_w [48][40], lin_b [48]: CepsUnit's Linear with rows permuted so that row 16 t + 4 q + r = (r >> 1 ? imaginary : real) output
 *           of channel 8 t + 2 q + (r & 1) (zero rows for channels >= 20);
 *   inv_tbl [10][41][64]: k-steps 0..20 = real parts of bins 4 s .. 4 s + 3, 21..40 = imaginary parts of bins 4 (s - 21) .. + 3
 *           (zero for bin 0 and bins > 80); out_fix [20][10][64]: q = 0 -> conv31(ln1_w)[c][16 m + i], q = 1 -> conv31(ln1_b) + bias. */
typedef struct vadx_dfsmn_cfb_weights {
    const float *ln0_w, *gate_w, *in_w, *in_b, *front_tab, *conv_w, *fwd_tbl, *fwd_fix, *lin_w, *lin_b, *inv_tbl, *out_fix;
    /* ABI 5: the two DFT tables as bf16 x 3 split A fragments (csrc/split3.h) for the split-product kernels, or NULL (the f32-MFMA
     * kernels run then): fwd_tbl_q [10 row tiles][5 chunks of 32 bins][3 planes][256 floats], lane 16 g + i of a fragment
     * holds T[16 tile + i][32 chunk + 8 g + e], e = 0..7, as eight bf16;  inv_tbl_q [10][5 chunks][3][256], same fragment layout, with
     * the 160 columns (81 real + 79 imaginary parts) ordered so that chunk j = [re of ceps bins 16 j .. 16 j + 15 | im of the same
     * bins] and the slot of the non-existent im of bin 0 holds re of bin 80. */
    const float *fwd_tbl_q, *inv_tbl_q;
    /* ABI 6: VADX_ARITH_* of the two halves.  front: AUTO = BF16X3 when fwd_tbl_q is given, else F32.  back: AUTO = F32 (its split form is
     * no faster: that half waits on 64-byte rows, not on the matrix pipe).  F16X2 is not built for these kernels and is refused. */
    int32_t front_arithmetic, back_arithmetic;
} vadx_dfsmn_cfb_weights;
int vadx_dfsmn_cfb_front(const vadx_dfsmn_cfb_weights *w, const vadx_ft_view *a, const vadx_ft_view *b, const float *stats0,
                         float *y1, float *stats1, float *li, float *stats_li, int tiles, void *stream);
int vadx_dfsmn_cfb_back(const vadx_dfsmn_cfb_weights *w, const float *hf, const float *li, const float *y1, const float *stats1,
                        const vadx_ft_view *out, float *part, int tiles, void *stream);

/* x4 = [mix_re, mix_im, |alpha| far_re, |alpha| far_im] (FT, 4 ch x 160), DFSMN_VAD.forward :326-335.
 * pow_far NULL: far power from channels 2, 3 (near + far model).  pow_far = [160][frames][10] floats: the near-end-only
 * model's baked far-end power (DFSMN/only_near_end_audio/Export_DFSMN_VAD.py:309, :327); channels 2, 3 of `in` then
 * hold its constant far spectrum. */
int vadx_dfsmn_alpha_scale(const float *in, float *out, int chunks, int nt, const float *w1, const float *b1,
                           const float *w2, const float *b2, const float *pow_far, int frames, void *stream);
/* LSTM along time, 16 bins per workgroup.  which = 0: NET.ch_lstm (in 20, hidden 40, 2 layers, Linear 40->20,
 * output multiplied element-wise with `mul` = e5);  which = 1: NET.out_ch_lstm (in 40, hidden 20, Linear 20->40).
 * wl rows zero-padded to a multiple of 16. */
int vadx_dfsmn_lstm_t(int which, const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2], const float *const w_hh[2],
                      const float *const b_ih[2], const float *const b_hh[2], const float *wl, const float *bl,
                      const vadx_ft_view *mul, const vadx_ft_view *out, int F, int frames, int chunks, void *stream);
/* The same with an explicit frame stride between chunks (a multiple of 4): chunk c's frame t is column (c * frame_stride + t) % 16 of
 * tile (c * frame_stride + t) / 16.  vadx_dfsmn_lstm_t is frame_stride = 16 * ceil(frames / 16). */
/* arithmetic (ABI 6): VADX_ARITH_AUTO / VADX_ARITH_F32 = float32 MFMAs; VADX_ARITH_F16X2 = the two-layer net (which = 0) as fp16 x 2 split
 * products (csrc/split2.h; weights split by the kernel itself), range_flag = two zeroed device words {sticky flag, bits of the largest
 * |operand|} raised when an input or weight left the fp16 range (the caller then recomputes on VADX_ARITH_F32); which = 1 runs float32
 * MFMAs for every arithmetic. */
int vadx_dfsmn_lstm_t_ex(int which, const vadx_ft_view *in, const vadx_ft_ln *ln, const float *const w_ih[2], const float *const w_hh[2],
                         const float *const b_ih[2], const float *const b_hh[2], const float *wl, const float *bl,
                         const vadx_ft_view *mul, const vadx_ft_view *out, int F, int frames, int chunks, int frame_stride, void *stream,
                         int arithmetic, void *range_flag);
/* Copy an FT tensor [channels][F] of `chunks` windows between frame strides (both multiples of 4, >= frames): e.g. 112 -> 104 packs
 * 101-frame windows onto 6.5 tiles each (the per-frame kernels then process 7 % fewer tiles), 104 -> 112 unpacks the result.
 * dst holds ceil(chunks * dst_stride / 16) tiles. */
int vadx_dfsmn_ft_repack(const float *src, float *dst, int channels, int F, int frames, int chunks, int src_stride, int dst_stride, void *stream);
/* NET.istft :220-224: y_ft FT [2 ch x 160] -> out f32 [chunks][(frames-1)*160 + 1]; basis_t [320 j][320 ch]
 * (transposed inverse basis, row 319 zero), wsum_inv = the reference's window_sum_inv buffer; z_ws scratch
 * of chunks*frames*320 floats.  wsum_inv must hold at least (frames-1)*160 + 319 floats -- it is read at samples 159 ..
 * (frames-1)*160 + 159 of the uncropped signal -- and the entry point cannot check that: the caller bounds `frames` by
 * the frame count its buffer was built for (200 in NET.__init__; vadx.dfsmn.ISTFT_MAX_FRAMES). */
int vadx_dfsmn_istft(const float *y_ft, const float *basis_t, const float *wsum_inv, float *z_ws, float *out,
                     int chunks, int frames, void *stream);
/* mask-net head: device pointers; linear weights zero-padded to multiples of 16 in BOTH dims
 * ([Hp][240], [H2p][Hp], [Hp][H2p]); conv1 [hidden][lorder]; shift already includes log(32768^2). */
typedef struct vadx_dfsmn_mask_weights {
    int hidden, fsmn_hidden, layers, lorder;
    const float *shift, *scale, *linear1_w, *linear1_b, *linear3_w, *linear3_b;
    const float *fsmn_linear_w[8], *fsmn_linear_b[8], *fsmn_project_w[8], *fsmn_conv_w[8];
} vadx_dfsmn_mask_weights;
/* feat f32 [chunks][frames][240] (3 x 80 log-fbank streams) -> vad f32 [chunks][frames]
 * (DFSMN_VAD.forward :349-353 + UniDeepFsmn.compute1, uni_deep_fsmn.py:311-329).  One workgroup per chunk with the activations in
 * LDS: frames in [1, 64], hidden in [1, 128], fsmn_hidden in [1, 256], layers in [0, 8], lorder in [1, 20]; anything else is
 * VADX_EINVAL with a message naming the limit. */
int vadx_dfsmn_mask_net(const vadx_dfsmn_mask_weights *w, const float *feat, int chunks, int frames, float *vad,
                        void *stream);
/* Look-ahead vote + tail of the DFSMN driver (Inference_DFSMN_VAD_ONNX.py:231-273): vad f32 [B][W][frames]
 * -> flags u8 [B][W*(frames-lb) + lb] (1 = silence). */
int vadx_dfsmn_vote(const float *vad, int batch, int windows, int frames, int look_backward, double speaking_score,
                    double silence_score, uint8_t *flags, void *stream);

/* DFSMN over a RAGGED batch (ABI 10): B clip pairs of ANY lengths, work proportional to the sum of their windows.  The caller cuts each
 * pair to its shorter side, pads each side to the window grid on the host (Inference_DFSMN_VAD_ONNX.py:124-163) and lays the padded clips
 * end to end, with no filler, in two int16 vectors that share the tables win_first int32 [B+1] and win_src int64 [n_windows] of "Ragged
 * batches" above (vadx.ragged.RaggedPairs builds all of this).  DFSMN's grid -- 16 001 samples every 10 881 -- is not made of 16-byte
 * runs, so the sequence on one HIP stream is
 *   vadx_windows_gather_any    once per channel: pcm, win_src -> int16 [n_windows][window_len]
 *   the network                unchanged (windows are stateless): vadx_frontend_stft_ft .. vadx_dfsmn_mask_net with batch = n_windows,
 *                              windows_per_clip = 1, row_stride = win_stride = window_len -> vad f32 [n_windows][frames]
 *   vadx_dfsmn_vote_ragged     -> flags u8 [B][flag_stride] */

/* vadx_windows_gather for any grid: row w of window_buf int16 [n_windows][window_len] = pcm[win_src[w], win_src[w] + window_len), for any
 * window_len >= 1 and any offset >= 0; pcm and window_buf 2-byte aligned.  A window whose source range leaves [0, pcm_len) is written as
 * ZEROS; nothing outside pcm is ever read.  A pure copy, one int16 per access (64 KB per window pair ahead of a network pass that moves
 * orders of magnitude more).  Returns VADX_EINVAL, before any HIP call, for a NULL pointer, n_windows < 1, pcm_len < 1 or window_len < 1.
 * Replaces the slicing `near_end_audio[:, :, slice_start:slice_end]` of DFSMN/near_and_far_end_audio/Inference_DFSMN_VAD_ONNX.py:221-229,
 * 259-260 for every window of every clip at once. */
int vadx_windows_gather_any(const int16_t *pcm, int64_t pcm_len, const int64_t *win_src, int n_windows, int window_len,
                            int16_t *window_buf, void *stream);

/* vadx_dfsmn_vote over a ragged batch (one device function votes a window in both): vad f32 [n_windows][frames], clip b owns the rows
 * win_first[b] .. win_first[b+1]-1.  Row b of flags u8 [batch][flag_stride]: its first W_b * (frames - look_backward) + look_backward
 * entries are the reference's `saved` list of clip b (1 = silence), bit for bit what vadx_dfsmn_vote gives for that clip's rows alone
 * (the same float32 threshold comparison); every other entry is 255 (the call fills flags with 255 first, on `stream`).  max_windows: the
 * largest W_b the caller sized flag_stride for.  A table entry that does not describe rows inside vad -- W_b <= 0, W_b > max_windows,
 * win_first[b] < 0, win_first[b+1] > n_windows -- leaves that row all 255 and indexes nothing out of bounds.  Returns VADX_EINVAL, before
 * any HIP call, for a NULL pointer, batch / n_windows / max_windows / frames < 1, flag_stride < max_windows * (frames - look_backward) +
 * look_backward, or a look_backward outside [1, frames).
 * Replaces the while-loop + tail, Inference_DFSMN_VAD_ONNX.py:231-273, for B file pairs of different lengths. */
int vadx_dfsmn_vote_ragged(const float *vad, int batch, int n_windows, int max_windows, const int32_t *win_first, int frames,
                           int look_backward, double speaking_score, double silence_score, uint8_t *flags, int64_t flag_stride,
                           void *stream);

/* Live DFSMN streams (ABI 10): S calls (microphone + loudspeaker reference, or the microphone alone) advance by `windows` analysis windows
 * per tick.  What the reference loop carries from window to window -- the vote's `silence` and the (look_backward + 1) * 320 samples two
 * consecutive windows share, per channel -- lives, with a "has a carry" word and a 64-bit count of the windows done since the reset, in a
 * device RECORD of vadx_dfsmn_stream_state_bytes bytes.  The record is opaque except that a record of all zero bytes is S streams in
 * their reset state (no init call) and that its size is a multiple of 16 bytes; records are 16-byte aligned.
 * One tick on one HIP stream:
 *   vadx_dfsmn_stream_windows  new samples + carry -> near_buf / far_buf int16 [n_slots*windows][window_len], the new carry
 *   the network                unchanged, with batch = n_slots * windows, windows_per_clip = 1 -> vad f32 [n_slots*windows][frames]
 *   vadx_dfsmn_stream_vote     -> flags, tail, the rest of the record
 * Both stream calls of a tick take the SAME state_in, state_out, slot and reset.  state_in is never written (a tick can be repeated from
 * it); state_in and state_out must not overlap.  vadx_dfsmn_stream_windows writes only the carry and the "has a carry" word of state_out,
 * vadx_dfsmn_stream_vote everything else.
 * slot (NULL or int32 [S]) is the active mask AND the row map, because a stream without audio must cost no network time: slot[s] = -1 =
 * no audio for stream s this tick; slot[s] = a in [0, n_slots) = stream s owns the rows a*windows .. a*windows + windows - 1 of near_buf /
 * far_buf / vad.  NULL = the identity (a stream s >= n_slots is then inactive); a value outside [-1, n_slots) is treated as -1.  Two
 * streams naming one slot is the caller's error -- documented, not checked, like `order` of vadx_fsmn_clips_ragged: their window rows
 * race.  Rows of a slot no stream names are not written.  An inactive stream's record in state_out is a bitwise copy of state_in's (a
 * reset request on it is ignored), its flags and tail are 255.
 * reset (NULL or uint8 [S]): != 0 = back to the reset state before this tick.
 * The fp16 x 2 range protocol needs nothing here: it concerns the network calls, which read only the window buffers.
 * The flags of successive ticks followed by the last tick's tail are bit for bit vadx_dfsmn_vote over the concatenated windows. */

/* Bytes of the record of `streams` streams of `channels` channels (1 = near-end only, 2 = near + far): a multiple of 16, linear in
 * streams.  0 for streams < 1, channels outside {1, 2}, look_backward < 1 or (look_backward + 1) * 320 >= window_len (no stride left). */
size_t vadx_dfsmn_stream_state_bytes(int streams, int window_len, int look_backward, int channels);

/* Window assembly, per channel (far and far_buf both NULL = one channel).  stride = window_len - (look_backward + 1) * 320.  near / far
 * int16 [S][row_stride] hold each stream's NEW samples from column 0: windows * stride of them for a stream that has a carry, window_len +
 * (windows - 1) * stride for one that has none (zero record, or reset this tick); row_stride >= windows * stride is all this call can
 * check, and a sample past row_stride reads as zero.  Window j of a stream is [j * stride, j * stride + window_len) of (carry ++ new
 * samples); the last (look_backward + 1) * 320 samples become the carry in state_out.  Any window_len: buffers 2-byte aligned, records
 * 16-byte.  Returns VADX_EINVAL, before any HIP call, for a NULL pointer (near, state_in, state_out, near_buf; far without far_buf or the
 * reverse), streams / n_slots / windows < 1, look_backward < 1 or leaving no stride, a row_stride below windows * stride, or overlapping
 * records.
 * Replaces the slicing and `slice_start += stride_step` of Inference_DFSMN_VAD_ONNX.py:221-229, 259-260 for audio that arrives in pieces. */
int vadx_dfsmn_stream_windows(const int16_t *near, const int16_t *far, int64_t row_stride, int streams, int n_slots, int windows,
                              int window_len, int look_backward, const int32_t *slot, const uint8_t *reset, const void *state_in,
                              void *state_out, int16_t *near_buf, int16_t *far_buf, void *stream);

/* The vote of one tick, with the carried `silence`: flags u8 [S][windows * (frames - look_backward)] are the next entries of the
 * reference's `saved` list (1 = silence); tail u8 [S][look_backward] is what the plain rule appends if the stream ENDS with this tick -- it
 * does not touch the carried state, so the stream can go on.  channels: that of the record (it sizes the overlap check).  Returns
 * VADX_EINVAL, before any HIP call, for a NULL pointer, streams / n_slots / windows / frames < 1, look_backward outside [1, frames),
 * channels outside {1, 2}, or overlapping records.
 * Replaces the while-loop body + tail, Inference_DFSMN_VAD_ONNX.py:231-273, for S calls that arrive in pieces. */
int vadx_dfsmn_stream_vote(const float *vad, int streams, int n_slots, int windows, int frames, int look_backward, int channels,
                           double speaking_score, double silence_score, const int32_t *slot, const uint8_t *reset,
                           const void *state_in, void *state_out, uint8_t *flags, uint8_t *tail, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Chunks: cut the speech out of a resident batch (or drop it), every clip in one launch sequence -- the batched form of the reference's
 * collect_chunks / drop_chunks (Silero/modeling_modified/utils_vad.py:588-631 / 634-682).  Input is the table vadx_silero_segments
 * writes (or any table of that shape): segments int64 [batch][cap][2] = (start, end) in elements of the clip, counts int32 [batch].
 *
 * A PIECE is a half-open source interval of one clip, resolved by exactly Python's slice rule (what `wav[start:end]` does there): an
 * index i < 0 becomes i + len, it is then clamped to [0, len], and lo >= hi is empty.  Rows may overlap, be unsorted, reversed or out
 * of range; they give what the reference's slicing gives (overlaps duplicate samples in COLLECT, give empty pieces in DROP).
 *   VADX_CHUNKS_COLLECT  (utils_vad.py:588-631)  n = counts[b] pieces:  piece k = [start_k, end_k)
 *   VADX_CHUNKS_DROP     (utils_vad.py:634-682)  n + 1 pieces:          piece k = [cur_k, start_k), cur_0 = 0, cur_k = end_{k-1}; the last
 *                                                                       piece is [cur_n, len)
 * The output is a PACKED vector: clip after clip, each clip's start rounded up to `align` elements (align = 8 int16 gives the 16-byte
 * clip starts of the ragged batches above), the filler between clips -- and after the last one, up to the total -- written as zeros.
 *
 * The PLAN record (device memory, vadx_chunks_plan_bytes(batch, cap) bytes, 16-byte aligned; byte offsets):
 *   0    int64 total                      = clip_dst[batch]: at a fixed offset, so that a host reads 8 bytes and knows what to allocate
 *   8    int32 status                     VADX_CHUNKS_ST_* bits (vadx_chunks_plan resets the word, vadx_chunks_copy only adds bits); 12: int32 0
 *   16   int64 clip_dst  [batch+1]        exclusive prefix of the clips' output lengths, each rounded up to `align`
 *   then int64 piece_dst [batch][cap+2]   exclusive prefix of the piece lengths inside the clip; entry n_pieces -- and every later entry --
 *                                         is the clip's output length
 *   then int64 piece_src [batch][cap+1][2]  the resolved intervals (lo, hi), hi >= lo; (0, 0) beyond n_pieces
 *   then int32 n_pieces  [batch]
 * A clip with counts[b] < 0, counts[b] > cap or clip_len[b] < 0 is a BAD clip: n_pieces = -1, output length 0, VADX_CHUNKS_ST_BAD_CLIP
 * set; its table rows are never read and it copies nothing.  All offsets are 64-bit; batch may be 2^20 and more. */
#define VADX_CHUNKS_COLLECT 0   /* utils_vad.py:588-631 */
#define VADX_CHUNKS_DROP    1   /* utils_vad.py:634-682 */
#define VADX_CHUNKS_ST_BAD_CLIP  1   /* vadx_chunks_plan: some clip's count or length was refused */
#define VADX_CHUNKS_ST_OVERFLOW  2   /* vadx_chunks_copy: total > dst_elems -- NOTHING was written */
#define VADX_CHUNKS_ST_SRC_RANGE 4   /* vadx_chunks_copy: a piece lay outside [0, src_elems) (clip_src / clip_len do not describe src); those
                                        elements were written as zeros, nothing outside src was read */
/* Bytes of the plan record of (batch, cap) that vadx_chunks_plan writes for collect_chunks / drop_chunks (utils_vad.py:588-631 / 634-682);
 * 0 when either is < 1. */
size_t vadx_chunks_plan_bytes(int batch, int cap);
/* The plan of collect_chunks (utils_vad.py:588-631) / drop_chunks (utils_vad.py:634-682) for every clip: two launches on `stream`, no
 * synchronisation.  clip_len int64 [batch] = every clip's length in elements; align: a power of two in [1, 4096].  VADX_EINVAL (before any
 * HIP call) for a NULL pointer, batch / cap < 1, another mode, another align, a misaligned pointer, plan_bytes < vadx_chunks_plan_bytes. */
int vadx_chunks_plan(const int64_t *segments, const int32_t *counts, const int64_t *clip_len, int batch, int cap, int mode, int align,
                     void *plan, size_t plan_bytes, void *stream);
/* The copy of collect_chunks / drop_chunks (utils_vad.py:588-631 / 634-682: the slices and the torch.cat) for every clip: fills
 * dst[0, total) from src by the plan; one launch over 16 KB tiles of the DESTINATION.  elem_bytes 2 (int16 PCM) or 4 (float32); a pure
 * copy.  Clip b's elements start at src[clip_src[b]] (int64 element offsets: b * N for a rectangle [batch][N], the clip offsets of a
 * packed ragged vector otherwise).  src and dst 16-byte aligned, holding src_elems / dst_elems elements: no byte outside
 * [src, src + src_elems) is read, none outside [dst, dst + min(total, dst_elems)) written.  total > dst_elems sets
 * VADX_CHUNKS_ST_OVERFLOW and writes nothing.  VADX_EINVAL (before any HIP call) for a NULL pointer, batch / cap < 1, elem_bytes not 2 or 4,
 * a negative element count, src / dst not 16-byte aligned, plan_bytes < vadx_chunks_plan_bytes, ceil(dst_elems / tile) >= 2^31. */
int vadx_chunks_copy(const void *src, int64_t src_elems, const int64_t *clip_src, int elem_bytes, void *plan, size_t plan_bytes, int batch, int cap,
                     void *dst, int64_t dst_elems, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Timestamps: per-frame decisions or a segment table -> timestamps in seconds AND in samples, for every clip of a resident batch, in
 * one launch (one wave per clip) -- the step between a model's device output and vadx_chunks_plan, which the drivers otherwise do on
 * the host, one clip at a time.  Every number is bit for bit what the reference's Python computes (csrc/timestamps.hip states each rule).
 * Three inputs, one entry point each; all share the second half, process_timestamps (FSMN/Inference_FSMN_VAD_ONNX.py:123-141): rows with
 * (end - start) >= min_duration are kept, a kept row opens a new segment when start - (the previous kept row's end) > fusion_threshold
 * and extends the open one otherwise.  (The reference runs the fuse twice; its second pass compares the same numbers and changes nothing.)
 *
 * Outputs of every call (device memory):
 *   seconds f64   [batch][cap][2]   (start_s, end_s)
 *   samples int64 [batch][cap][2]   the same rows in samples, by params.sample_rule:
 *                                   VADX_TS_NEAREST int(round(s * sampling_rate)), VADX_TS_TRUNC int(s * sampling_rate)
 *                                   -- the table vadx_chunks_plan takes as it is
 *   counts  int32 [batch]           the TRUE number of segments; rows beyond cap are not written (nothing is indexed past cap)
 *   head    16 bytes                int32 status (VADX_TS_ST_* bits), int32 the largest count, 8 bytes of zeros: one small read answers
 *                                   both "did it fit" and "was anything refused"
 * A REFUSED clip (its n_flags / counts_in / n_frames / clip_len outside its table, as listed per call) gets count 0 and sets
 * VADX_TS_ST_BAD_CLIP; none of its input rows is read, none of its output rows written.  VADX_EINVAL, before any HIP call, for a NULL
 * or misaligned pointer, batch < 1, cap outside [1, 2^30], sampling_rate < 1, another sample_rule, process not 0 / 1, a NaN threshold
 * with process = 1, and what each call adds. */
#define VADX_TS_NEAREST 0           /* int(round(s * sr)): vadx.chunks.from_seconds */
#define VADX_TS_TRUNC   1           /* int(s * sr): timestamps_indices.txt, FSMN/Inference_FSMN_VAD_ONNX.py:252-258 */
#define VADX_TS_ST_BAD_CLIP 1       /* some clip was refused (its count is 0) */
#define VADX_TS_ST_OVERFLOW 2       /* some clip has more segments than cap: call again with cap = the head's largest count */
typedef struct vadx_ts_params {
    double frame_s;                 /* FLAGS: seconds per flag (> 0) */
    double fusion_threshold;        /* process_timestamps, used when process = 1 */
    double min_duration;
    float  frame_shift;             /* FRAMES: seconds per frame, float32 as VadPostprocessor holds it (> 0) */
    float  frame_length;            /* FRAMES: added to an end at the end of the audio when use_frame_length = 1 (FireRed 0.025; MarbleNet none) */
    int    use_frame_length;
    int    sampling_rate;           /* the rate of `samples`; SAMPLES: also the divisor, 16000 or 8000 */
    int    process;                 /* 1: process_timestamps after the conversion; 0: the rows go through as they are */
    int    sample_rule;             /* VADX_TS_NEAREST / VADX_TS_TRUNC */
} vadx_ts_params;
/* FLAGS: silence flags uint8 [batch][stride], n_flags int32 [batch] valid per row (what vadx_fsmn_clips* and vadx_dfsmn_vote write;
 * speech = flag 0 at a position < n_flags[b], so the 255 filler of a ragged row is silence).  A run [a, b) of speech gives
 * (a * frame_s, b == n ? n * frame_s : b * frame_s + frame_s), then process_timestamps when process = 1.
 * Replaces vad_to_timestamps + process_timestamps, FSMN/Inference_FSMN_VAD_ONNX.py:102-141 (the DFSMN drivers carry the same code).
 * Refused: n_flags[b] < 0 or > stride.  Also VADX_EINVAL: stride < 0, frame_s not positive and finite. */
int vadx_timestamps_flags(const vadx_ts_params *prm, const uint8_t *flags, int64_t stride, const int32_t *n_flags, int batch,
                          double *seconds, int64_t *samples, int32_t *counts, int cap, void *head, void *stream);
/* FRAMES: the table vadx_vadpost writes, segments int32 [batch][cap_in][2] + counts_in int32 [batch], with n_frames int32 [batch] and
 * wav_dur f64 [batch] (seconds; NaN = none).  float32 frame * frame_shift; when the clip's last row ends at n_frames[b] its end is
 * n_frames[b] * frame_shift (+ frame_length), capped by wav_dur[b], as float32; then Python's round(, 3).  n_frames[b] = 0: no segment.
 * Replaces the tail of decision_to_segment, FireRedVAD/Inference_FireRed_ONNX.py:169-179 (and MarbleNet's copy).
 * Refused: counts_in[b] < 0 or > cap_in, n_frames[b] < 0.  Also VADX_EINVAL: cap_in < 1, frame_shift not positive and finite,
 * use_frame_length not 0 / 1. */
int vadx_timestamps_frames(const vadx_ts_params *prm, const int32_t *segments, const int32_t *counts_in, int cap_in, const int32_t *n_frames,
                           const double *wav_dur, int batch, double *seconds, int64_t *samples, int32_t *counts, int cap, void *head,
                           void *stream);
/* SAMPLES: the table vadx_silero_segments writes, segments int64 [batch][cap_in][2] + counts_in int32 [batch], with clip_len int64
 * [batch]: start = max(round(s / sr, 1), 0), end = min(round(e / sr, 1), clip_len / sr), Python's round (time_resolution = 1 only;
 * |s|, |e|, clip_len < 2^53).  Replaces the return_seconds branch of get_speech_timestamps, Silero/modeling_modified/utils_vad.py:478-482,
 * and with process = 1 the process_timestamps pass of Silero/Inference_Silero_VAD_ONNX.py over its result.
 * Refused: counts_in[b] < 0 or > cap_in, clip_len[b] < 0.  Also VADX_EINVAL: cap_in < 1, sampling_rate not 16000 or 8000. */
int vadx_timestamps_samples(const vadx_ts_params *prm, const int64_t *segments, const int32_t *counts_in, int cap_in, const int64_t *clip_len,
                            int batch, double *seconds, int64_t *samples, int32_t *counts, int cap, void *head, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Test hooks (used by tests/ only)
 * ------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------
 * Audio ingest: the reference drivers' pydub chain set_channels(1).set_frame_rate(r)
 * (FSMN/Inference_FSMN_VAD_ONNX.py:68 and the other four drivers) = audioop.tomono(0.5, 0.5) + audioop.ratecv,
 * bit-exact on 16-bit PCM.  src: batch rows of frames_in interleaved frames (1 or 2 channels), row stride in
 * int16 elements; dst: batch rows of vadx_ingest_out_frames(frames_in, in_rate, out_rate) mono samples.
 * ------------------------------------------------------------------------------------------- */
int64_t vadx_ingest_out_frames(int64_t frames_in, int in_rate, int out_rate);
int vadx_ingest_pcm16(const int16_t *src, int64_t src_stride, int channels, int64_t frames_in, int in_rate,
                      int out_rate, int16_t *dst, int64_t dst_stride, int batch, void *stream);
/* The same arithmetic over a RAGGED batch: the raw interleaved clips lie in one int16 vector `src`, clip b = frames_in[b] frames of
 * channels[b] (1 or 2) channels at in_rate[b] from element src_off[b]; its vadx_ingest_out_frames(frames_in[b], in_rate[b], out_rate)
 * mono samples go to dst from element dst_off[b].  One launch over tiles of 1024 output samples: tile_first int32 [batch + 1] is the prefix
 * of max(1, ceil(out frames / 1024)) tiles per clip (every clip has a tile: its first writes the status), tile_clip int32 [tiles] the clip of
 * every tile.  status int32 [batch] receives VADX_INGEST_ST_* bits per clip: what vadx_ingest_pcm16 refuses for its whole batch (channels not
 * 1 or 2, a rate or frame count that is not positive, frames_in >= 2^31, reduced output rate >= 65536) is refused per clip, and so is a
 * clip whose source range leaves [0, src_elems): its samples are written as zeros, nothing outside src is read.  A clip whose output
 * range leaves [0, dst_elems) writes nothing.  VADX_EINVAL (before any HIP call) for a NULL or misaligned pointer, batch / tiles < 1,
 * out_rate < 1, a negative element count. */
#define VADX_INGEST_ST_BAD_CLIP  1
#define VADX_INGEST_ST_SRC_RANGE 2
#define VADX_INGEST_ST_DST_RANGE 4
int vadx_ingest_pcm16_ragged(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *frames_in, const int32_t *channels,
                             const int32_t *in_rate, int out_rate, const int64_t *dst_off, const int32_t *tile_first, const int32_t *tile_clip,
                             int batch, int tiles, int16_t *dst, int64_t dst_elems, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Prepare: a resident packed vector of clips -> the packed, normalised, grid-padded vector of a ragged batch (vadx.ragged), bit for bit
 * what the host loop builds per clip: normalize_to_int16 (PEAK, FSMN/Inference_FSMN_VAD_ONNX.py:60-63) or normalise_audio (RMS,
 * Inference_NVIDIA_MarbleNet_VAD_ONNX.py:110-118) or nothing (NONE), then pad_to_window_grid's noise at the RMS of the normalised
 * tail (FSMN/Inference_FSMN_VAD_ONNX.py:88-99).  csrc/prepare.hip states the arithmetic: float32, one rounding per operation, and the mean
 * of squares in numpy's own order -- consecutive chunks of 8192 elements added in order, numpy's pairwise tree inside a chunk.
 *
 * Tables (device memory): clip b is lengths[b] samples of src from element src_off[b] (any residue) and owns elements
 * dst_off[b] .. dst_off[b+1]-1 of dst (dst_off int64 [batch + 1], non-decreasing): first its samples, then dst_off[b+1] - dst_off[b] -
 * lengths[b] samples of fill -- the caller lays dst out, by pad_to_window_grid's count for a window grid or end to end for none.  The fill's
 * reference region is the clip's last `fill` samples when lengths[b] > window and the whole clip otherwise.  tile_first int32 [batch + 1] is
 * the prefix of ceil(lengths[b] / 8192) chunks per clip, tile_clip int32 [tiles] the clip of every chunk.
 * The workspace (vadx_prepare_workspace_bytes, 16-byte aligned) starts with one 16-byte record per clip, which the caller may read:
 *   float scale (s or g; 1 when the clip stays as it is), float tail_rms, int32 status (VADX_PREPARE_ST_* bits), int32 0.
 * Three launches on `stream`, in this order, whatever the batch: vadx_prepare_stats (per chunk: peak / sum of squares; not needed for NONE),
 * vadx_prepare_scale (per clip: the record), vadx_prepare_write (per 16 KB of dst: the samples, then fill_k = int16(tail_rms * noise[noise_off[b]
 * + k]) with the product in float64 and the cast as numpy's: toward zero, low 16 bits).  A clip whose source range leaves [0, src_elems), or
 * whose length is < 1, sets VADX_PREPARE_ST_SRC_RANGE: nothing of src is read for it, its elements of dst are zeros.  A fill index outside
 * [0, noise_elems) sets VADX_PREPARE_ST_NOISE_RANGE and writes zero.  A fill count that is neither 0 nor pad_to_window_grid's for (lengths[b],
 * window, stride) sets VADX_PREPARE_ST_GRID (and is honoured).  Elements of dst that no clip owns are written as zeros; nothing outside
 * [dst, dst + dst_elems) is written.
 * VADX_EINVAL (before any HIP call) for a NULL or misaligned pointer (src, dst, workspace: 16 bytes), batch / tiles < 1, a negative
 * element count, window or stride that is not a positive multiple of 8, another mode, target_rms not positive and finite,
 * workspace_bytes < vadx_prepare_workspace_bytes(batch, tiles). */
#define VADX_PREPARE_NONE 0
#define VADX_PREPARE_PEAK 1
#define VADX_PREPARE_RMS  2
#define VADX_PREPARE_ST_SRC_RANGE   1
#define VADX_PREPARE_ST_NOISE_RANGE 2
#define VADX_PREPARE_ST_GRID        4
size_t vadx_prepare_workspace_bytes(int batch, int tiles);
int vadx_prepare_stats(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int32_t *tile_first,
                       const int32_t *tile_clip, int batch, int tiles, int mode, void *workspace, size_t workspace_bytes, void *stream);
int vadx_prepare_scale(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int64_t *dst_off,
                       const int32_t *tile_first, int batch, int tiles, int window, int stride, int mode, float target_rms, void *workspace,
                       size_t workspace_bytes, void *stream);
int vadx_prepare_write(const int16_t *src, int64_t src_elems, const int64_t *src_off, const int64_t *lengths, const int64_t *dst_off,
                       const double *noise, int64_t noise_elems, const int64_t *noise_off, int batch, int tiles, int mode, void *workspace,
                       size_t workspace_bytes, int16_t *dst, int64_t dst_elems, void *stream);

/* Weight layout of every GEMM operand the kernels stream from L2 ("fragment-major"): a row-major
 * [rows][cols] matrix, zero-padded to multiples of 16 both ways, stored as
 * [rows/16 tiles][cols/16 blocks][64 lanes][4]: the float4 of (tile, block S, lane 16q+i) holds
 * W[16*tile + i][16*S + 4*q + 0..3], so one wave-wide load is one contiguous 1 KB run.  The *_pack_host
 * functions produce it themselves; entry points that take bare weight pointers (vadx_sepconv_block's
 * pw_w / res_w, vadx_dfsmn_mask_weights' linear1_w / fsmn_linear_w / fsmn_project_w)
 * expect buffers converted with this helper.  dst holds vadx_frag_major_floats(rows, cols) floats. */
size_t vadx_frag_major_floats(int rows, int cols);
int vadx_frag_major_host(const float *src, int rows, int cols, float *dst);
/* The fp16 x 2 counterpart for the entry points that take bare weight pointers and an `arithmetic` (vadx_marblenet_block2 / _tail):
 * [rows/16 tiles][cols/32 chunks][2 planes][64 lanes][8 fp16], lane 16q+i slot e = W[16*tile + i][32*chunk + k(q, e)], round-to-nearest
 * fp16 terms h0, h1 = (w - h0) * 2^11 (csrc/split2.h).  k_order: VADX_H2_K_PLAIN k = 8q + e (vadx_marblenet_tail's pw / w6),
 * VADX_H2_K_QUARTER k = 16*(e>>2) + 4q + (e&3) (vadx_marblenet_block2's pw0 / pw1 / res_w when cin = 128; with cin = 64 they are K_PLAIN).  dst holds vadx_frag_h2_floats(rows, cols)
 * floats; *wmax_out (optional) receives the largest |w|; fails when a weight is outside the fp16 range (keep that matrix on VADX_ARITH_F32). */
#define VADX_H2_K_PLAIN 0
#define VADX_H2_K_QUARTER 1
size_t vadx_frag_h2_floats(int rows, int cols);
int vadx_frag_h2_host(const float *src, int rows, int cols, int k_order, float *dst, float *wmax_out);

#ifdef __cplusplus
}
#endif
#endif /* VADX_H */
