"""Script-level drop-ins for the reference's `Inference_*_VAD_ONNX.py` programs: raw audio file(s) in,
`timestamps_second.txt` / `timestamps_indices.txt` out, same constants (as keyword arguments instead
of module-level globals), same stdout summary.  Each function also accepts a LIST of files: FSMN, FireRed and FireRed-AED hand
the list to their engine as ONE ragged batch (vadx.ragged: clips of any lengths, work proportional to the audio), and so does MarbleNet
in both window modes (dynamic axis: vadx.ragged.RaggedFrames, one window per clip; INPUT_AUDIO_LENGTH: each clip on its own window
grid) and both DFSMN drivers (vadx.ragged.RaggedPairs: near / far pairs on a grid of odd window and stride), and the Silero driver
(vadx.ragged.RaggedClips, at 16000 Hz and -- with a model that holds the 8 kHz network -- at 8000).  The
printed RTF is over the total audio duration.  `engine` / `model` may be an engine object, a weight dict, a checkpoint path, or the explicit
opt-in "synthetic:<seed>" (vadx.checkpoints.resolve) -- never an implicit default."""
from __future__ import annotations

import time

import numpy as np

from . import audio_io, timestamps


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _engine_of(cls, spec, *args):
    """`spec` itself when it is an engine object; `cls(spec, *args)` when it is something to build one from: a checkpoint path, a
    weight dict, "synthetic:<seed>" -- or None, which raises there (vadx.checkpoints.resolve: no implicit default)."""
    return cls(spec, *args) if (spec is None or isinstance(spec, (str, dict))) else spec


def _load(files, normalise=False):
    """The files as int16 clips at 16 kHz, through the reference's optional NORMALIZE_AUDIO."""
    clips = [audio_io.load_wav(f, 16000) for f in files]
    return [timestamps.normalise_audio(c) for c in clips] if normalise else clips


def _ingest(files, device):
    """device_ingest=True: the files' raw frames go up once and are down-mixed and resampled to 16 kHz there (audio_io.ingest_ragged)
    -> (pcm on the device, clip_offsets, lengths): what an engine's `ragged_packed` takes.  16-bit PCM wav only."""
    raws = [audio_io.read_wav_raw(f) for f in files]
    return audio_io.ingest_ragged([r[0] for r in raws], [r[1] for r in raws], [r[2] for r in raws], 16000, device)


def _detect_files(detect, clips, as_list, pad_noise):
    """`detect(clips, pad_noise) -> one result per clip` over the clips of a driver call: a list of files goes to the engine as it is,
    ONE ragged batch of clips of any lengths; a single file goes the way it always went, as a [1, N] array (`_grouped`)."""
    return detect(clips, pad_noise) if as_list else _grouped(clips, pad_noise, detect)


def _grouped(clips, noises, run):
    """Run `run(stacked_clips [G, n], stacked_noise or None) -> list of G results` once per group of equal-length clips
    (one device batch each) and hand the results back in input order.  A clip may be a [channels, n] array (DFSMN's near / far
    pairs: stacked to [G, 2, n]); `noises` is then a tuple with one entry per channel, and `run` gets one stacked noise per entry."""
    by_len = {}
    for k, c in enumerate(clips):
        by_len.setdefault(c.shape[-1], []).append(k)
    out = [None] * len(clips)
    for idx in by_len.values():
        stacked = [_stack_noise(nz, idx) for nz in (noises if isinstance(noises, tuple) else (noises,))]
        for k, r in zip(idx, run(np.stack([clips[k] for k in idx]), *stacked)):
            out[k] = r
    return out


def _stack_noise(noises, idx):
    """Per-clip pad-noise rows of one length group as a matrix: rows may be ragged (each clip ran alone in the reference), so
    they are trimmed to the group's shortest row -- the engines take `[B, >= pad]` and use the first `pad` samples."""
    if noises is None:
        return None
    rows = [np.asarray(noises[k]).reshape(-1) for k in idx]
    n = min(len(r) for r in rows)
    return np.stack([r[:n] for r in rows])


def _table_files(detect_table, clips, as_list, pad_noise):
    """`_detect_files` for the `detect_table` calls (save_speech_audio): a list of files is one ragged batch, a single file a [1, N]
    array with its noise row -> the vadx.tstable.TimestampTable of the call."""
    if as_list:
        return detect_table(clips, pad_noise)
    return detect_table(clips[0][None, :], _stack_noise(pad_noise, [0]))


def _finish_speech(files, table, save_speech_audio, device, save_second, save_indices, single, elapsed, echo):
    """The end of a driver call that was given save_speech_audio (a wav path; for a list of files `<path>.<k>`, as the timestamp files):
    the call ran its engine's `detect_table`, so the timestamps are a device table (vadx.tstable).  The files' int16 samples inside
    them are cut from that table (vadx.chunks) -- no timestamp crosses to the host in between -- and the timestamp files are written
    from the table's one read-back."""
    _save_speech(files, table, 16000, save_speech_audio, single, device)
    return _finish(table.lists(), 16000, save_second, save_indices, single, elapsed, echo)


def _finish(all_ts, sample_rate, save_second, save_indices, single, elapsed, echo):
    if single:
        timestamps.write_timestamp_files(all_ts[0], sample_rate, save_second, save_indices, echo)
    else:
        for k, ts in enumerate(all_ts):
            timestamps.write_timestamp_files(ts, sample_rate, f"{save_second}.{k}", f"{save_indices}.{k}", lambda *_: None)
    echo(f"\nVAD Process Complete.\n\nTime Cost: {elapsed:.3f} Seconds")
    return all_ts[0] if single else all_ts


def inference_silero(test_vad_audio="./vad_sample.wav", model=None, save_timestamps_second="./timestamps_second.txt",
                     save_timestamps_indices="./timestamps_indices.txt", ACTIVATE_THRESHOLD=0.5, FUSION_THRESHOLD=0.3,
                     MIN_SPEECH_DURATION=0.25, MAX_SPEECH_DURATION=20, MIN_SILENCE_DURATION=250, SAMPLE_RATE=16000,
                     use_fp16=False, echo=print, save_speech_audio=None):
    """Silero/Inference_Silero_VAD_ONNX.py:80-120.  use_fp16 (:16, :83): the samples are quantised to float16 and scaled there, as
    the reference feeds its fp16-optimised model -- I/O-compatible: the network arithmetic here stays float32.
    save_speech_audio (off by default, not in the reference script): a wav path -- for a list of files `<path>.<k>`, as the timestamp
    files -- that receives the file's int16 samples inside the written timestamps, cut out on the device (vadx.chunks)."""
    from . import silero
    files = _as_list(test_vad_audio)
    model = silero.load_silero_vad(onnx=True, use_cpu=True, path=model) if (model is None or isinstance(model, (str, dict))) else model
    if use_fp16:            # np.array(samples, dtype=float16) * 0.000030517578: NumPy keeps float16 (the constant is 2^-15: exact, subnormals round)
        clips = [(audio_io.load_wav(f, SAMPLE_RATE).astype(np.float16) * np.float16(0.000030517578)).astype(np.float32) for f in files]
    else:
        clips = [audio_io.load_wav(f, SAMPLE_RATE).astype(np.float32) * np.float32(0.000030517578) for f in files]
    echo("\nStart to run the VAD process.")
    t0 = time.time()
    # the network follows SAMPLE_RATE where the model holds the 8 kHz one (otherwise, as the reference script, the 16 kHz default runs)
    rate = 8000 if (SAMPLE_RATE == 8000 and getattr(getattr(model, "engine", model), "has_8k", False)) else 16000
    if len(clips) > 1 and (SAMPLE_RATE == 16000 or rate == 8000):       # a list of files: one ragged batch (every file pays for its own windows)
        batch, lengths = clips, None
    else:
        n = max(len(c) for c in clips)
        batch, lengths = np.zeros((len(clips), n), np.float32), [len(c) for c in clips]
        for k, c in enumerate(clips):
            batch[k, :len(c)] = c
    res = silero.get_speech_timestamps_batch(batch, model, lengths=lengths, threshold=ACTIVATE_THRESHOLD, sampling_rate=rate,
                                             max_speech_duration_s=MAX_SPEECH_DURATION,
                                             min_speech_duration_ms=int(MIN_SPEECH_DURATION * 1000),
                                             min_silence_duration_ms=MIN_SILENCE_DURATION, return_seconds=True)
    elapsed = time.time() - t0
    echo(f"\nVAD Complete. Time Cost: {elapsed:.3f} seconds.")
    all_ts = [timestamps.process_timestamps([(d["start"], d["end"]) for d in r], FUSION_THRESHOLD, MIN_SPEECH_DURATION) for r in res]
    if save_speech_audio is not None:
        _save_speech(files, all_ts, SAMPLE_RATE, save_speech_audio, not isinstance(test_vad_audio, (list, tuple)), getattr(model, "engine", model).device)
    return _finish(all_ts, SAMPLE_RATE, save_timestamps_second, save_timestamps_indices, not isinstance(test_vad_audio, (list, tuple)), elapsed, echo)


def _save_speech(files, all_ts, sample_rate, path, single, device):
    """Every file's int16 samples inside its (start_s, end_s) timestamps as a wav: the clips go up once as a packed vector, ONE
    collect_chunks_batch cuts them all, the packed speech comes back once.  all_ts: the host lists, uploaded as a table -- or a
    vadx.tstable.TimestampTable, whose sample rows are on the device already (no timestamp crosses to the host for the cut)."""
    import torch
    from . import chunks
    pcm = [audio_io.load_wav(f, sample_rate) for f in files]
    lens = np.asarray([len(c) for c in pcm], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum((lens + 7) // 8 * 8)]).astype(np.int64)       # every clip on a 16-byte boundary
    flat = np.zeros(int(starts[-1]), np.int16)
    for k, c in enumerate(pcm):
        flat[starts[k]:starts[k] + len(c)] = c
    table = all_ts.chunks_table() if hasattr(all_ts, "chunks_table") else chunks.from_seconds(all_ts, sample_rate)
    packed, offsets, plan = chunks.collect_chunks_batch(table, torch.from_numpy(flat).to(device), lengths=lens, clip_offsets=starts[:-1], return_plan=True)
    packed, offsets, n = packed.cpu().numpy(), offsets.cpu().numpy(), plan.lengths.cpu().numpy()
    for k in range(len(files)):
        audio_io.save_wav(path if single else f"{path}.{k}", packed[offsets[k]:offsets[k] + n[k]], sample_rate)


def inference_fsmn(test_vad_audio="./vad_sample.wav", engine=None, save_timestamps_second="./timestamps_second.txt",
                   save_timestamps_indices="./timestamps_indices.txt", FUSION_THRESHOLD=0.3, MIN_SPEECH_DURATION=0.2,
                   SPEAKING_SCORE=0.5, SILENCE_SCORE=0.5, LOOK_BACKWARD=0.3, SNR_THRESHOLD=10.0,
                   BACKGROUND_NOISE_dB_INIT=30.0, ONE_MINUS_SPEECH_THRESHOLD=1.0, pad_noise=None, echo=print, save_speech_audio=None,
                   device_ingest=False):
    """FSMN/Inference_FSMN_VAD_ONNX.py:66-260.  save_speech_audio: `_finish_speech`.
    device_ingest (off by default): the files' raw frames are uploaded once; down-mix, resampling, peak normalisation, padding and
    packing run on the device (`_ingest`, FsmnEngine.ragged_packed) -- the same timestamps, no per-clip host loop."""
    from . import fsmn
    engine = _engine_of(fsmn.FsmnEngine, engine)
    files, single = _as_list(test_vad_audio), not isinstance(test_vad_audio, (list, tuple))
    if device_ingest:
        clips = engine.ragged_packed(*_ingest(files, engine.device), pad_noise=pad_noise, look_backward_s=LOOK_BACKWARD)
        single_clips, pad_noise = False, None                   # one packed batch, its noise already in it
    else:
        clips, single_clips = _load(files), single
    echo("\nRunning the FSMN_VAD by ONNX Runtime.")
    t0 = time.time()
    kw = dict(fusion_threshold=FUSION_THRESHOLD, min_speech_duration=MIN_SPEECH_DURATION, look_backward_s=LOOK_BACKWARD,
              speaking_score=SPEAKING_SCORE, silence_score=SILENCE_SCORE, snr_threshold=SNR_THRESHOLD,
              noise_init_dB=BACKGROUND_NOISE_dB_INIT, one_minus_speech_threshold=ONE_MINUS_SPEECH_THRESHOLD)
    # (the int16 clips as they are: `detect` widens each to float32 itself before its peak normalisation)
    if save_speech_audio is not None:
        table = _table_files(lambda c, nz: engine.detect_table(c, pad_noise=nz, **kw), clips, not single_clips, pad_noise)
        return _finish_speech(files, table, save_speech_audio, engine.device, save_timestamps_second, save_timestamps_indices, single,
                              time.time() - t0, echo)
    all_ts = _detect_files(lambda c, nz: engine.detect(c, pad_noise=nz, **kw), clips, not single_clips, pad_noise)
    elapsed = time.time() - t0
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, not isinstance(test_vad_audio, (list, tuple)), elapsed, echo)


def inference_fsmn_stream(test_vad_audio="./vad_sample.wav", engine=None, save_timestamps_second="./timestamps_second.txt",
                          save_timestamps_indices="./timestamps_indices.txt", FUSION_THRESHOLD=0.3, MIN_SPEECH_DURATION=0.2,
                          SPEAKING_SCORE=0.5, SILENCE_SCORE=0.5, LOOK_BACKWARD=0.3, SNR_THRESHOLD=10.0,
                          BACKGROUND_NOISE_dB_INIT=30.0, ONE_MINUS_SPEECH_THRESHOLD=1.0, pad_noise=None, echo=print, windows_per_tick=1):
    """FSMN/Inference_FSMN_VAD_ONNX.py:66-260 with every file fed as a LIVE STREAM: the files of a list are the streams of one batch
    (FsmnEngine.stream_detect: ragged ticks, every file advancing by up to `windows_per_tick` windows per tick until the longest is
    done) -> the outputs `inference_fsmn` produces for the same files."""
    from . import fsmn
    engine = _engine_of(fsmn.FsmnEngine, engine)
    files, single = _as_list(test_vad_audio), not isinstance(test_vad_audio, (list, tuple))
    clips = _load(files)
    echo("\nRunning the FSMN_VAD by ONNX Runtime (streamed).")
    t0 = time.time()
    all_ts = engine.stream_detect(clips, windows_per_tick=windows_per_tick, pad_noise=pad_noise, fusion_threshold=FUSION_THRESHOLD,
                                  min_speech_duration=MIN_SPEECH_DURATION, look_backward_s=LOOK_BACKWARD, speaking_score=SPEAKING_SCORE,
                                  silence_score=SILENCE_SCORE, snr_threshold=SNR_THRESHOLD, noise_init_dB=BACKGROUND_NOISE_dB_INIT,
                                  one_minus_speech_threshold=ONE_MINUS_SPEECH_THRESHOLD)
    elapsed = time.time() - t0
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, single, elapsed, echo)


def inference_firered(test_vad_audio="./vad_sample.wav", engine=None, save_timestamps_second="./timestamps_second.txt",
                      save_timestamps_indices="./timestamps_indices.txt", NORMALIZE_AUDIO=False, SMOOTH_WINDOW_SIZE=5,
                      SPEAKING_SCORE=0.4, MIN_SPEECH_FRAME=20, MAX_SPEECH_FRAME=2000, MIN_SILENCE_FRAME=20,
                      MERGE_SILENCE_FRAME=5, EXTEND_SPEECH_FRAME=0, pad_noise=None, echo=print, save_speech_audio=None,
                      device_ingest=False):
    """FireRedVAD/Inference_FireRed_ONNX.py:523-613 (RUN_VAD).  save_speech_audio: `_finish_speech`.
    device_ingest (off by default): as inference_fsmn's; NORMALIZE_AUDIO then runs on the device too."""
    from . import firered
    engine = _engine_of(firered.FireRedEngine, engine)
    files, single = _as_list(test_vad_audio), not isinstance(test_vad_audio, (list, tuple))
    if device_ingest:
        clips = engine.ragged_packed(*_ingest(files, engine.device), pad_noise=pad_noise, normalize="rms" if NORMALIZE_AUDIO else None)
        single_clips, pad_noise, n_samples = False, None, int(clips.lengths.sum())
    else:
        clips, single_clips = _load(files, NORMALIZE_AUDIO), single
        n_samples = sum(len(c) for c in clips)
    echo("\nRunning the FireRedVAD by ONNX Runtime.")
    t0 = time.time()
    post = (SMOOTH_WINDOW_SIZE, SPEAKING_SCORE, MIN_SPEECH_FRAME, MAX_SPEECH_FRAME, MIN_SILENCE_FRAME,
            MERGE_SILENCE_FRAME, EXTEND_SPEECH_FRAME)
    table = None
    if save_speech_audio is not None:
        table = _table_files(lambda c, nz: engine.detect_table(c, pad_noise=nz, post=post), clips, not single_clips, pad_noise)
    else:
        all_ts = _detect_files(lambda c, nz: engine.detect(c, pad_noise=nz, post=post), clips, not single_clips, pad_noise)
    elapsed = time.time() - t0
    echo(f"RTF: {elapsed / (n_samples / 16000):.4f}")
    if table is not None:
        return _finish_speech(files, table, save_speech_audio, engine.device, save_timestamps_second, save_timestamps_indices, single, elapsed, echo)
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, not isinstance(test_vad_audio, (list, tuple)), elapsed, echo)


def inference_firered_aed(test_aed_audio="./vad_sample.wav", engine=None, NORMALIZE_AUDIO=False, SMOOTH_WINDOW_SIZE=5,
                          SPEAKING_SCORE=0.4, SINGING_THRESHOLD=0.5, MUSIC_THRESHOLD=0.5, MIN_EVENT_FRAME=20,
                          MAX_EVENT_FRAME=2000, MIN_SILENCE_FRAME=20, MERGE_SILENCE_FRAME=5, EXTEND_SPEECH_FRAME=0,
                          pad_noise=None, echo=print):
    """FireRedVAD/Inference_FireRed_ONNX.py:620-742 (RUN_AED): -> (event2timestamps, event2ratio) per file."""
    from . import firered
    engine = _engine_of(firered.FireRedEngine, engine)
    clips = _load(_as_list(test_aed_audio), NORMALIZE_AUDIO)
    echo("\nRunning the FireRedAED by ONNX Runtime.")
    t0 = time.time()
    post = (SMOOTH_WINDOW_SIZE, MIN_EVENT_FRAME, MAX_EVENT_FRAME, MIN_SILENCE_FRAME, MERGE_SILENCE_FRAME, EXTEND_SPEECH_FRAME)
    thresholds = (SPEAKING_SCORE, SINGING_THRESHOLD, MUSIC_THRESHOLD)
    if isinstance(test_aed_audio, (list, tuple)):          # files of any lengths: one ragged batch
        results = engine.detect_events(clips, pad_noise=pad_noise, thresholds=thresholds, post=post)
    else:
        nz = None if pad_noise is None else np.asarray(pad_noise[0])[None, :]
        results = engine.detect_events(clips[0][None, :], pad_noise=nz, thresholds=thresholds, post=post)
    elapsed = time.time() - t0
    for (ts, ratio), c in zip(results, clips):
        echo(f"\nAED Results:\n  Audio duration: {len(c) / 16000:.3f}s\n  Event ratios: {ratio}")
        for event, seg in ts.items():
            echo(f"\n  [{event}] segments ({len(seg)}):")
            for a, b in seg:
                echo(f"    {timestamps.format_time(a)} --> {timestamps.format_time(b)}")
    echo(f"\nAED Process Complete.\n\nTime Cost: {elapsed:.3f} Seconds\nRTF: {elapsed / (len(clips[0]) / 16000):.4f}")
    return results[0] if not isinstance(test_aed_audio, (list, tuple)) else results


def inference_firered_stream(test_vad_audio="./vad_sample.wav", engine=None, NORMALIZE_AUDIO=False, SMOOTH_WINDOW_SIZE=5,
                             STREAM_VAD_THRESHOLD=0.4, PAD_START_FRAME=5, MIN_SPEECH_FRAME_STREAM=8,
                             MAX_SPEECH_FRAME_STREAM=2000, MIN_SILENCE_FRAME_STREAM=20, STREAM_CHUNK_SAMPLES=2560, echo=print,
                             batched=False, CHUNKS_PER_TICK=1):
    """FireRedVAD/Inference_FireRed_ONNX.py:744-840 (RUN_STREAM_VAD): -> [(start_s, end_s)] per file.
    batched=True with a list of files runs them as the streams of one batch (FireRedEngine.stream_detect over the list: all files tick
    together on the chunk grid) instead of one file after the other; CHUNKS_PER_TICK = k > 1 then advances every file by up to k
    chunks per tick (ragged ticks: the same segments in a k-th of the launches)."""
    from . import firered
    engine = _engine_of(firered.FireRedEngine, engine, STREAM_CHUNK_SAMPLES)
    clips = _load(_as_list(test_vad_audio), NORMALIZE_AUDIO)
    echo("\nRunning the FireRedStreamVAD by ONNX Runtime.")
    t0 = time.time()
    post = (SMOOTH_WINDOW_SIZE, STREAM_VAD_THRESHOLD, PAD_START_FRAME, MIN_SPEECH_FRAME_STREAM, MAX_SPEECH_FRAME_STREAM,
            MIN_SILENCE_FRAME_STREAM)
    results = []
    if batched and isinstance(test_vad_audio, (list, tuple)):
        results = engine.stream_detect(list(clips), chunk=STREAM_CHUNK_SAMPLES, post=post, chunks_per_tick=CHUNKS_PER_TICK)
    else:
        for c in clips:
            results += engine.stream_detect(c[None, :], chunk=STREAM_CHUNK_SAMPLES, post=post)
    elapsed = time.time() - t0
    for seg, c in zip(results, clips):
        echo(f"\nStream-VAD Results:\n  Audio duration: {len(c) / 16000:.3f}s\n  Segments detected: {len(seg)}\n\n  Timestamps in Second:")
        for a, b in seg:
            echo(f"    {timestamps.format_time(a)} --> {timestamps.format_time(b)}")
    echo(f"\nStream-VAD Process Complete.\n\nTime Cost: {elapsed:.3f} Seconds\nRTF: {elapsed / (len(clips[0]) / 16000):.4f}")
    return results[0] if not isinstance(test_vad_audio, (list, tuple)) else results


def inference_marblenet_stream(test_vad_audio="./vad_sample.wav", engine=None, chunk_frames=16, NORMALIZE_AUDIO=False, SMOOTH_WINDOW_SIZE=3,
                               SPEAKING_SCORE=0.5, MIN_SPEECH_FRAME=10, MAX_SPEECH_FRAME=1000, MIN_SILENCE_FRAME=10,
                               MERGE_SILENCE_FRAME=3, EXTEND_SPEECH_FRAME=0, echo=print):
    """NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-135, 369-388 (the dynamic-axis call) with every file fed as a LIVE STREAM:
    the files of a list are the streams of one batch (MarbleNetEngine.stream_detect: all files tick together, `chunk_frames` frames of
    20 ms per tick, each file with its own final tick) -> [(start_s, end_s)] per file, the segments `inference_marblenet` gives."""
    from . import marblenet
    engine = _engine_of(marblenet.MarbleNetEngine, engine)
    clips = _load(_as_list(test_vad_audio), NORMALIZE_AUDIO)
    echo("\nRunning the NVIDIA_VAD by ONNX Runtime (streamed).")
    t0 = time.time()
    post = (SMOOTH_WINDOW_SIZE, SPEAKING_SCORE, MIN_SPEECH_FRAME, MAX_SPEECH_FRAME, MIN_SILENCE_FRAME, MERGE_SILENCE_FRAME, EXTEND_SPEECH_FRAME)
    results = engine.stream_detect(list(clips), chunk_frames=chunk_frames, post=post)
    elapsed = time.time() - t0
    for seg, c in zip(results, clips):
        echo(f"\nStream Results:\n  Audio duration: {len(c) / 16000:.3f}s\n  Segments detected: {len(seg)}\n\n  Timestamps in Second:")
        for a, b in seg:
            echo(f"    {timestamps.format_time(a)} --> {timestamps.format_time(b)}")
    # the files tick together as one batch: the wall time is set against the longest of them
    echo(f"\nStream Process Complete.\n\nTime Cost: {elapsed:.3f} Seconds\nRTF: {elapsed / (max(len(c) for c in clips) / 16000):.4f}")
    return results[0] if not isinstance(test_vad_audio, (list, tuple)) else results


def inference_marblenet(test_vad_audio="./vad_sample.wav", engine=None, save_timestamps_second="./timestamps_second.txt",
                        save_timestamps_indices="./timestamps_indices.txt", NORMALIZE_AUDIO=False, SMOOTH_WINDOW_SIZE=3,
                        SPEAKING_SCORE=0.5, MIN_SPEECH_FRAME=10, MAX_SPEECH_FRAME=1000, MIN_SILENCE_FRAME=10,
                        MERGE_SILENCE_FRAME=3, EXTEND_SPEECH_FRAME=0, INPUT_AUDIO_LENGTH=None, pad_noise=None, echo=print,
                        save_speech_audio=None, device_ingest=False):
    """NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:120-422 (dynamic axis: one window per clip).  save_speech_audio: `_finish_speech`.
    device_ingest (off by default): as inference_fsmn's, in either window mode; NORMALIZE_AUDIO then runs on the device too."""
    from . import marblenet
    engine = _engine_of(marblenet.MarbleNetEngine, engine)
    files, single = _as_list(test_vad_audio), not isinstance(test_vad_audio, (list, tuple))
    if device_ingest:
        clips = engine.ragged_packed(*_ingest(files, engine.device), window_len=INPUT_AUDIO_LENGTH, pad_noise=pad_noise,
                                     normalize="rms" if NORMALIZE_AUDIO else None)
        single_clips, pad_noise = False, None
    else:
        clips, single_clips = _load(files, NORMALIZE_AUDIO), single
    echo("\nRunning the NVIDIA_VAD by ONNX Runtime.")
    t0 = time.time()
    post = (SMOOTH_WINDOW_SIZE, SPEAKING_SCORE, MIN_SPEECH_FRAME, MAX_SPEECH_FRAME, MIN_SILENCE_FRAME,
            MERGE_SILENCE_FRAME, EXTEND_SPEECH_FRAME)
    if save_speech_audio is not None:
        table = _table_files(lambda c, nz: engine.detect_table(c, window_len=INPUT_AUDIO_LENGTH, pad_noise=nz, post=post), clips, not single_clips,
                             pad_noise)
        return _finish_speech(files, table, save_speech_audio, engine.device, save_timestamps_second, save_timestamps_indices, single,
                              time.time() - t0, echo)
    all_ts = _detect_files(lambda c, nz: engine.detect(c, window_len=INPUT_AUDIO_LENGTH, pad_noise=nz, post=post), clips, not single_clips, pad_noise)
    elapsed = time.time() - t0
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, not isinstance(test_vad_audio, (list, tuple)), elapsed, echo)


def inference_dfsmn(test_near_end_audio="./examples/nearend_mic.wav", test_far_end_audio="./examples/farend_speech.wav", engine=None,
                    save_timestamps_second="./timestamps_second.txt", save_timestamps_indices="./timestamps_indices.txt",
                    SPEAKING_SCORE=0.5, SILENCE_SCORE=0.5, FUSION_THRESHOLD=0.3, MIN_SPEECH_DURATION=0.2,
                    pad_noise_near=None, pad_noise_far=None, echo=print, save_speech_audio=None):
    """DFSMN/near_and_far_end_audio/Inference_DFSMN_VAD_ONNX.py:121-300: near-end mic + far-end reference -> AEC ->
    mask-net VAD -> look-ahead vote -> timestamps (both text files).  Lists of paths run as ONE ragged batch of clip pairs of any lengths.
    save_speech_audio: `_finish_speech`, cut from the near-end file."""
    from . import dfsmn
    nears, fars = _as_list(test_near_end_audio), _as_list(test_far_end_audio)
    engine = _engine_of(dfsmn.DfsmnEngine, engine)
    echo(f"\nTest Input Near_End Audio: {test_near_end_audio}\nTest Input Far_End Audio: {test_far_end_audio}")
    pairs = []
    for pn, pf in zip(nears, fars):                 # files are read before the clock starts, like the reference script
        a, f = audio_io.load_wav(pn, 16000).astype(np.float32), audio_io.load_wav(pf, 16000).astype(np.float32)
        n = min(len(a), len(f))
        pairs.append(np.stack([a[:n], f[:n]]))
    t0 = time.time()
    kw = dict(fusion_threshold=FUSION_THRESHOLD, min_speech_duration=MIN_SPEECH_DURATION, speaking_score=SPEAKING_SCORE, silence_score=SILENCE_SCORE)

    def detect(pr, *nz):
        """a list of [2, n] pairs with the (near, far) noise tuple (_detect_files), or a stacked [1, 2, n] with one noise per side (_grouped);
        the noise of each side independently, either may be None"""
        if isinstance(pr, list):
            return engine.detect([p[0] for p in pr], [p[1] for p in pr], *nz[0], **kw)
        return engine.detect(pr[:, 0], pr[:, 1], *nz, **kw)
    if save_speech_audio is not None:
        single = not isinstance(test_near_end_audio, (list, tuple))
        if single:
            table = engine.detect_table(pairs[0][None, 0], pairs[0][None, 1], _stack_noise(pad_noise_near, [0]), _stack_noise(pad_noise_far, [0]), **kw)
        else:
            table = engine.detect_table([p[0] for p in pairs], [p[1] for p in pairs], pad_noise_near, pad_noise_far, **kw)
        return _finish_speech(nears, table, save_speech_audio, engine.device, save_timestamps_second, save_timestamps_indices, single,
                              time.time() - t0, echo)
    all_ts = _detect_files(detect, pairs, isinstance(test_near_end_audio, (list, tuple)), (pad_noise_near, pad_noise_far))
    elapsed = time.time() - t0
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, not isinstance(test_near_end_audio, (list, tuple)), elapsed, echo)


def inference_dfsmn_near_only(test_vad_audio="./vad_sample.wav", engine=None, save_timestamps_second="./timestamps_second.txt",
                              save_timestamps_indices="./timestamps_indices.txt", SPEAKING_SCORE=0.5, SILENCE_SCORE=0.5,
                              FUSION_THRESHOLD=0.3, MIN_SPEECH_DURATION=0.2, pad_noise=None, echo=print, save_speech_audio=None):
    """DFSMN/only_near_end_audio/Inference_DFSMN_VAD_ONNX.py: one microphone file in, timestamps out (a list of files:
    one ragged batch).  `engine` must
    carry the export's baked white-noise constants (DfsmnEngine.set_near_only_constants).  save_speech_audio: `_finish_speech`."""
    from . import dfsmn, weights
    files = _as_list(test_vad_audio)
    if engine is None or isinstance(engine, (str, dict)):
        raise ValueError("inference_dfsmn_near_only needs a DfsmnEngine carrying the export's baked white-noise constants "
                         "(DfsmnEngine.set_near_only_constants); weights.dfsmn_near_only_constants(seed) gives a stand-in")
    echo(f"\nTest Input Audio: {test_vad_audio}")
    clips = [audio_io.load_wav(pth, 16000).astype(np.float32) for pth in files]
    t0 = time.time()
    if save_speech_audio is not None:
        single = not isinstance(test_vad_audio, (list, tuple))
        table = _table_files(lambda c, nz: engine.detect_table(c, None, nz, None, fusion_threshold=FUSION_THRESHOLD, min_speech_duration=MIN_SPEECH_DURATION,
                                                               speaking_score=SPEAKING_SCORE, silence_score=SILENCE_SCORE), clips, not single, pad_noise)
        return _finish_speech(files, table, save_speech_audio, engine.device, save_timestamps_second, save_timestamps_indices, single,
                              time.time() - t0, echo)
    all_ts = _detect_files(lambda c, nz: engine.detect(c, None, nz, None, fusion_threshold=FUSION_THRESHOLD, min_speech_duration=MIN_SPEECH_DURATION,
                                                       speaking_score=SPEAKING_SCORE, silence_score=SILENCE_SCORE),
                           clips, isinstance(test_vad_audio, (list, tuple)), pad_noise)
    elapsed = time.time() - t0
    return _finish(all_ts, 16000, save_timestamps_second, save_timestamps_indices, not isinstance(test_vad_audio, (list, tuple)), elapsed, echo)
