"""Whole clips on the host: what every model's `detect` does between "clips in host memory" and "seconds per clip", written once.

Before the launches: `pad_to_window_grid` (one clip) and `pad_batch` (a rectangular batch) put audio on a model's sliding-window grid.
After them: `gather_tracks` lays the scores of a ragged batch out as one track per clip, `track_segments` runs a VadPostprocessor over
the tracks of a batch (one launch, one read-back) and `flag_timestamps` turns FSMN / DFSMN silence flags into timestamps.  Nothing here
knows which model calls it: the window grid, the clip preparation, the post-processor with its frame shift, and each clip's duration
in seconds -- which carries the caller's sample rate -- are arguments."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import timestamps as _ts


def pad_count(n, window, stride):
    """How many samples `pad_to_window_grid` appends to a clip of n samples: a function of the three numbers alone, so that the layout of
    a batch is known from its lengths (vadx.prepare)."""
    if n > window:
        return int(np.ceil((n - window) / stride)) * stride + window - n
    return window - n


def pad_to_window_grid(audio_i16, window, stride, noise=None):
    """Tail padding to the sliding-window grid with white noise at the RMS of the tail
    (FSMN/Inference_FSMN_VAD_ONNX.py:88-99).  `noise` = standard-normal samples (seeded by the
    caller); None draws from numpy's global RNG like the reference does."""
    a = np.asarray(audio_i16).reshape(-1)
    n = a.shape[0]
    if n > window:
        num_windows = int(np.ceil((n - window) / stride)) + 1
        pad = (num_windows - 1) * stride + window - n
        if pad == 0:
            return a.copy()
        ref = a[-pad:].astype(np.float32)
    elif n < window:
        pad = window - n
        ref = a.astype(np.float32)
    else:
        return a.copy()
    z = np.random.normal(loc=0.0, scale=1.0, size=pad) if noise is None else np.asarray(noise[:pad], dtype=np.float64)
    fill = (np.sqrt(np.mean(ref * ref)) * z).astype(a.dtype)
    return np.concatenate((a, fill))


def pad_batch(clips, window, stride, pad_noise=None, prep=None):
    """Equal-length clips [B, N] (host) -> (padded [B, N'], W): every row through `prep` (FSMN / DFSMN: peak normalisation to int16;
    None: as it is) and `pad_to_window_grid` with row b of pad_noise (standard-normal [B, >= pad]; None: numpy's global RNG),
    W = (N' - window) // stride + 1 windows per clip."""
    clips = np.asarray(clips)
    B, _ = clips.shape
    rows = [pad_to_window_grid(clips[b] if prep is None else prep(clips[b]), window, stride, None if pad_noise is None else pad_noise[b])
            for b in range(B)]
    padded = np.stack(rows)
    return padded, (padded.shape[1] - window) // stride + 1


def gather_tracks(device, probs, win_floats, offset, frames_per_window, win_first, n_frames):
    """tracks f32 [B, max(n_frames, 1)] on `device` (vadx_tracks_gather): row b = the first n_frames[b] scores of clip b's windows laid
    end to end, zeros after them -- the input of one vadx_vadpost launch.  probs: per-window scores on the device, `win_floats` floats
    per window of which `frames_per_window` from `offset` on are the track's; win_first int32 [B+1] (device), n_frames [B] (host)."""
    t = _lib.require_gpu()
    stride = max(int(n_frames.max()), 1)
    tracks = t.empty((len(n_frames), stride), dtype=t.float32, device=device)
    nfd = t.from_numpy(np.ascontiguousarray(n_frames, dtype=np.int32)).to(device)
    with t.cuda.device(device):
        _lib.check(_lib.lib().vadx_tracks_gather(probs.data_ptr(), win_floats, offset, frames_per_window, win_first.data_ptr(), nfd.data_ptr(),
                                                 len(n_frames), tracks.data_ptr(), stride, _lib.stream_ptr()))
    return tracks


def track_segments(pp, track, n_frames, durations_s):
    """track f32 [B, S] (device) through the VadPostprocessor `pp` -> (per clip [(start_s, end_s)], decisions i8 [B, S] on the device):
    one process_batch launch, one read-back of the segment table, then the seconds arithmetic per clip with its own frame count and
    duration.  n_frames [B] (host): the valid frames of each row, a clip with none gives []; None = all S columns of every row."""
    dec, segs, counts = pp.process_batch(track, n_frames=n_frames)
    segs, counts = segs.cpu().numpy(), counts.cpu().numpy()
    nf = [track.shape[1]] * track.shape[0] if n_frames is None else n_frames
    return [pp.segments_to_seconds(segs[b, :counts[b]].tolist(), int(nf[b]), durations_s[b]) if nf[b] else []
            for b in range(track.shape[0])], dec


def track_table(pp, track, n_frames, durations_s, sampling_rate, sample_rule=0, cap=64):
    """`track_segments` without the frame table leaving the device -> (vadx.tstable.TimestampTable, decisions i8 [B, S] on the device):
    one process_batch launch, one vadx_timestamps_frames launch, one 16-byte read of the table's head.  Only when that head reports a
    clip with more than `cap` segments (refused) is the frame table made again as wide as it must be, the way `process_batch` does."""
    from . import tstable
    nf = [track.shape[1]] * track.shape[0] if n_frames is None else n_frames
    dec, segs, counts = pp.process_batch(track, n_frames=n_frames, cap=cap, check=False)
    table = tstable.from_frames(pp, segs, counts, nf, durations_s, sampling_rate, sample_rule)
    if table.head()[0] & tstable.ST_BAD_CLIP:
        dec, segs, counts = pp.process_batch(track, n_frames=n_frames, cap=cap)
        table = tstable.from_frames(pp, segs, counts, nf, durations_s, sampling_rate, sample_rule)
    return table, dec


def flag_timestamps(flags, frame_s, fusion_threshold, min_speech_duration):
    """One clip's or stream's silence flags (1-D, one per `frame_s` seconds) -> [(start_s, end_s)]: the reference's vad_to_timestamps +
    process_timestamps over its `saved` list."""
    ts = _ts.vad_to_timestamps(np.asarray(flags).astype(bool), frame_s)
    return _ts.process_timestamps(ts, fusion_threshold, min_speech_duration)
