"""What the GPU tests of the two crop-frame kernels share (tests/test_gpu_pitch.py: dsp_pitch_track,
tests/test_gpu_lpc.py: dsp_lpc_autocorr): guarded outputs, packed clips, the builder of a call's inputs
from hand-made clips and crops, WAV trees, and the batch that walks the kernels' gate (a plain helper
module like tests/knn_edge_cases.py: no test, no fixture)."""
import types
import wave

import numpy as np

import pitch_reference as P
from device_outputs import Guarded  # noqa: F401 -- the two test modules take it from here


def pack(clips, lead=0):
    """int16 clips back to back behind ``lead`` samples that belong to no clip -> (pcm, offsets)."""
    lens = np.array([len(c) for c in clips], np.int64)
    off = lead + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pcm = np.concatenate([np.full(lead, 12345, np.int16)] + [np.asarray(c, np.int16) for c in clips] + [np.full(8, -12345, np.int16)])
    return pcm, off


def given(clips, crops, L, S, status=None, ld=None, lead=0, n_frames=None, untouched=(), max_len=None, stride=0):
    """Hand-made clips with their crops given directly: the host arrays se [B, 2], nf and status (int32;
    n_frames None: each crop's own frame count), ld (None: the largest nf), max_len (None: the longest
    clip), ``skip`` = status with a failing one for the ``untouched`` clips (those the call must leave
    alone although their status is good: what the restatement is given), and the device tensors pcm,
    off and ``fields`` = (start_end, n_frames, status) -- separate arrays for stride 0, slices of
    [B, 19] int32 rows holding them in words 15 .. 18 for stride 19."""
    import torch
    B = len(clips)
    pcm, off = pack(clips, lead)
    se = np.asarray(crops, np.int32).reshape(B, 2)
    nf = np.array([P.frame_count(e - s, L, S) for s, e in se], np.int32) if n_frames is None else np.asarray(n_frames, np.int32)
    status = np.zeros(B, np.int32) if status is None else np.asarray(status, np.int32)
    skip = status.copy()
    skip[list(untouched)] = 1
    dev = lambda a: torch.as_tensor(a).to("cuda")
    if stride == 0:
        fields = (dev(se), dev(nf), dev(status))
    else:
        assert stride == 19
        rows = np.full((B, 19), -3, np.int32)
        rows[:, 15:17], rows[:, 17], rows[:, 18] = se, nf, status
        rows = dev(rows)
        fields = (rows[:, 15:], rows[:, 17:], rows[:, 18:])
    return types.SimpleNamespace(B=B, se=se, nf=nf, status=status, skip=skip, ld=int(nf.max()) if ld is None else ld,
                                 max_len=max(len(c) for c in clips) if max_len is None else max_len, stride=stride,
                                 pcm=dev(pcm), off=dev(off), fields=fields)


def gate_batch():
    """One batch at L = 64, S = 16, ld = 12, max_len = 308 that meets every condition of the kernels' gate:
    ten clips of 300 .. 309 samples,
      0  crop (1, 300), 16 frames > ld           processed, 12 frames
      1  status 3                                untouched
      2  status 0x100 (flag bits only)           processed
      3  crop (-1, 200)                          untouched
      4  crop (120, 100): the end before the start, n_frames 3   untouched
      5  crop (0, 306) on 305 samples            untouched
      6  n_frames 0                              untouched
      7  n_frames -2                             untouched
      8  crop (40, 40), n_frames 1               processed: one all-zero frame
      9  309 samples > max_len                   untouched
    None of these crops lets a kernel read outside pcm: they are the inputs the gate exists to refuse.
    -> the keyword arguments of ``given`` (and of track_given / autocorr_given)."""
    rng = np.random.default_rng(21)
    clips = [rng.integers(-9000, 9000, 300 + j).astype(np.int16) for j in range(10)]
    crops = [(0, len(c)) for c in clips]
    crops[0], crops[3], crops[4], crops[5], crops[8] = (1, 300), (-1, 200), (120, 100), (0, 306), (40, 40)
    nf = [P.frame_count(e - s, 64, 16) for s, e in crops]
    nf[4], nf[6], nf[7], nf[8] = 3, 0, -2, 1
    assert nf[0] == 16 and nf[5] > 0 and nf[9] > 0
    return dict(clips=clips, crops=crops, L=64, S=16, n_frames=nf, status=[0, 3, 0x100, 0, 0, 0, 0, 0, 0, 0], ld=12,
                max_len=308, untouched=(3, 4, 5, 6, 7, 9))


GATE_UNTOUCHED = [1, 3, 4, 5, 6, 7, 9]  # with the failed clip


def _write_wav(path, data, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(data).tobytes())


def wav_tree(tmp_path, per_class, seed, n_samples=20000):
    """Three class directories w0 .. w2 of ``per_class`` synthetic clips of n_samples + 1013 j samples."""
    from src.synth import make_clip
    for c in range(3):
        d = tmp_path / ("w%d" % c)
        d.mkdir()
        for j in range(per_class):
            _write_wav(d / ("s%d.wav" % j), make_clip(seed + 10 * c + j, n_samples=n_samples + 1013 * j, label=c, n_classes=3))
