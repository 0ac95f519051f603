"""Overlap synthesis and its scoring: OverlapDetection/scripts/data_augmentation.py on the GPU.

``generate_overlap_segment(wav_list, overlap_path)`` is the reference's function (:20-34): the first
1.5 s of the first utterance is the canvas, every other utterance is laid over it with pydub's
``overlay`` at a random multiple of 100 ms, and the mix is written as a WAV.  The positions are drawn
from the ``random`` module exactly as line 31 draws them, so ``random.seed`` reproduces the reference's
draws; all overlays of a segment are one ``mmla_od_mix`` call (``AudioSegment._overlay_many``).

``overlap_plan`` is the same recipe as a plan over recordings that already sit in one pool (a room's
conditioned enrolment recordings): labelled 1.5 s clips in ``run_overlaps_generator``'s mix of degrees
(:43-52: 50 % with 2 talkers, 30 % with 3, 15 % with 4, 5 % with 5), which ``Context.od_pipeline_mixed``
mixes and classifies without the mixed PCM leaving the device.  ``confusion`` is the scoring of
overlap_detector_temp.py:455-466: rows = truth, columns = predicted, recall and precision of the
overlapped class.

``run_overlaps_generator`` itself is not mirrored: it needs the TIMIT label CSV, and it calls the
non-existent ``str.segment`` (:62), so the reference's own function raises before it writes a clip.
The pyramid blur of ``augment_images`` is out of scope too.

pydub is not installed here; its slicing arithmetic is restated from its published source
(audio_segment.AudioSegment) and parity with the library itself is unpinned.
"""
import random

import numpy as np

from . import _lib
from .audio_segment import AudioSegment

WINDOW = _lib.OD_CLIP       # an utterance of a plan: 1.5 s at 16 kHz
POSITIONS = 13              # randrange(int(1.5 * 10) - 2) multiples of 100 ms = 1600 samples
# run_overlaps_generator's shares of 2, 3, 4 and 5 talkers as cumulative twentieths (3150, 5040, 5985 of 6300)
DEGREE_SHARES = ((2, 10), (3, 16), (4, 19), (5, 20))


def generate_overlap_segment(wav_list, overlap_path, ctx=None):
    """
    :param wav_list: path list of wav files to synthesize the overlapped segment
    :param overlap_path: output path to store the overlapped segment
    A canvas shorter than 0.3 s makes random.randrange raise ValueError, as in the reference.
    """
    canvas = AudioSegment.from_file(wav_list[0], ctx=ctx)
    time_durations = 1.5 if canvas.duration_seconds > 1.5 else canvas.duration_seconds
    canvas = canvas[:time_durations * 1000]

    items = []
    for i in range(1, len(wav_list)):
        sound = AudioSegment.from_file(wav_list[i], ctx=ctx)
        index = random.randrange(int(time_durations * 10) - 2) * 100
        items.append((sound, index, 1))

    canvas._overlay_many(items).export(out_f=overlap_path, format="wav")


def overlap_degree(i, n_overlapped, n_speakers):
    """talkers of overlapped clip i of n_overlapped: run_overlaps_generator's split by index, capped at
    the number of speakers"""
    for degree, twentieths in DEGREE_SHARES:
        if i * 20 < n_overlapped * twentieths:
            return min(degree, n_speakers)
    return min(DEGREE_SHARES[-1][0], n_speakers)


def overlap_plan(lens, speaker_of, n_overlapped, n_single, rng):
    """A plan of n_overlapped + n_single labelled 1.5 s clips over a pool that holds recording r, of
    lens[r] samples and speaker speaker_of[r], behind recording r - 1.  An utterance is one of the whole
    24000-sample windows of a recording.  Overlapped clips come first: clip i has overlap_degree(i, ...)
    talkers, each a window of a different speaker (the reference draws speakers with replacement; distinct
    ones are what the label 'overlapped' needs in a room of few speakers), the first the canvas, the others
    laid over it at rng.randrange(13) * 1600 samples.  Single clips are one window of one speaker.
    rng: a random.Random (or the random module).  -> (MixPlan, labels int32 [n] (1 = overlapped, the
    network's class), talkers int32 [n]).  ValueError without two speakers that have a window."""
    lens = [int(x) for x in lens]
    if len(speaker_of) != len(lens):
        raise ValueError(f'{len(speaker_of)} speakers for {len(lens)} recordings')
    if n_overlapped < 0 or n_single < 0:
        raise ValueError('n_overlapped and n_single must be >= 0')
    windows = {}       # speaker -> pool offsets of its windows
    start = 0
    for n, sp in zip(lens, speaker_of):
        if n < 0:
            raise ValueError('a negative recording length')
        windows.setdefault(sp, []).extend(start + w * WINDOW for w in range(n // WINDOW))
        start += n
    speakers = [sp for sp in windows if windows[sp]]      # in order of first appearance
    if len(speakers) < (2 if n_overlapped else 1 if n_single else 0):
        raise ValueError(f'{len(speakers)} speakers with a whole window of {WINDOW} samples: an overlapped '
                         'clip needs two')

    def utterance(sp):
        return windows[sp][rng.randrange(len(windows[sp]))]

    clips = []
    for i in range(n_overlapped):
        talkers = rng.sample(speakers, overlap_degree(i, n_overlapped, len(speakers)))
        layers = [(utterance(talkers[0]), WINDOW, 0)]
        for sp in talkers[1:]:
            off = utterance(sp)
            layers.append((off, WINDOW, rng.randrange(POSITIONS) * 1600))
        clips.append(layers)
    for _ in range(n_single):
        clips.append([(utterance(speakers[rng.randrange(len(speakers))]), WINDOW, 0)])
    plan = _lib.MixPlan.from_layers(clips)
    labels = np.array([1] * n_overlapped + [0] * n_single, np.int32)
    return plan, labels, plan.n_layers.copy()


def confusion(labels, argmax):
    """overlap_detector_temp.py:455-466: -> (matrix float64 [2,2], rows = truth, columns = predicted;
    recall = tp / (tp + fn) and precision = tp / (tp + fp) of the overlapped class, NaN where the
    denominator is 0).  Clips whose argmax is -1 ('silent') are in neither column and are not counted."""
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    argmax = np.asarray(argmax).astype(np.int64).reshape(-1)
    if labels.shape != argmax.shape:
        raise ValueError(f'{labels.size} labels for {argmax.size} predictions')
    matrix = np.zeros((2, 2))
    for t, p in zip(labels, argmax):
        if t not in (0, 1):
            raise ValueError(f'label {t}: 0 (non-overlapped) or 1 (overlapped)')
        if p in (0, 1):
            matrix[t, p] += 1
    tp, fn, fp = matrix[1, 1], matrix[1, 0], matrix[0, 1]
    recall = tp / (tp + fn) if tp + fn else float('nan')
    precision = tp / (tp + fp) if tp + fp else float('nan')
    return matrix, recall, precision
