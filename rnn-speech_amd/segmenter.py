"""The cut planner of long recordings: from the speech flags and frame energies of ONE row (ops.vad_flags / ops.vad_energy, five bytes
per 10 ms frame, copied to the host) to the sample spans that go through the model as an ordinary mini-batch.  Pure numpy, a pure
function of its arguments:

1. The regions are the maximal runs [a, b) of speech == 1; none: no segments.
2. Lmax = budget - 2 pad.  A region longer than Lmax is split: while b - a > Lmax, c = the frame of the smallest energy_db in
   [a + Lmax // 2, a + Lmax] (both ends included, the LAST such frame on ties); [a, c) is emitted and a = c.
3. The pieces are walked left to right into groups: a piece [a, b) joins the current group [s, e) iff b - s <= Lmax, else the
   group closes and the piece opens the next.  Short phrases share a row: long context, few batches.
4. Every group is padded by `pad` frames on both sides, clipped at 0 and F and at the midpoint (e_left + s_right) // 2 of the gap
   to each neighbour: no frame lies in two segments, and a forced cut (no gap) gets no padding.
5. Sample spans are [s hop, min(n, e hop)).

`budget` is the largest frame count whose span still fits the model (frame_budget): it asks the library's own host-side length
functions, the resampler's and the front end's, instead of re-deriving their rounding."""
import numpy as np

from . import lib as _l
from . import ops

def speech_regions(speech):
    """The maximal runs [a, b) of non-zero flags, left to right."""
    flags = np.asarray(speech).astype(bool)
    edges = np.diff(np.concatenate(([0], flags.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(edges == 1).tolist(), np.flatnonzero(edges == -1).tolist()))


def plan_frames(speech, energy_db, budget, pad):
    """Steps 1 to 4: the segments [s, e) in frames, ordered and disjoint, each at most `budget` long."""
    flags, energy = np.asarray(speech), np.asarray(energy_db)
    F, budget, pad = len(flags), int(budget), int(pad)
    if len(energy) != F:
        raise ValueError("segmenter: %d flags but %d energies" % (F, len(energy)))
    l_max = budget - 2 * pad
    if pad < 0 or l_max < 2:
        raise ValueError("segmenter: a budget of %d frames leaves no room beside 2 x %d frames of padding" % (budget, pad))
    pieces = []
    for a, b in speech_regions(flags):
        while b - a > l_max:
            window = energy[a + l_max // 2:a + l_max + 1]
            c = a + l_max // 2 + (len(window) - 1 - int(np.argmin(window[::-1])))
            pieces.append((a, c))
            a = c
        pieces.append((a, b))
    groups = []
    for a, b in pieces:
        if groups and b - groups[-1][0] <= l_max:
            groups[-1][1] = b
        else:
            groups.append([a, b])
    out = []
    for i, (s, e) in enumerate(groups):
        lo = (groups[i - 1][1] + s) // 2 if i else 0
        hi = (e + groups[i + 1][0]) // 2 if i + 1 < len(groups) else F
        out.append((max(s - pad, lo, 0), min(e + pad, hi, F)))
    return out


def _largest(fits, top):
    """The largest v in 0 .. top with fits(v), fits being true up to some point and false beyond."""
    lo, hi = 0, int(top)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def model_frames(n, rate, load_sr, mode):
    """Frames the front end makes of n samples at `rate` once they are resampled to load_sr: the library's own two length functions."""
    lib = _l.load()
    m = n if int(rate) == int(load_sr) else ops.resample_rows_num_samples(n, rate, load_sr)
    got = lib.amdspeech_frontend_num_frames(ops.MODE_MFCC if mode == "mfcc" else ops.MODE_FBANK, int(m), int(load_sr))
    if got < 0:
        _l.check(got, "frontend_num_frames")
    return got


def frame_budget(rate, hop, load_sr, mode, max_frames):
    """The largest count of `hop`-sample frames at `rate` whose span, resampled to load_sr, gives the front end (mode "mfcc" /
    "fbank") at most max_frames frames; 0 when not even one frame fits."""
    top = (int(max_frames) + 2) * int(rate) // (100 * int(hop)) + 2          # (generous: a front-end frame is 10 ms)
    return _largest(lambda f: model_frames(f * int(hop), rate, load_sr, mode) <= int(max_frames), top)


def min_span_samples(rate, load_sr, mode, n_mfcc=20):
    """The shortest span at `rate` the front end accepts after resampling to load_sr (the check in ops.frontend: mfcc wants more
    than n_dft / 2 samples for the reflect padding, fbank nine frames for its deltas)."""
    n_dft = ops.frontend_plan(mode, load_sr, n_mfcc, 1, 1, 1)["n_dft"]

    def too_short(n):
        m = n if int(rate) == int(load_sr) else ops.resample_rows_num_samples(n, rate, load_sr)
        return m <= n_dft // 2 if mode == "mfcc" else model_frames(n, rate, load_sr, mode) < 9
    return _largest(too_short, 2 * int(rate)) + 1


def plan_spans(speech, energy_db, n_samples, hop, budget, pad, min_samples=1):
    """All five steps: [(start_sample, n_samples, start_frame, end_frame), ...].  A span shorter than min_samples is widened
    symmetrically to it where the row allows; a row shorter than min_samples yields no segment."""
    n, hop, min_samples = int(n_samples), int(hop), int(min_samples)
    if n < min_samples:
        return []
    spans = []
    for s, e in plan_frames(speech, energy_db, budget, pad):
        lo, hi = s * hop, min(n, e * hop)
        if hi - lo < min_samples:
            lo = max(0, min(lo - (min_samples - (hi - lo)) // 2, n - min_samples))
            hi = lo + min_samples
        spans.append((lo, hi - lo, s, e))
    return spans
