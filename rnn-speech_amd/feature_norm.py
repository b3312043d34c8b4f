"""Corpus statistics for global feature normalisation (config key `feature_norm : global`): mean and variance of every feature dim
over the training set, accumulated from the per-row moments of ops.feature_moments and kept in an .npz beside the description of
the features they were taken from.  Host arithmetic in float64, rows merged in row order: the result is deterministic."""
import numpy as np

MODES = ("none", "utterance", "global")
VAR_FLOOR = 1e-10
_KEYS = ("signal_processing", "n_mfcc", "sample_rate", "width")


def describe(signal_processing, n_mfcc, sample_rate, width):
    """What a statistics file is valid for.  n_mfcc only shapes mfcc features: fbank files carry 0."""
    return dict(signal_processing=str(signal_processing), n_mfcc=int(n_mfcc) if signal_processing == "mfcc" else 0,
                sample_rate=int(sample_rate), width=int(width))


def describe_processor(audio):
    return describe(audio.feature_type, audio.n_mfcc, audio.load_sr, audio.source_feature_size)


class FeatureStats(object):
    """count frames seen so far, their mean[D] and M2[D] = sum (x - mean)^2, all float64."""

    def __init__(self, description):
        self.description = dict(description)
        D = int(self.description["width"])
        self.count = 0.0
        self.mean = np.zeros(D, np.float64)
        self.M2 = np.zeros(D, np.float64)

    @property
    def var(self):
        """Population variance per dim."""
        return self.M2 / self.count if self.count > 0 else np.zeros_like(self.M2)

    def merge_moments(self, moments, n_frames, t_in):
        """moments float64 [B, 2, D] (ops.feature_moments: mean and M2 per row), n_frames the rows' UNtruncated counts, t_in the
        frames the tensor held: row by row, in row order, with the pairwise update (Chan et al.)."""
        moments = np.asarray(moments, np.float64)
        if moments.ndim != 3 or moments.shape[1:] != (2, self.mean.shape[0]):
            raise ValueError("FeatureStats: moments are %s, expected [B, 2, %d]" % (moments.shape, self.mean.shape[0]))
        for b in range(moments.shape[0]):
            n = float(min(int(n_frames[b]), int(t_in)))
            if n <= 0:
                continue
            total = self.count + n
            delta = moments[b, 0] - self.mean
            self.mean = self.mean + delta * (n / total)
            self.M2 = self.M2 + moments[b, 1] + delta * delta * (self.count * n / total)
            self.count = total
        return self

    def accumulate(self, feat, n_frames):
        """A mini-batch of UNNORMALISED source frames [t_in, B, D] on the device and its frame counts."""
        from . import ops
        return self.merge_moments(ops.feature_moments(feat, n_frames).cpu().numpy(), n_frames, feat.shape[0])

    def save(self, path):
        with open(path, "wb") as fh:        # (a file object: np.savez would append .npz to a bare path)
            np.savez(fh, count=np.float64(self.count), mean=self.mean, var=self.var,
                     **{k: np.asarray(self.description[k]) for k in _KEYS})

    @classmethod
    def load(cls, path, expect=None):
        """expect: describe(...) of the processor that reads the file; a file taken from other features raises ValueError."""
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("count", "mean", "var") + _KEYS if k not in z.files]
            if missing:
                raise ValueError("%s is no feature statistics file: it lacks %s" % (path, ", ".join(missing)))
            found = describe(str(z["signal_processing"]), int(z["n_mfcc"]), int(z["sample_rate"]), int(z["width"]))
            count, mean, var = float(z["count"]), np.array(z["mean"], np.float64), np.array(z["var"], np.float64)
        if expect is not None and dict(expect) != found:
            raise ValueError("%s holds statistics of %r, the processor computes %r" % (path, found, dict(expect)))
        if not count > 0:
            raise ValueError("%s holds statistics of no frame (count %r)" % (path, count))
        if mean.shape != (found["width"],) or var.shape != mean.shape:
            raise ValueError("%s: mean %s / var %s do not match the width %d" % (path, mean.shape, var.shape, found["width"]))
        stats = cls(found)
        stats.count, stats.mean, stats.M2 = count, mean, var * count
        return stats

    def table_numpy(self, norm_vars=True, var_floor=VAR_FLOOR):
        """float64 [2, D]: the means and the scales 1 / sqrt(max(var, var_floor)) (ones without variance normalisation)."""
        if not self.count > 0:
            raise ValueError("FeatureStats: no frame has been accumulated")
        if not var_floor > 0:
            raise ValueError("FeatureStats: var_floor must be positive, not %r" % (var_floor,))
        scale = 1.0 / np.sqrt(np.maximum(self.var, var_floor)) if norm_vars else np.ones_like(self.mean)
        return np.stack([self.mean, scale]).astype(np.float64)

    def table(self, norm_vars=True, var_floor=VAR_FLOOR, device="cuda"):
        """... on the device, as ops.feature_norm's global mode reads it."""
        import torch
        return torch.from_numpy(self.table_numpy(norm_vars, var_floor)).to(device)
