"""AudioProcessor drop-in (reference: /root/reference/util/audioprocessor.py:11-61).

Same constructor, attributes and return contract -- (features [T', D] truncated to
max_input_seq_length, UNtruncated frame count) -- but the features are computed by the
HIP front-end kernels (csrc/frontend.hip) instead of librosa/numpy.  `process_batch`
is the fast path: a whole mini-batch of signals -> one time-major device tensor.
"""
import collections

import numpy as np
import torch

from . import ops, segmenter
from .feature_norm import MODES, FeatureStats, describe_processor

FRAME_STRIDE = 0.01
FRAME_SIZE = 0.025
DEFAULT_LOAD_SR = 22050   # librosa.load default used by the reference's file path (:49)


# What AudioProcessor.segment returns: the recording on the device (pcm [1, n] at rate sr), the detector's hop, the spans
# [(start_sample, n_samples, start_frame, end_frame), ...] (segmenter.plan_spans) and the row's stats (floor, peak, threshold in dB)
Segments = collections.namedtuple("Segments", "pcm n sr hop spans stats")


class AudioProcessor(object):
    def __init__(self, max_input_seq_length, feature_type="mfcc", n_mfcc=20, device="cuda", load_sr=DEFAULT_LOAD_SR,
                 frame_stack=1, frame_skip=1, feature_norm="none", feature_norm_variance=True, feature_stats=None,
                 augment_bank=None):
        """feature_type: 'mfcc' (n_mfcc-dim, reference default 20) or 'fbank' (120-dim).  load_sr: the rate audio
        FILES are resampled to before feature extraction (config.ini `sample_rate`; the reference's librosa.load
        default, 22,050 Hz) -- set it to the corpus rate (16,000 for LibriSpeech) to skip resampling.
        frame_stack / frame_skip (1 .. 16; 1 / 1 is the reference's behaviour): low frame rate input -- `frame_stack` consecutive
        frames are concatenated into one MODEL frame and every `frame_skip`-th one is kept (ops.frame_stack).
        max_input_seq_length stays in SOURCE frames (audio is truncated as without the option); what the process_* calls return
        is out_seq_length = ceil(max_input_seq_length / frame_skip) model frames of feature_size = frame_stack * D values, and
        lengths of ceil(n / frame_skip).
        feature_norm ("none": the reference's behaviour | "utterance" | "global"): mean (and, with feature_norm_variance, variance)
        normalisation of the SOURCE frames on the GPU, between the front end and the frame stacking (ops.feature_norm) -- over the
        frames of the utterance that survive the truncation, or with the corpus statistics in feature_stats (a FeatureStats or the
        path of the file `stt.py --feature_stats` wrote; a file taken from other features is refused).
        augment_bank: the AugmentBank (impulse responses and noise clips at load_sr, on the device) that the `augment` draws of the
        process_* calls index; None: those calls take no draws."""
        self.max_input_seq_length = max_input_seq_length
        self.augment_bank = augment_bank
        self.load_sr = int(load_sr)
        self.feature_type = feature_type
        self.device = device
        if feature_type == "mfcc":
            self.feature_size = int(n_mfcc)
        elif feature_type == "fbank":
            self.feature_size = 120
        else:
            raise ValueError("{0} is not a valid extraction function, only fbank and mfcc are accepted."
                             .format(feature_type))
        self.n_mfcc = int(n_mfcc)
        self.frame_stack, self.frame_skip = int(frame_stack), int(frame_skip)
        for name, v in (("frame_stack", self.frame_stack), ("frame_skip", self.frame_skip)):
            if not 1 <= v <= 16:
                raise ValueError("%s must be in 1 .. 16, not %r" % (name, v))
        self.source_feature_size = self.feature_size            # what the front end emits per 10 ms frame
        self.feature_size *= self.frame_stack                   # ... and the model reads per model frame
        if self.feature_size > 4096:
            raise ValueError("frame_stack * feature width = %d exceeds 4096" % self.feature_size)
        self.out_seq_length = -(-int(max_input_seq_length) // self.frame_skip)
        if feature_norm not in MODES:
            raise ValueError("feature_norm must be one of %s, not %r" % (", ".join(MODES), feature_norm))
        self.feature_norm, self.feature_norm_variance = feature_norm, bool(feature_norm_variance)
        self.feature_stats, self._norm_tables = None, {}
        if feature_norm == "global":
            if feature_stats is None:
                raise ValueError("feature_norm 'global' needs feature_stats (the file `stt.py --feature_stats` writes)")
            expect = describe_processor(self)
            if not isinstance(feature_stats, FeatureStats):
                feature_stats = FeatureStats.load(feature_stats, expect)
            elif feature_stats.description != expect:
                raise ValueError("feature_stats holds statistics of %r, the processor computes %r" % (feature_stats.description, expect))
            self.feature_stats = feature_stats
        # samples between the starts of two frames (csrc/frontend.hip: 10 ms, rounded half to even, in both modes): frame t of a
        # file starts t * hop_samples / load_sr seconds in
        self.hop_samples = int(round(self.load_sr * 0.01))
        # ... and between the starts of two MODEL frames: model frame j starts with source frame j * frame_skip
        self.frame_hop_samples = self.hop_samples * self.frame_skip

    @staticmethod
    def get_mfcc_length_from_duration(duration):
        """Estimate only (reference :30-39)."""
        return int(duration // FRAME_STRIDE) - 1

    # ---- reference surface ----------------------------------------------------
    def process_audio_file(self, file_name):
        feat, lengths = self.process_files([file_name])
        n = min(lengths[0], self.out_seq_length)
        return feat[:n, 0, :].cpu().numpy(), lengths[0]

    def process_signal(self, sig, sr):
        feat, lengths = self.process_batch([np.asarray(sig, dtype=np.float32)], sr)
        n = min(lengths[0], self.out_seq_length)
        return feat[:n, 0, :].cpu().numpy(), lengths[0]

    # ---- batched device path ----------------------------------------------------
    def stage(self, signals, rows=None):
        """Host half of an upload, safe to run on a producer thread: the signals packed into one [rows, width] float32 block in
        PINNED memory (a small pool of blocks, each reused once the copy that read it has completed), so that the device half is
        one asynchronous DMA instead of a pageable copy the host thread has to sit through (20 MB: 5 ms)."""
        n = [len(s) for s in signals]
        shape = (rows or len(signals), max(max(n) if n else 0, 1))
        block = _PINNED.get(shape) if (self.device != "cpu" and torch.cuda.is_available()) else _Staged(torch.zeros(shape))
        host = block.tensor.numpy()
        for i, s in enumerate(signals):
            host[i, :len(s)] = s
            host[i, len(s):] = 0.0
        host[len(signals):] = 0.0
        return block, n

    def _upload_staged(self, block):
        dev = block.tensor.to(self.device, non_blocking=True)
        block.mark_in_flight()
        return dev

    def _upload(self, signals, rows=None):
        block, n = self.stage(signals, rows)
        return self._upload_staged(block), n

    def _source_t_max(self, t_max):
        """t_max counts the frames a process_* call RETURNS (model frames); the front end runs every source frame their windows
        reach, never more than max_input_seq_length (so at most out_seq_length model frames come back)."""
        if t_max is None:
            return self.max_input_seq_length
        if self.frame_stack == 1 and self.frame_skip == 1:
            return int(t_max)
        return max(1, min((int(t_max) - 1) * self.frame_skip + self.frame_stack, self.max_input_seq_length))

    def _normalised(self, feat, lengths):
        """Feature normalisation of the front end's [t_in, B, D] tensor, in place; "none": nothing is launched."""
        if self.feature_norm == "none":
            return
        table = None
        if self.feature_norm == "global":
            table = self._norm_tables.get(feat.device)
            if table is None:
                table = self._norm_tables[feat.device] = self.feature_stats.table(self.feature_norm_variance, device=feat.device)
        ops.feature_norm(feat, lengths, self.feature_norm, self.feature_norm_variance, table=table)

    def _stacked(self, feat, lengths, t_max):
        """Feature normalisation, then low frame rate input, behind the front end; with both off the front end's own tensor, no
        copy and no launch."""
        self._normalised(feat, lengths)
        if self.frame_stack == 1 and self.frame_skip == 1:
            return feat, lengths
        out, n_out = ops.frame_stack(feat, lengths, self.frame_stack, self.frame_skip)
        return (out if t_max is None or out.shape[0] <= t_max else out[:int(t_max)]), n_out

    @staticmethod
    def _speeds(speed_permille, rows):
        """Per-row speed factors (permille, 500 .. 2000) of a process_* call, checked; None: no speed change."""
        if speed_permille is None:
            return None
        speeds = [int(v) for v in speed_permille]
        if len(speeds) != rows:
            raise ValueError("speed_permille: %d factors for %d rows" % (len(speeds), rows))
        for v in speeds:
            if not 500 <= v <= 2000:
                raise ValueError("speed_permille: %d outside 500 .. 2000" % v)
        return speeds

    @staticmethod
    def _resampled(pcm, n, speeds, rate_in, rate_out):
        """One ops.resample_rows call for a group of rows at one source rate: rate conversion and speed change together.  A group
        whose rows all have ratio exactly 1 (rate_out * 1000 == rate_in * speed) makes no call."""
        rows = len(n)
        speeds = list(speeds) + [1000] * (pcm.shape[0] - rows)       # (padding rows are empty)
        n = list(n) + [0] * (pcm.shape[0] - rows)
        if all(int(rate_out) * 1000 == int(rate_in) * v for v in speeds[:rows]):
            return pcm, n[:rows]
        out, n_out = ops.resample_rows(pcm, n, speeds, rate_in, rate_out)
        return out, n_out[:rows]

    def _augmented(self, pcm, n, augment):
        """Reverberation, then additive noise, on the rows of one call (ops.reverb_rows, ops.row_sumsq, ops.noise_mix_rows):
        augment holds (rir_index, noise_index, noise_offset, snr_decidb) per row, an index of -1 = not applied; rows past the list
        are padding.  None, or no row with an index: nothing is launched and pcm is returned as it came."""
        if augment is None:
            return pcm
        bank, rows = self.augment_bank, pcm.shape[0]
        if bank is None:
            raise ValueError("augment draws without an augment_bank")
        if len(augment) > rows:
            raise ValueError("augment: %d draws for %d rows" % (len(augment), rows))
        draws = [tuple(int(v) for v in d) for d in augment] + [(-1, -1, 0, 0)] * (rows - len(augment))
        n = list(n) + [0] * (rows - len(n))
        rir, noise = [d[0] for d in draws], [d[1] for d in draws]
        if any(r >= 0 for r in rir):
            if bank.rir_bank is None:
                raise ValueError("augment: a draw names an impulse response, the bank holds none")
            pcm = ops.reverb_rows(pcm, n, bank.rir_bank, bank.rir_taps, bank.rir_delay, rir)
        if any(m >= 0 for m in noise):
            if bank.noise_bank is None:
                raise ValueError("augment: a draw names a noise clip, the bank holds none")
            energy = ops.row_sumsq(pcm, n)
            pcm = ops.noise_mix_rows(pcm, n, energy, bank.noise_bank, bank.noise_len, bank.noise_sumsq, noise, [d[2] for d in draws],
                                     [d[3] for d in draws], out=pcm)
        return pcm

    def _features(self, pcm, n, sr, t_out, augment):
        """The tail of both process_* calls: augmentation, the front end at rate sr, normalisation and stacking to t_out model frames."""
        pcm = self._augmented(pcm, n, augment)
        # (an empty row has no frames; the front end wants > n_fft/2 samples for real ones)
        feat, lengths = ops.frontend(pcm, n, int(sr), self.feature_type, int(self._source_t_max(t_out)), self.n_mfcc)
        return self._stacked(feat, lengths, t_out)

    def process_batch(self, signals, sr, t_max=None, staged=None, speed_permille=None, augment=None):
        """signals: list of 1-D float arrays, all at sample rate `sr`.  Returns (feat [t_max, B, feature_size] device
        float32, zero past each utterance; list of UNtruncated frame counts) -- model frames under low frame rate input,
        t_max defaulting to out_seq_length.  staged: (block, n) from stage().  speed_permille: a speed factor per signal (speed
        perturbation, ops.resample_rows: a row played f times faster has 1 / f of its samples); None or all 1000: nothing is launched.
        augment: (rir_index, noise_index, noise_offset, snr_decidb) per signal, indices into augment_bank (whose audio is taken to be at
        `sr`): reverberation, then noise, behind the speed change; None or no index >= 0: nothing is launched."""
        if staged is not None:
            pcm, n = self._upload_staged(staged[0]), staged[1]
        else:
            pcm, n = self._upload(signals)
        speeds = self._speeds(speed_permille, len(n))
        if speeds is not None:
            pcm, n = self._resampled(pcm, n, speeds, int(sr), int(sr))
        return self._features(pcm, n, sr, t_max, augment)

    def stage_files(self, decoded, speed_permille=None):
        """stage() for decoded files, grouped by source rate as process_files uploads them: [(sr, idx, block, n)].  speed_permille
        (a factor per file, handed to process_files with the result) is checked here, on the producer's thread."""
        self._speeds(speed_permille, len(decoded))
        by_rate = {}
        for i, (_, sr) in enumerate(decoded):
            by_rate.setdefault(int(sr), []).append(i)
        return [(sr, idx) + self.stage([decoded[i][0] for i in idx]) for sr, idx in by_rate.items()]

    def process_files(self, file_names, t_max=None, rows=None, decoded=None, staged=None, speed_permille=None, augment=None):
        """What the reference's dataset map does per file (process_audio_file: librosa.load at 22,050 Hz,
        then the extractor, util/audioprocessor.py:41-61), for a whole mini-batch: files are decoded natively
        on host threads (or passed in as `decoded` [(signal, sr), ...]), uploaded once, resampled to
        22,050 Hz on the GPU per source rate and handed to the front-end kernels without leaving HBM.
        `rows` > len(files) pads the batch with empty utterances (length 0).  Model frames as process_batch.
        speed_permille: a speed factor per file (speed perturbation, None: 1000 each); per source rate ONE ops.resample_rows call does
        the rate conversion and the speed change together, and a group whose rows all have ratio 1 makes no call.  A row made longer than
        max_input_seq_length is truncated by the front end like any over-long file.
        augment: (rir_index, noise_index, noise_offset, snr_decidb) per file, indices into augment_bank: reverberation, then noise,
        ONCE on the assembled [B, width] tensor at load_sr, behind the per-rate groups; None or no index >= 0: nothing is launched."""
        if decoded is None:
            decoded = decode_files(file_names)
        B = rows or len(decoded)
        speeds = self._speeds(speed_permille, len(decoded)) or [1000] * len(decoded)
        if staged is None:
            staged = self.stage_files(decoded)
        parts, lengths = [], [0] * B
        for sr, idx, block, n in staged:
            pcm = self._upload_staged(block)
            pcm, n = self._resampled(pcm, n, [speeds[i] for i in idx], sr, self.load_sr)
            parts.append((idx, pcm, n))
        width = max(max(p[1].shape[1] for p in parts), 1) if parts else 1
        if len(parts) == 1 and len(parts[0][0]) == B:
            pcm, n = parts[0][1], parts[0][2]
        else:
            pcm = torch.zeros(B, width, device=self.device)
            n = [0] * B
            for idx, part, lens in parts:
                ii = torch.as_tensor(idx, device=self.device)
                pcm[ii, :part.shape[1]] = part
                for j, i in enumerate(idx):
                    n[i] = lens[j]
        return self._features(pcm, n, self.load_sr, t_max, augment)

    # ---- long recordings ----------------------------------------------------------
    def segment(self, signal, sr, floor_percentile=10, margin_db=10.0, range_db=50.0, min_db=-70.0, min_speech_ms=50.0,
                hangover_ms=200.0, pad_ms=100.0):
        """Where to cut a recording longer than the model's input: signal (1-D floats at rate sr) is uploaded once, the voice-activity
        kernels run at the file's own rate with hop = round-half-even(0.01 sr) (ops.vad_energy, ops.vad_flags; the milliseconds
        become 10 ms frames), and the cut planner (segmenter.plan_spans) turns the flags into spans of at most the budget the
        resampler and the front end leave of max_input_seq_length.  Returns a Segments record; process_segments takes it from there."""
        sig = np.ascontiguousarray(signal, dtype=np.float32).ravel()
        sr, n = int(sr), len(sig)
        hop = int(round(sr * 0.01))
        frames = lambda ms: int(round(float(ms) / 10.0))
        pcm, _ = self._upload([sig])
        if n == 0:
            return Segments(pcm, 0, sr, hop, [], (-120.0, -120.0, -120.0))
        F = ops.vad_num_frames(n, hop)
        energy = ops.vad_energy(pcm, [n], hop)
        speech, stats = ops.vad_flags(energy, [F], floor_percentile, margin_db, range_db, min_db, max(1, frames(min_speech_ms)),
                                      frames(hangover_ms))
        budget = segmenter.frame_budget(sr, hop, self.load_sr, self.feature_type, self.max_input_seq_length)
        shortest = segmenter.min_span_samples(sr, self.load_sr, self.feature_type, self.n_mfcc)
        spans = segmenter.plan_spans(speech[0, :F].cpu().numpy(), energy[0, :F].cpu().numpy(), n, hop, budget, frames(pad_ms), shortest)
        return Segments(pcm, n, sr, hop, spans, tuple(float(v) for v in stats[0].cpu().numpy()))

    def process_segments(self, pcm_device, n, sr, spans, rows=None):
        """The features of spans of ONE long device row pcm_device [1, >= n] at rate sr, as process_files returns them for as many
        files: one ops.gather_spans call builds the padded [rows, width] block, then the per-row resampler to load_sr and the front
        end as for any mini-batch.  spans: (start_sample, n_samples, ...) tuples; `rows` > len(spans) pads with empty rows.
        feature_norm : utterance normalises per span (a span is the utterance the model sees); no speed, noise or reverberation
        draw is ever applied here."""
        S = len(spans)
        B = rows or S
        counts = [int(sp[1]) for sp in spans]
        block = torch.empty(B, max(counts + [1]), device=pcm_device.device, dtype=torch.float32)
        ops.gather_spans(pcm_device, [int(n)], [0] * S, [int(sp[0]) for sp in spans], counts, block.shape[1], out=block[:S])
        block[S:] = 0.0
        pcm, lens = self._resampled(block, counts, [1000] * S, int(sr), self.load_sr)
        return self._features(pcm, list(lens) + [0] * (B - S), self.load_sr, None, None)


AUDIO_SUFFIXES = (".wav", ".flac", ".sph")


class AugmentBank(object):
    """Room impulse responses and noise clips for the waveform augmentation (ops.reverb_rows / ops.noise_mix_rows), resident on the
    device, built once per dataset.
    rirs / noises: lists of 1-D float arrays at the processor's load_sr (from_dirs decodes and resamples files).  An impulse
    response is cut to max_taps samples, scaled IN FLOAT64 to unit energy (one of zero energy is refused) and given delay =
    argmax |h|, the direct path, so that reverberant speech stays aligned with its labels; the responses are stored as ONE
    zero-padded tensor rir_bank [R, taps_max] with rir_taps / rir_delay (python ints).  A noise clip is cut to max_noise_samples;
    the clips are ONE tensor noise_bank [M, m_max] with noise_len (python ints) and noise_sumsq (float64 [M] on the device,
    ops.row_sumsq).  A part with no arrays is None.  The two tensors together may not exceed bank_mb MiB (`augment_bank_mb`)."""

    def __init__(self, rirs=(), noises=(), device="cuda", max_taps=8192, max_noise_samples=None, bank_mb=256):
        if not 1 <= int(max_taps) <= 8192:
            raise ValueError("reverb_max_taps must be in 1 .. 8192, not %r" % (max_taps,))
        rirs = [np.asarray(h, np.float64).ravel()[:int(max_taps)] for h in rirs]
        noises = [np.asarray(v, np.float32).ravel()[:max_noise_samples] for v in noises]
        for i, h in enumerate(rirs):
            if h.size == 0 or not np.isfinite(h).all() or not np.sum(h * h) > 0.0:
                raise ValueError("impulse response %d is empty, not finite or has no energy" % i)
        for i, v in enumerate(noises):
            if v.size == 0 or not np.isfinite(v).all():
                raise ValueError("noise clip %d is empty or not finite" % i)
        taps_max, m_max = max([h.size for h in rirs] + [0]), max([v.size for v in noises] + [0])
        nbytes = 4 * (len(rirs) * taps_max + len(noises) * m_max)
        if nbytes > int(bank_mb) << 20:
            raise ValueError("the augmentation bank needs %.1f MiB, augment_bank_mb allows %d: raise augment_bank_mb, lower "
                             "noise_max_seconds or use fewer files" % (nbytes / 2.0 ** 20, int(bank_mb)))
        self.device, self.nbytes = device, nbytes
        self.rir_bank, self.rir_taps, self.rir_delay = None, [], []
        self.noise_bank, self.noise_len, self.noise_sumsq = None, [], None
        if rirs:
            host = np.zeros((len(rirs), taps_max), np.float32)
            for i, h in enumerate(rirs):
                host[i, :h.size] = h / np.sqrt(np.sum(h * h))
                self.rir_taps.append(int(h.size))
                self.rir_delay.append(int(np.argmax(np.abs(h))))
            self.rir_bank = torch.from_numpy(host).to(device)
        if noises:
            host = np.zeros((len(noises), m_max), np.float32)
            for i, v in enumerate(noises):
                host[i, :v.size] = v
                self.noise_len.append(int(v.size))
            self.noise_bank = torch.from_numpy(host).to(device)
            self.noise_sumsq = ops.row_sumsq(self.noise_bank, self.noise_len)

    @staticmethod
    def list_files(directory):
        """The audio files under a directory (recursively), sorted: the order the draws index."""
        import os
        found = []
        for root, _, names in os.walk(directory):
            found += [os.path.join(root, f) for f in names if f.lower().endswith(AUDIO_SUFFIXES)]
        return sorted(found)

    @classmethod
    def from_dirs(cls, load_sr, noise_dir="", reverb_dir="", device="cuda", max_taps=8192, noise_max_seconds=30.0, bank_mb=256):
        """The bank of two directories of WAVE / FLAC / SPHERE files (either may be empty: that part is off), decoded by the
        native decoders and brought to load_sr by ops.resample."""
        def load(directory, what, limit):
            if not directory:
                return []
            files = cls.list_files(directory)
            if not files:
                raise ValueError("%s %r holds no %s file" % (what, directory, " / ".join(AUDIO_SUFFIXES)))
            out = []
            for sig, sr in decode_files(files):
                sig = sig[:max(1, int(np.ceil(limit * sr / float(load_sr))))]      # (what survives the cut below, at the source rate)
                if sr != load_sr and sig.size:
                    pcm = torch.from_numpy(np.ascontiguousarray(sig[None, :])).to(device)
                    res, n = ops.resample(pcm, [len(sig)], sr, load_sr)
                    sig = res[0, :n[0]].cpu().numpy()
                out.append(sig)
            return out
        max_noise = max(1, int(float(noise_max_seconds) * load_sr))
        return cls(load(reverb_dir, "reverb_dir", int(max_taps)), load(noise_dir, "noise_dir", max_noise), device=device,
                   max_taps=max_taps, max_noise_samples=max_noise, bank_mb=bank_mb)


class _Staged(object):
    """A [rows, width] host block handed out by the staging pool.  Claimed from get() until mark_in_flight() records the event
    behind the copy that reads it; free again once that event has completed."""

    def __init__(self, tensor, flat=None):
        self.tensor, self.flat = tensor, flat
        self.event, self.claimed = None, True

    def mark_in_flight(self):
        if self.tensor.is_pinned():
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream())
        self.claimed = False

    def free(self):
        return not self.claimed and (self.event is None or self.event.query())


class _PinnedPool(object):
    """Pinned staging blocks, reused: a hipHostMalloc per mini-batch would cost more than the copy it speeds up."""

    def __init__(self, limit=12):
        import threading
        self._lock = threading.Lock()
        self._blocks, self._limit = [], limit

    def get(self, shape):
        need = shape[0] * shape[1]
        with self._lock:
            for i, blk in enumerate(self._blocks):
                if blk.flat.numel() >= need and blk.free():
                    self._blocks[i] = _Staged(blk.flat[:need].view(shape), blk.flat)
                    return self._blocks[i]
            if len(self._blocks) >= self._limit:      # make room: forget a free block (too small, or just the oldest)
                for i, blk in enumerate(self._blocks):
                    if blk.free():
                        del self._blocks[i]
                        break
        flat = torch.empty(need, dtype=torch.float32).pin_memory()
        blk = _Staged(flat.view(shape), flat)
        with self._lock:
            if len(self._blocks) < self._limit:
                self._blocks.append(blk)
        return blk


_PINNED = _PinnedPool()
_POOL = None


def decode_files(file_names):
    """[(mono float32 signal, sample_rate), ...] -- native decoders (WAVE / FLAC / NIST SPHERE) on a
    thread pool; the C call releases the GIL."""
    global _POOL
    if len(file_names) <= 1:
        return [ops.audio_decode(f) for f in file_names]
    if _POOL is None:
        import os
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1))
    return list(_POOL.map(ops.audio_decode, file_names))


def load_audio(file_name, target_sr=DEFAULT_LOAD_SR, device="cuda"):
    """librosa.load(file, sr=target_sr) equivalent: mono float32 numpy at target_sr (native decode, GPU
    resampler with resampy kaiser_best semantics; not bit-compatible with any particular librosa release)."""
    sig, sr = ops.audio_decode(file_name)
    if sr != target_sr:
        pcm = torch.from_numpy(np.ascontiguousarray(sig[None, :])).to(device)
        out, n = ops.resample(pcm, [len(sig)], sr, target_sr)
        sig = out[0, :n[0]].cpu().numpy()
    return sig, target_sr
