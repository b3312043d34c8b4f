"""The training input pipeline: AcousticDataset (what AcousticModel.build_dataset returns), its length-bucketed ordering and the
iterator the model reads it through -- the part of the reference's models/AcousticModel.py that tf.data does (:820-827)."""
import collections
import copy

import numpy as np
import torch

from . import dataparallel
from . import hyperparams
from . import labels as _labels
from . import ops
from .audioprocessor import AudioProcessor, decode_files


class OutOfRangeError(Exception):
    """Stands in for tf.errors.OutOfRangeError (iterator exhausted)."""


class _Upload(collections.namedtuple("_Upload", "staged rate blocks")):
    """The staged upload of a prepared mini-batch.  rate is not None: in-memory signals at that one rate, `staged` is what
    AudioProcessor.process_batch takes (one block); rate None: `staged` is what process_files takes (a group per source rate).
    blocks: the pinned blocks either way."""
    __slots__ = ()

    def release(self):
        """This mini-batch will never be uploaded (the iterator was reset): its pinned blocks return to the pool."""
        for blk in self.blocks:
            blk.claimed = False


# Host half of one mini-batch, from the producer to the consumer: the items, (kind, payload) per item (signal | decoded | cached),
# the label matrix, the _Upload (None with a cached row), the items' speed factors and augmentation draws (None: option off)
_Prepared = collections.namedtuple("_Prepared", "chunk parts dense upload speeds draws")


class AcousticDataset(object):
    """What build_dataset returns: items [audio, label, (length)] where `audio` is a file
    path or an in-memory (signal, sample_rate) pair, batched to [T_max, B, D] device tensors
    with the reference's padding rules (:825-827, :144-159).

    The reference maps files through two py_func threads and prefetches 30 items (:820-822), and recomputes
    every feature every epoch.  Here a producer thread decodes the NEXT `prefetch` mini-batches (native
    decoders on a thread pool, GIL released) while the GPU trains on the current one, and -- optionally --
    the features of file items are kept in host memory after their first use (`feature_cache_mb` > 0), so
    later epochs skip decode, resampling and the front end altogether.

    frame_stack / frame_skip: low frame rate input (AudioProcessor).  max_input_seq_length stays in SOURCE frames; the batches,
    their lengths, T and the feature cache are in MODEL frames (T = audio.out_seq_length rows of audio.feature_size values).
    feature_norm / feature_norm_variance / feature_stats: feature normalisation (AudioProcessor); the batches and the feature
    cache hold normalised features.
    speed_perturb: None (off: nothing is launched), or (factors_permille, seed) -- speed perturbation of the waveform on the GPU
    (ops.resample_rows).  The factor of an item is ops.speed_perturb_draw(seed64, (epoch_serial << 32) | position in self.items,
    factors) with seed64 = (seed + data-parallel rank) << 32; epoch_serial is a counter shared with the with_items siblings that
    advances once per batches() pass, so a re-shuffled epoch draws afresh and a run is reproducible.  Durations used for bucketing
    stay the unperturbed ones; a row made longer than max_input_seq_length is truncated like any over-long file.  Cached features
    would freeze the draw: feature_cache_mb > 0 beside it is refused.
    augment: None (off: nothing is launched, nothing is allocated), or (bank, reverb_permille, noise_permille, (snr_lo, snr_hi) in
    tenths of a dB, seed) -- reverberation and additive noise on the waveform on the GPU, behind the speed change
    (AudioProcessor._augmented); bank is an audioprocessor.AugmentBank at sample_rate, shared with the with_items siblings.  The draw
    of an item is ops.augment_draw with the seed64 / epoch_serial / position scheme of the speed draw (and its rank handling), on
    the producer thread.  feature_cache_mb > 0 beside it is refused for the same reason."""

    def __init__(self, input_set, batch_size, max_input_seq_length, max_target_seq_length,
                 signal_processing, char_map, n_mfcc=20, prefetch=2, feature_cache_mb=0,
                 sample_rate=22050, frame_stack=1, frame_skip=1, feature_norm="none", feature_norm_variance=True,
                 feature_stats=None, speed_perturb=None, augment=None, device="cuda"):
        self.items = [(it[0], it[1]) for it in input_set]
        self.batch_size = batch_size
        self.U = max_target_seq_length
        self.char_map = char_map
        self._augment = self._augment_option(augment, feature_cache_mb)
        self.audio = AudioProcessor(max_input_seq_length, signal_processing, n_mfcc=n_mfcc, device=device,
                                    load_sr=sample_rate, frame_stack=frame_stack, frame_skip=frame_skip,
                                    feature_norm=feature_norm, feature_norm_variance=feature_norm_variance,
                                    feature_stats=feature_stats, augment_bank=None if self._augment is None else self._augment[0])
        self.T = self.audio.out_seq_length
        self.prefetch = int(prefetch)
        # with_items siblings are shallow copies: they share the processor, the cache and the two one-element cells below
        self._cache = {} if feature_cache_mb > 0 else None
        self._room = [int(feature_cache_mb) << 20]          # bytes the feature cache may still take
        self._speed = self._speed_option(speed_perturb, feature_cache_mb)
        self._epoch = [0]                                   # the draws' epoch_serial: batches() passes so far, of all siblings
        # the data-parallel rank, resolved HERE on the caller's thread: the draws run on the decode-ahead thread
        self._rank = dataparallel.current().rank if (self._speed is not None or self._augment is not None) else 0

    @staticmethod
    def _speed_option(speed_perturb, feature_cache_mb):
        if speed_perturb is None:
            return None
        factors, seed = speed_perturb
        factors = tuple(hyperparams.check_speed_factors("speed_perturb", [int(f) for f in factors]))
        if factors == (1000,):
            return None
        if feature_cache_mb > 0:
            raise ValueError("speed_perturb with feature_cache_mb > 0: cached features would freeze the draw; set feature_cache_mb : 0")
        return factors, int(seed)

    @staticmethod
    def _augment_option(augment, feature_cache_mb):
        if augment is None:
            return None
        bank, reverb_permille, noise_permille, snr, seed = augment
        reverb_permille = hyperparams.check_range("augment: reverb_permille", int(reverb_permille), 0, 1000)
        noise_permille = hyperparams.check_range("augment: noise_permille", int(noise_permille), 0, 1000)
        snr = hyperparams.check_snr_decidb("augment", (int(snr[0]), int(snr[1])))
        if bank is None or bank.rir_bank is None:
            reverb_permille = 0
        if bank is None or bank.noise_bank is None:
            noise_permille = 0
        if reverb_permille == 0 and noise_permille == 0:
            return None
        if feature_cache_mb > 0:
            raise ValueError("noise / reverberation augmentation with feature_cache_mb > 0: cached features would freeze the draw; "
                             "set feature_cache_mb : 0")
        return bank, reverb_permille, noise_permille, snr, int(seed)

    def _draw_keys(self, seed, epoch_serial, start, count):
        """What both draws are keyed by: (seed64 of this dataset, [the index of item `pos` in pass epoch_serial, for the items
        start .. start + count])."""
        stop = len(self.items) if count is None else min(start + count, len(self.items))
        return ((seed + self._rank) << 32) & 0xFFFFFFFFFFFFFFFF, [(int(epoch_serial) << 32) | pos for pos in range(start, stop)]

    def speed_draws(self, epoch_serial, start=0, count=None):
        """The speed factors (permille) of items start .. start + count of pass `epoch_serial`; None when the option is off."""
        if self._speed is None:
            return None
        factors, seed = self._speed
        seed64, keys = self._draw_keys(seed, epoch_serial, start, count)
        return [ops.speed_perturb_draw(seed64, key, factors) for key in keys]

    def augment_draws(self, epoch_serial, start=0, count=None):
        """(rir_index, noise_index, noise_offset, snr_decidb) of items start .. start + count of pass `epoch_serial`; None when the
        option is off."""
        if self._augment is None:
            return None
        bank, reverb_permille, noise_permille, snr, seed = self._augment
        seed64, keys = self._draw_keys(seed, epoch_serial, start, count)
        return [ops.augment_draw(seed64, key, reverb_permille, len(bank.rir_taps), noise_permille, bank.noise_len, snr) for key in keys]

    def with_items(self, input_set):
        """The same dataset over a re-ordered / re-shuffled item list (the reference builds a fresh tf.data pipeline at every
        epoch, stt.py:198-207): a shallow copy, so the processor, the feature cache and its room, the epoch counter, the rank and
        the augmentation bank are the parent's own objects."""
        other = copy.copy(self)
        other.items = [(it[0], it[1]) for it in input_set]
        return other

    # ---- producer side (host only) -------------------------------------------------
    def _chunks(self):
        B = self.batch_size
        for start in range(0, len(self.items), B):
            yield start, self.items[start:start + B]

    def _prepare(self, start, chunk, epoch_serial):
        """Host half of one mini-batch, the items start .. of pass epoch_serial: their draws (speed, noise, reverberation), cached
        features or decoded waveforms per item."""
        speeds = self.speed_draws(epoch_serial, start, len(chunk))
        draws = self.augment_draws(epoch_serial, start, len(chunk))
        cache = self._cache
        need = [a for a, _ in chunk if isinstance(a, str) and (cache is None or a not in cache)]
        from_disk = dict(zip(need, decode_files(need)))
        parts = []
        for a, _ in chunk:
            if not isinstance(a, str):
                parts.append(("signal", (np.asarray(a[0], np.float32), int(a[1]))))
            elif a in from_disk:
                parts.append(("decoded", from_disk[a]))
            else:
                parts.append(("cached", cache[a]))
        # everything the consumer would otherwise do on the training thread between two kernel launches: the label codec
        # (0.12 ms per utterance) and the packing of the waveforms into one pinned block for an asynchronous upload
        B = self.batch_size
        dense = np.zeros((B, self.U), np.int32)
        for i, (_, text) in enumerate(chunk):
            ids = _labels.get_str_labels(self.char_map, text)[:self.U]
            dense[i, :len(ids)] = ids
        kinds = {k for k, _ in parts}
        rates = {sr for _, (_, sr) in parts} if kinds == {"signal"} else ()
        upload = None
        if len(rates) == 1:
            block, n = self.audio.stage([sig for _, (sig, _) in parts] + [np.zeros(0, np.float32)] * (B - len(parts)))
            upload = _Upload((block, n), rates.pop(), [block])
        elif "cached" not in kinds:
            groups = self.audio.stage_files([p for _, p in parts], speeds)
            upload = _Upload(groups, None, [block for _, _, block, _ in groups])
        return _Prepared(chunk, parts, dense, upload, speeds, draws)

    def _prepared(self, epoch_serial=0):
        if self.prefetch <= 0:
            for start, chunk in self._chunks():
                yield self._prepare(start, chunk, epoch_serial)
            return
        import queue
        import threading
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()

        def produce():
            try:
                for start, chunk in self._chunks():
                    if stop.is_set():
                        return
                    q.put(("ok", self._prepare(start, chunk, epoch_serial)))
                q.put(("end", None))
            except BaseException as exc:            # surfaced in the consumer
                q.put(("error", exc))

        th = threading.Thread(target=produce, name="amdspeech-decode", daemon=True)
        th.start()
        try:
            while True:
                tag, payload = q.get()
                if tag == "end":
                    return
                if tag == "error":
                    raise payload
                yield payload
        finally:
            stop.set()
            while th.is_alive() or not q.empty():   # unblock a producer waiting on a full queue; hand its staging blocks back
                try:
                    tag, payload = q.get_nowait()
                    if tag == "ok" and payload.upload is not None:
                        payload.upload.release()
                except queue.Empty:
                    th.join(0.01)

    # ---- consumer side (device) -----------------------------------------------------
    def batches(self):
        B, T = self.batch_size, self.T
        epoch_serial = self._epoch[0]              # this pass's draws (speed, noise, reverberation); the next pass draws afresh
        self._epoch[0] += 1
        for p in self._prepared(epoch_serial):
            extra = {} if p.draws is None else {"augment": p.draws}      # (off: the call is the one it was before the option existed)
            if p.upload is None:
                feat, lengths = self._assemble(p.parts)
            elif p.upload.rate is not None:
                # in-memory signals at one rate: the process_signal convention (no resampling)
                feat, lengths = self.audio.process_batch(None, p.upload.rate, t_max=T, staged=p.upload.staged,
                                                         speed_permille=None if p.speeds is None else p.speeds + [1000] * (B - len(p.speeds)),
                                                         **extra)
            else:
                # files: librosa.load semantics (22,050 Hz); a short final batch is padded with empty rows
                feat, lengths = self.audio.process_files(None, t_max=T, rows=B, decoded=[d for _, d in p.parts], staged=p.upload.staged,
                                                         speed_permille=p.speeds, **extra)
            if self._cache is not None:
                self._remember(p.chunk, p.parts, feat, lengths)
            yield feat, np.asarray(lengths, np.int32), p.dense

    def _assemble(self, parts):
        """A mini-batch with cached rows: fresh rows go through the device path, cached rows are copied in."""
        B, T, D = self.batch_size, self.T, self.audio.feature_size
        fresh = [i for i, (k, _) in enumerate(parts) if k != "cached"]
        lengths = [0] * B
        host = np.zeros((T, B, D), np.float32)
        for i, (k, p) in enumerate(parts):
            if k == "cached":
                f, n = p
                host[:f.shape[0], i] = f
                lengths[i] = n
        feat = torch.from_numpy(host).to(self.audio.device)
        if fresh:
            sub, sub_len = self.audio.process_files(None, t_max=T, decoded=[parts[i][1] for i in fresh])
            feat[:, torch.as_tensor(fresh, device=feat.device)] = sub
            for j, i in enumerate(fresh):
                lengths[i] = sub_len[j]
        return feat, lengths

    def _remember(self, chunk, parts, feat, lengths):
        rows = [i for i, (k, _) in enumerate(parts) if k == "decoded"]
        if not rows or self._room[0] <= 0:
            return
        host = feat[:, torch.as_tensor(rows, device=feat.device)].cpu().numpy()
        for j, i in enumerate(rows):
            n = min(int(lengths[i]), self.T)
            f = host[:n, j].copy()
            if f.nbytes > self._room[0]:
                self._room[0] = 0
                return
            self._room[0] -= f.nbytes
            self._cache[chunk[i][0]] = (f, int(lengths[i]))


def bucketed_order(items, batch_size, rng=None):
    """Length-bucketed batching: items [audio, label, duration] sorted by duration, cut into
    mini-batches, and the mini-batches -- not the items -- shuffled.  Every batch then holds utterances of
    similar length, so the recurrence (which stops at the batch's longest utterance) wastes no frames."""
    import random
    ordered = sorted(items, key=lambda it: (it[2] if len(it) > 2 and it[2] is not None else 0.0))
    groups = [ordered[i:i + batch_size] for i in range(0, len(ordered), batch_size)]
    tail = [groups.pop()] if groups and len(groups[-1]) < batch_size else []     # a short group stays last,
    (rng or random).shuffle(groups)                                              # or every later batch straddles
    return [it for g in groups + tail for it in g]


class DatasetIterator(object):
    """Iterator over a dataset's mini-batches.  `prefetch()` prepares the NEXT mini-batch ahead of its use: the
    host part comes from the dataset's decode-ahead thread, the device part (upload, resampling, front-end
    kernels) is enqueued on a side stream, so it runs under the tail of the training step in flight (the
    reference's tf.data pipeline overlaps feature extraction with training the same way, :820-822)."""

    _UNSET = object()

    def __init__(self, dataset):
        self._dataset = dataset
        self._gen = None
        self._ahead = self._UNSET
        self._side = None
        self.initializer = self._reset           # an "op": what Session.run calls

    def _reset(self):
        self._gen = self._dataset.batches()
        self._ahead = self._UNSET

    @property
    def dataset(self):
        return self._dataset

    def make_initializer(self, dataset):
        def _swap():
            self._dataset = dataset
            self._reset()
        return _swap

    def prefetch(self, after=None):
        """Prepare the next mini-batch ahead of its use.  after: an event the device half must wait for.
        Returns the event that marks the device half done (None when there is nothing new in flight)."""
        if self._gen is None or self._ahead is not self._UNSET:
            return None
        if not torch.cuda.is_available():        # host-only runs (multi-process CPU tests): nothing to overlap
            try:
                self._ahead = (next(self._gen), None)
            except StopIteration:
                self._ahead = None
            return None
        if self._side is None:
            self._side = torch.cuda.Stream()
        if after is not None:
            self._side.wait_event(after)
        try:
            with torch.cuda.stream(self._side):
                batch = next(self._gen)
                done = torch.cuda.Event()
                done.record(self._side)
            self._ahead = (batch, done)
            return done
        except StopIteration:
            self._ahead = None
            return None

    def has_next(self):
        """True when another mini-batch is available (prepares it ahead if that has not happened yet)."""
        if self._gen is None:
            return False
        self.prefetch()
        return self._ahead is not None

    def get_next(self):
        if self._gen is None:
            raise RuntimeError("iterator used before its initializer was run")
        self.prefetch()
        ahead, self._ahead = self._ahead, self._UNSET
        if ahead is None:
            self._ahead = None
            raise OutOfRangeError()
        batch, done = ahead
        if done is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(done)
            if torch.is_tensor(batch[0]):
                batch[0].record_stream(cur)
        return batch
