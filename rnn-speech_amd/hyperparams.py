"""config.ini reader + checkpoint-side pickle logic (reference:
/root/reference/util/hyperparams.py:17-141).  Same section/key names and defaults; a few
optional keys are added for the MI355X build (n_mfcc, sample_rate, frame_stack / frame_skip, lookahead_context, conv_*, feature_norm*, spec_augment_*,
speed_perturb_*, noise_* / reverb_* / augment_*, long_audio / vad_* ...) and the reference's [lm_network_params] section with this build's lm_* keys."""
import configparser
import logging
import os
import pickle
import time

_ACOUSTIC, _GENERAL, _TRAINING, _LOGGING = "acoustic_network_params", "general", "training", "logging"
# a change of any of these makes an existing checkpoint unusable (the reference compares the first four,
# util/hyperparams.py:75-92; n_mfcc / sample_rate are this build's extra keys and change the input layer's
# shape / the features' meaning; so do frame_stack / frame_skip, the low frame rate input, and feature_norm /
# feature_norm_variance: a model trained on normalised features is useless on raw ones.  The statistics file's path is not.
# lookahead_context adds a parameter tensor and a layer; so do conv_channels / conv_kernel / conv_stride, which also set the input
# layer's shape and the frame rate of everything above)
_STRUCTURAL = ("num_layers", "hidden_size", "signal_processing", "language", "n_mfcc", "sample_rate", "bidirectional",
               "bidirectional_mode", "frame_stack", "frame_skip", "feature_norm", "feature_norm_variance", "lookahead_context",
               "conv_channels", "conv_kernel", "conv_stride")
# ... and the training objective with the transducer's sizes (a list of its own: it names a second and a third network)
_STRUCTURAL_OBJECTIVE = ("objective", "transducer_joint_size", "transducer_pred_layers", "transducer_pred_hidden")
_STRUCTURAL_DEFAULTS = {"signal_processing": "mfcc", "language": "", "n_mfcc": 20, "sample_rate": 22050, "bidirectional": False,
                        "bidirectional_mode": "top", "frame_stack": 1, "frame_skip": 1, "feature_norm": "none", "feature_norm_variance": True,
                        "lookahead_context": 0, "conv_channels": 0, "conv_kernel": (11, 21), "conv_stride": (2, 2),
                        "objective": "ctc", "transducer_joint_size": 512, "transducer_pred_layers": 1, "transducer_pred_hidden": 0}
CONV_CHANNELS = (0, 16, 32, 48, 64)


def read_config_file(config_file):
    cp = configparser.ConfigParser()
    cp.read(config_file)
    d = {}
    for key, getter in (("num_layers", cp.getint), ("hidden_size", cp.getint),
                        ("dropout_input_keep_prob", cp.getfloat), ("dropout_output_keep_prob", cp.getfloat),
                        ("batch_size", cp.getint), ("mini_batch_size", cp.getint),
                        ("learning_rate", cp.getfloat), ("lr_decay_factor", cp.getfloat),
                        ("grad_clip", cp.getint), ("signal_processing", cp.get), ("language", cp.get),
                        ("rnn_state_reset_ratio", cp.getfloat)):
        d[key] = getter(_ACOUSTIC, key)
    d["use_config_file_if_checkpoint_exists"] = cp.getboolean(_GENERAL, "use_config_file_if_checkpoint_exists")
    d["steps_per_checkpoint"] = cp.getint(_GENERAL, "steps_per_checkpoint")
    d["steps_per_evaluation"] = cp.getint(_GENERAL, "steps_per_evaluation")
    d["checkpoint_dir"] = cp.get(_GENERAL, "checkpoint_dir")
    d["training_dataset_dirs"] = cp.get(_TRAINING, "training_dataset_dirs")
    d["training_filelist_cache"] = cp.get(_TRAINING, "training_filelist_cache", fallback=None)
    d["test_dataset_dirs"] = cp.get(_TRAINING, "test_dataset_dirs", fallback=None)
    d["train_frac"] = cp.getfloat(_TRAINING, "train_frac", fallback=None)
    d["max_input_seq_length"] = cp.getint(_TRAINING, "max_input_seq_length")
    d["max_target_seq_length"] = cp.getint(_TRAINING, "max_target_seq_length")
    tb = cp.get(_TRAINING, "tensorboard_dir", fallback=None)
    d["tensorboard_dir"] = tb if tb is not None and os.path.exists(tb) else None
    d["batch_normalization"] = cp.getboolean(_TRAINING, "batch_normalization", fallback=False)
    d["dataset_size_ordering"] = cp.get(_TRAINING, "dataset_size_ordering", fallback="False")
    d["log_file"] = cp.get(_LOGGING, "log_file", fallback=None)
    level = cp.get(_LOGGING, "log_level", fallback="WARNING")
    d["log_level"] = getattr(logging, level, None)
    if not isinstance(d["log_level"], int):
        raise ValueError("Invalid log level: %s" % level)
    # MI355X-build extras (absent from the reference's config.ini -> reference behaviour)
    d["n_mfcc"] = cp.getint(_ACOUSTIC, "n_mfcc", fallback=20)
    d["prefetch_batches"] = cp.getint(_TRAINING, "prefetch_batches", fallback=2)    # decode-ahead depth
    d["feature_cache_mb"] = cp.getint(_TRAINING, "feature_cache_mb", fallback=0)    # host feature cache, 0 = off
    d["precision"] = cp.get(_ACOUSTIC, "precision", fallback="f32")       # f32 (exact) | bf16x3 (split MFMA) | bf16 (plain bf16 operands)
    d["sample_rate"] = cp.getint(_TRAINING, "sample_rate", fallback=22050)
    d["bidirectional"] = cp.getboolean(_ACOUSTIC, "bidirectional", fallback=False)
    # top: two stacks joined in front of the output layer; layer: stack_bidirectional_dynamic_rnn (every layer reads both
    # directions of the layer below).  Only read when bidirectional is True.
    d["bidirectional_mode"] = cp.get(_ACOUSTIC, "bidirectional_mode", fallback="top")
    if d["bidirectional_mode"] not in ("top", "layer"):
        raise ValueError("bidirectional_mode must be 'top' or 'layer', not %r" % d["bidirectional_mode"])
    # low frame rate input: frame_stack consecutive 10 ms frames concatenated into one model frame, every frame_skip-th kept
    # (1 / 1: off, the reference's behaviour).  max_input_seq_length stays in source frames
    for key in ("frame_stack", "frame_skip"):
        d[key] = check_range(key, cp.getint(_ACOUSTIC, key, fallback=1), 1, 16)
    # lookahead (row) convolution above the top layer of a unidirectional stack (ops.lookahead_fwd): future model frames each output
    # frame sees.  0: off, the reference's graph
    d["lookahead_context"] = check_range("lookahead_context", cp.getint(_ACOUSTIC, "lookahead_context", fallback=0), 0, 32)
    if d["lookahead_context"] and d["bidirectional"]:
        raise ValueError("lookahead_context : %d with bidirectional : True -- the row convolution gives a unidirectional stack its "
                         "future context; a bidirectional one already reads the whole utterance" % d["lookahead_context"])
    # strided time-frequency convolution between the features and the input Linear (ops.conv2d_fwd): conv_channels 0 (off, the
    # reference's graph: the other two keys are then only checked) | 16 | 32 | 48 | 64; conv_kernel "kt, kf" taps in time and in
    # frequency, both odd; conv_stride "st, sf".  The time stride is the learned form of frame_stack / frame_skip: refused with them
    d.update(read_conv_keys(lambda key, dflt: cp.get(_ACOUSTIC, key, fallback=dflt), d["signal_processing"], d["n_mfcc"],
                            d["frame_stack"], d["frame_skip"]))
    # the training objective: ctc (the reference's, the default: nothing of the transducer is loaded, launched or allocated) |
    # transducer (rnn_speech_amd/transducer.py: a prediction network and a joint network trained with the encoder)
    d.update(read_objective_keys(lambda key, dflt: cp.get(_ACOUSTIC, key, fallback=dflt)))
    # feature normalisation between the front end and the frame stacking (ops.feature_norm): none (the reference's behaviour) |
    # utterance (mean / variance of the utterance itself) | global (of the training corpus, from the file feature_norm_stats names,
    # which `stt.py --feature_stats` writes).  feature_norm_variance False: means only
    d["feature_norm"] = cp.get(_ACOUSTIC, "feature_norm", fallback="none").strip()
    if d["feature_norm"] not in ("none", "utterance", "global"):
        raise ValueError("feature_norm must be 'none', 'utterance' or 'global', not %r" % d["feature_norm"])
    d["feature_norm_variance"] = cp.getboolean(_ACOUSTIC, "feature_norm_variance", fallback=True)
    d["feature_norm_stats"] = (cp.get(_ACOUSTIC, "feature_norm_stats", fallback="") or "").strip() or None
    if d["feature_norm"] == "global" and d["feature_norm_stats"] is None:
        raise ValueError("feature_norm : global needs feature_norm_stats, the file `stt.py --feature_stats` writes")
    d["sync_batch_norm"] = cp.getboolean(_TRAINING, "sync_batch_norm", fallback=False)   # DP only; deviation from the reference
    # the decoder behind the per-mini-batch training error rate: greedy (GPU) | beam (default: the reference's width-100 beam
    # decoder, models/AcousticModel.py:312-314,:641, on host threads, reported `train_decoder_lag` mini-batches late; 0 = wait)
    d["train_decoder"] = cp.get(_TRAINING, "train_decoder", fallback="beam")
    if d["train_decoder"] not in ("greedy", "beam"):
        raise ValueError("train_decoder must be 'greedy' or 'beam', not %r" % d["train_decoder"])
    d["train_decoder_lag"] = cp.getint(_TRAINING, "train_decoder_lag", fallback=1)
    # SpecAugment on training mini-batches (ops.spec_augment): masks per utterance and their largest widths, in mel / cepstral bins
    # and in model frames; no time mask is wider than spec_augment_time_ratio of its utterance.  All 0: off.  NOT structural: the
    # keys change the training data, not the model, and a checkpoint stays usable when they change
    for key, top in (("spec_augment_freq_masks", 8), ("spec_augment_freq_width", 4096), ("spec_augment_time_masks", 16),
                     ("spec_augment_time_width", 2 ** 31 - 1), ("spec_augment_seed", 2 ** 32 - 1)):
        d[key] = check_range(key, cp.getint(_TRAINING, key, fallback=0), 0, top)
    ratio = check_range("spec_augment_time_ratio", cp.getfloat(_TRAINING, "spec_augment_time_ratio", fallback=1.0), 0.0, 1.0)
    d["spec_augment_time_permille"] = int(round(1000 * ratio))
    # speed perturbation of the TRAINING waveforms (ops.resample_rows): a comma-separated list of speed factors, each rounded to
    # permille, one of which is drawn per utterance and epoch.  Absent, empty or 1.0 alone: off.  NOT structural, like SpecAugment
    d["speed_perturb_factors"] = parse_speed_factors(cp.get(_TRAINING, "speed_perturb_factors", fallback=""))
    d["speed_perturb_seed"] = check_range("speed_perturb_seed", cp.getint(_TRAINING, "speed_perturb_seed", fallback=0), 0, 2 ** 32 - 1)
    # noise and reverberation augmentation of the TRAINING waveforms (ops.reverb_rows / ops.noise_mix_rows), behind the speed
    # perturbation: directories of noise clips and of room impulse responses, the probability of each per utterance and epoch, the
    # SNR range in dB.  A part is off when its directory is empty or its probability 0 (the default).  NOT structural, like SpecAugment
    d.update(read_augment_keys(lambda key, dflt: cp.get(_TRAINING, key, fallback=dflt)))
    d.update(read_lm_keys(lambda key, dflt: cp.get(_LM, key, fallback=dflt)))
    d.update(read_long_audio_keys(lambda key, dflt: cp.get(_GENERAL, key, fallback=dflt)))
    d.update(read_decode_keys(lambda key, dflt: cp.get(_GENERAL, key, fallback=dflt)))
    return d


def read_objective_keys(get):
    """objective : ctc | transducer and the transducer's three sizes ([acoustic_network_params], all structural):
    transducer_joint_size (a multiple of 16 in 16 .. 1024, default 512), transducer_pred_layers (1 .. 8, default 1),
    transducer_pred_hidden (a multiple of 16 in 16 .. 4096; 0, the default, stands for hidden_size).  With objective : ctc the
    sizes are only checked."""
    objective = str(get("objective", "ctc")).strip()
    if objective not in ("ctc", "transducer"):
        raise ValueError("objective must be 'ctc' or 'transducer', not %r" % objective)
    joint = check_range("transducer_joint_size", int(get("transducer_joint_size", 512)), 16, 1024)
    if joint % 16:
        raise ValueError("transducer_joint_size : %d must be a multiple of 16" % joint)
    layers = check_range("transducer_pred_layers", int(get("transducer_pred_layers", 1)), 1, 8)
    hidden = check_range("transducer_pred_hidden", int(get("transducer_pred_hidden", 0)), 0, 4096)
    if hidden % 16:
        raise ValueError("transducer_pred_hidden : %d must be a multiple of 16 (0: hidden_size)" % hidden)
    return {"objective": objective, "transducer_joint_size": joint, "transducer_pred_layers": layers, "transducer_pred_hidden": hidden}


def read_conv_keys(get, signal_processing="fbank", n_mfcc=20, frame_stack=1, frame_skip=1):
    """conv_channels / conv_kernel / conv_stride from get(key, default) -> text, checked; a bad value raises ValueError that says
    why.  The frequency axis is the 40 mel bins of fbank (static, delta, delta-delta are the layer's three input groups) or the
    n_mfcc cepstra of mfcc."""
    def ints(key, dflt, count):
        text = get(key, dflt)
        try:
            vals = tuple(int(tok) for tok in str(text).split(","))
        except (ValueError, OverflowError):
            vals = ()
        if len(vals) != count:
            raise ValueError("%s must be %d integers separated by commas, not %r" % (key, count, text))
        return vals

    d = {"conv_channels": ints("conv_channels", "0", 1)[0], "conv_kernel": ints("conv_kernel", "11, 21", 2),
         "conv_stride": ints("conv_stride", "2, 2", 2)}
    if d["conv_channels"] not in CONV_CHANNELS:
        raise ValueError("conv_channels must be one of %s (0: no convolution), not %r" % (", ".join(map(str, CONV_CHANNELS)), d["conv_channels"]))
    (kt, kf), (st, sf) = d["conv_kernel"], d["conv_stride"]
    if not (1 <= kt <= 11 and 1 <= kf <= 41):
        raise ValueError("conv_kernel : %d, %d -- time taps 1 .. 11, frequency taps 1 .. 41" % (kt, kf))
    if kt % 2 == 0 or kf % 2 == 0:
        raise ValueError("conv_kernel : %d, %d -- both sizes must be odd (the padding is (k - 1) / 2 on each side)" % (kt, kf))
    if not (1 <= st <= 4 and 1 <= sf <= 4):
        raise ValueError("conv_stride : %d, %d -- each stride 1 .. 4" % (st, sf))
    if d["conv_channels"]:
        if frame_stack != 1 or frame_skip != 1:
            raise ValueError("conv_channels : %d with frame_stack : %d / frame_skip : %d -- the convolution's time stride is the "
                             "learned form of those two; use one or the other" % (d["conv_channels"], frame_stack, frame_skip))
        bins = 40 if signal_processing == "fbank" else int(n_mfcc)
        width = -(-bins // sf) * d["conv_channels"]
        if width > 4096:
            raise ValueError("conv_channels : %d at conv_stride : %d, %d -- %d output bins x %d channels = %d inputs of the input "
                             "layer, more than 4096" % (d["conv_channels"], st, sf, -(-bins // sf), d["conv_channels"], width))
    return d


LONG_AUDIO_MODES = ("truncate", "segment")
# key -> (default, kind, lo, hi).  The defaults are the customary values of an energy detector; nobody has tuned them on a corpus
_VAD_KEYS = {"vad_floor_percentile": ("10", int, 0, 100), "vad_margin_db": ("10", float, 0.0, 200.0),
             "vad_range_db": ("50", float, 0.0, 400.0), "vad_min_db": ("-70", float, -120.0, 100.0),
             "vad_min_speech_ms": ("50", float, 0.0, 10000.0), "vad_hangover_ms": ("200", float, 0.0, 10240.0),
             "vad_pad_ms": ("100", float, 0.0, 10000.0)}


def read_long_audio_keys(get):
    """Recordings longer than max_input_seq_length under --file ([general]): long_audio (truncate, the default and the reference's
    behaviour | segment: cut at the pauses a voice-activity detector finds, ops.vad_energy / ops.vad_flags / segmenter.py) and the
    detector's vad_* keys.  None is structural.  get(key, default) -> text; a bad value raises ValueError naming its key."""
    d = {"long_audio": (get("long_audio", "truncate") or "truncate").strip().lower()}
    if d["long_audio"] not in LONG_AUDIO_MODES:
        raise ValueError("long_audio : %r is not one of %s" % (d["long_audio"], " | ".join(LONG_AUDIO_MODES)))
    for key, (dflt, kind, lo, hi) in _VAD_KEYS.items():
        text = get(key, dflt)
        try:
            v = kind(str(text).strip())
        except (ValueError, OverflowError):
            raise ValueError("%s must be %s, not %r" % (key, "an integer" if kind is int else "a decimal", text))
        d[key] = check_range(key, v, lo, hi)
    return d


def read_decode_keys(get):
    """Blank-frame skipping in front of every beam decoder ([general]; ops.ctc_blank_skip): decode_blank_skip is 0 (off, the default:
    the decoders read every frame, nothing is launched or allocated) or the blank probability, above 0.5 and at most 1, at and above
    which a frame is skippable; of every run of skippable frames the first is kept.  0.95 .. 0.99 are the customary values; nobody
    has tuned them on a corpus here.  NOT structural: a checkpoint is usable either way.  get(key, default) -> text; a bad value
    raises ValueError naming the range."""
    text = get("decode_blank_skip", "0")
    try:
        v = float(str(text).strip() or "0")
    except (ValueError, OverflowError):
        v = float("nan")
    if not (v == 0.0 or 0.5 < v <= 1.0):
        raise ValueError("decode_blank_skip : %r -- 0 (off) or a blank probability above 0.5 and at most 1" % (text,))
    return {"decode_blank_skip": v}


_LM = "lm_network_params"
LM_FUSION_MODES = ("rescore", "beam")


def read_lm_keys(get):
    """The character language model (rnn_speech_amd.language_model): the reference's [lm_network_params] section -- num_layers,
    hidden_size, dropout (the keep probability of both DropoutWrapper sides), batch_size, learning_rate, lr_decay_factor, grad_clip,
    defaulting to the values of this build's config.ini -- under lm_* names, plus this build's keys: lm_text_files (comma-separated text files,
    one sentence per line; empty: the transcripts of the training and test corpora), lm_weight (0, the default: no rescoring,
    nothing of the language model is loaded), lm_nbest, lm_length_bonus and lm_fusion (rescore, the default: the model picks among
    the lm_nbest paths of the acoustic beam; beam: the model scores every extension inside the beam).  None is structural for the
    acoustic checkpoint.
    get(key, default) -> text; a bad value raises ValueError naming its key."""
    def number(key, dflt, kind, lo, hi):
        text = get(key, dflt)
        try:
            v = kind(str(text).strip())
        except (ValueError, OverflowError):
            raise ValueError("[%s] %s must be %s, not %r" % (_LM, key, "an integer" if kind is int else "a decimal", text))
        return check_range(key, v, lo, hi)

    d = {"lm_num_layers": number("num_layers", "2", int, 1, 16), "lm_hidden_size": number("hidden_size", "256", int, 1, 1 << 16),
         "lm_dropout": number("dropout", "0.9", float, 0.001, 1.0), "lm_batch_size": number("batch_size", "64", int, 1, 1 << 16),
         "lm_learning_rate": number("learning_rate", "0.001", float, 0.0, 1e3),
         "lm_lr_decay_factor": number("lr_decay_factor", "0.5", float, 0.0, 1.0), "lm_grad_clip": number("grad_clip", "5", float, 0.0, 1e9)}
    d["lm_text_files"] = [p.strip() for p in (get("lm_text_files", "") or "").split(",") if p.strip()]
    d["lm_weight"] = number("lm_weight", "0", float, 0.0, 1e3)
    d["lm_nbest"] = number("lm_nbest", "16", int, 1, 1000)
    d["lm_length_bonus"] = number("lm_length_bonus", "0", float, -1e3, 1e3)
    d["lm_fusion"] = (get("lm_fusion", "rescore") or "rescore").strip().lower()
    if d["lm_fusion"] not in LM_FUSION_MODES:
        raise ValueError("lm_fusion : %r is not one of %s" % (d["lm_fusion"], " | ".join(LM_FUSION_MODES)))
    return d


def read_augment_keys(get):
    """The noise_* / reverb_* / augment_* keys from get(key, default) -> text, checked; a bad value raises ValueError naming its key."""
    def number(key, dflt, kind, lo, hi):
        text = get(key, dflt)
        try:
            v = kind(str(text).strip())
        except (ValueError, OverflowError):
            raise ValueError("%s must be %s, not %r" % (key, "an integer" if kind is int else "a decimal", text))
        return check_range(key, v, lo, hi)

    d = {"noise_dir": (get("noise_dir", "") or "").strip(), "reverb_dir": (get("reverb_dir", "") or "").strip()}
    d["noise_prob"] = number("noise_prob", "0", float, 0.0, 1.0)
    d["reverb_prob"] = number("reverb_prob", "0", float, 0.0, 1.0)
    d["noise_snr_db"] = parse_snr_range(get("noise_snr_db", "5, 20"))
    d["noise_max_seconds"] = number("noise_max_seconds", "30", float, 0.001, 3600.0)
    d["reverb_max_taps"] = number("reverb_max_taps", "8192", int, 1, 8192)
    d["augment_bank_mb"] = number("augment_bank_mb", "256", int, 1, 1 << 20)
    d["augment_seed"] = number("augment_seed", "0", int, 0, 2 ** 32 - 1)
    return d


def parse_snr_range(text):
    """"5, 20" -> (50, 200): lo and hi of the SNR draw in tenths of a dB, lo <= hi inside -20 .. 60 dB; one number is both."""
    try:
        vals = [int(round(10 * float(tok))) for tok in (text or "").split(",") if tok.strip()]
    except (ValueError, OverflowError):
        raise ValueError("noise_snr_db must be 'lo, hi' in dB, not %r" % text)
    if not 1 <= len(vals) <= 2:
        raise ValueError("noise_snr_db must be 'lo, hi' in dB, not %r" % text)
    return check_snr_decidb("noise_snr_db", (vals[0], vals[-1]))


def parse_speed_factors(text):
    """"0.9, 1.0, 1.1" -> [900, 1000, 1100]: at most 8 decimals of 0.5 .. 2.0, each rounded to permille; [] (off) for an empty
    list or 1.0 alone."""
    try:
        factors = [int(round(1000 * float(tok))) for tok in (text or "").split(",") if tok.strip()]
    except (ValueError, OverflowError):          # (int() of a NaN / of an infinity)
        raise ValueError("speed_perturb_factors must be a comma-separated list of decimals, not %r" % text)
    return [] if factors in ([], [1000]) else check_speed_factors("speed_perturb_factors", factors)


# One checker per option, for the config keys above and for the arguments AcousticDataset takes (a probability is check_range's
# 0 .. 1 as a config key, 0 .. 1000 in permille); each returns what it was given
def check_speed_factors(name, factors):
    if not 1 <= len(factors) <= 8 or any(not 500 <= f <= 2000 for f in factors):
        raise ValueError("%s: 1 .. 8 factors of 500 .. 2000 permille (0.5 .. 2.0), not %r" % (name, factors))
    return factors


def check_snr_decidb(name, snr):
    if not -200 <= snr[0] <= snr[1] <= 600:
        raise ValueError("%s: lo <= hi inside -200 .. 600 tenths of a dB (-20 .. 60 dB), not %r" % (name, snr))
    return snr


def check_range(name, v, lo, hi):
    if not lo <= v <= hi:          # (a NaN fails both comparisons)
        raise ValueError("%s must be in %s .. %s, not %r" % (name, lo, hi, v))
    return v


class HyperParameterHandler(object):
    def __init__(self, config_file):
        hp = self.hyper_params = read_config_file(config_file)
        if hp["log_file"] is not None:
            logging.basicConfig(filename=hp["log_file"])
        logging.getLogger().setLevel(hp["log_level"])
        logging.info("Using checkpoint %s", hp["checkpoint_dir"])
        os.makedirs(hp["checkpoint_dir"], exist_ok=True)
        self.file_path = os.path.join(hp["checkpoint_dir"], "hyperparams.p")
        if not self.check_exists():
            self.save_params(hp)
            logging.info("No hyper params detected at checkpoint... reading config file")
        elif not self.check_changed(hp):
            logging.info("No hyper parameter changed detected, using old checkpoint...")
        elif not hp["use_config_file_if_checkpoint_exists"]:
            self.hyper_params = self.get_params()
            logging.info("Restoring hyper params from previous checkpoint...")
        else:   # structural change + "use config file": start a fresh, timestamped checkpoint dir
            sub = "{0}_hidden_size_{1}_numlayers_{2}_signal_processing_{3}".format(
                int(time.time()), hp["hidden_size"], hp["num_layers"], hp["signal_processing"])
            hp["checkpoint_dir"] = os.path.join(hp["checkpoint_dir"], sub)
            os.makedirs(hp["checkpoint_dir"])
            self.file_path = os.path.join(hp["checkpoint_dir"], "hyperparams.p")
            self.save_params(hp)

    def get_hyper_params(self):
        return self.hyper_params

    def save_params(self, dic):
        with open(self.file_path, "wb") as fh:
            pickle.dump(dic, fh)

    def get_params(self):
        with open(self.file_path, "rb") as fh:
            return pickle.load(fh)

    def check_exists(self):
        return os.path.exists(self.file_path)

    def check_changed(self, new_params):
        if not self.check_exists():
            return False
        old = self.get_params()
        for k, v in _STRUCTURAL_DEFAULTS.items():     # compatibility defaults (older pickles, the reference's own)
            old.setdefault(k, v)
        return any(old[k] != new_params.get(k, _STRUCTURAL_DEFAULTS.get(k)) for k in _STRUCTURAL + _STRUCTURAL_OBJECTIVE)

    read_config_file = staticmethod(read_config_file)
