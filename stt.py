# coding=utf-8
"""Command line of the speech recogniser -- same flags and loop semantics as the reference's
stt.py (argument parser :360-404, train loop + LR plateau rule :171-236, file / evaluate modes
:239-324), driving the MI355X-native AcousticModel instead of a TensorFlow session.  Two modes are this build's own:
--align AUDIO --transcript "text" prints when each word of a known transcript was spoken (forced CTC alignment), and
--feature_stats writes the corpus statistics that `feature_norm : global` normalises with.

--train_language trains the character language model of the [lm_network_params] section (rnn_speech_amd.language_model: a
next-token LSTM over the acoustic model's own label alphabet) on lm_text_files or, when that is empty, on the transcripts of the
training and test corpora, with the loop shape of --train_acoustic; single process.  With lm_weight > 0, --evaluate and --file
decode lm_nbest paths per utterance and return argmax(log p_ctc + lm_weight * log p_lm + lm_length_bonus * tokens); with
lm_weight 0 (the default) nothing of the language model is loaded.

--file on a recording longer than max_input_seq_length: with `long_audio : truncate` (the default, the reference's behaviour) the
rest of the file is dropped with a warning; with `long_audio : segment` a voice-activity detector on the GPU finds the pauses
(the vad_* keys), the recording is cut there into spans the model was trained on, the spans run as ordinary mini-batches of
batch_size through the forward pass and the decoder above, and one line -- the spans' texts joined by spaces -- is printed, with
one INFO line `start_s end_s text` per span.  --align and --evaluate do not segment.

Not kept (out of the hot-path scope): --generate_text, --record (pyaudio), --XLA (no tracing
compiler here; accepted and ignored), TensorBoard.  `training_dataset_dirs` takes the reference's corpus
trees (LibriSpeech / TED-LIUM / Shtooka / Vystadial, walked by rnn_speech_amd.corpus) or a `path<TAB>transcript`
manifest.

Data parallel: `python -m torch.distributed.run --nproc-per-node N stt.py --train_acoustic` -- every rank trains on
its own equal-size shard, gradients are summed over RCCL once per optimiser step, the logged loss / error rate (and
therefore the learning-rate plateau rule) are job-wide means, rank 0 writes the checkpoints.
"""
import argparse
import logging
import os
import sys
from random import shuffle

import numpy as np

from models.AcousticModel import AcousticModel, Session, bucketed_order
from models.SpeechRecognizer import SpeechRecognizer
import util.audioprocessor as audioprocessor
import util.dataprocessor as dataprocessor
import util.hyperparams as hyperparams
from rnn_speech_amd import dataparallel
from rnn_speech_amd.audioprocessor import decode_files
from rnn_speech_amd.segmenter import model_frames


def main():
    prog_params = parse_args()
    grp = dataparallel.Group.single()
    if prog_params["train_acoustic"]:
        # one process per GPU (torch.distributed.run): joins the job described by RANK / WORLD_SIZE / LOCAL_RANK
        grp = dataparallel.current()
    # rank 0 owns the checkpoint directory (hyperparams.p, a possibly timestamped sub-directory): the others
    # take its view instead of racing it
    hyper_params = None
    if grp.rank == 0:
        hyper_params = hyperparams.HyperParameterHandler(prog_params["config_file"]).get_hyper_params()
    hyper_params = grp.broadcast_object(hyper_params)
    # (--feature_stats writes the file a `feature_norm : global` processor would want to read: it builds its own, unnormalised)
    audio_processor = None if prog_params["feature_stats"] else build_audio_processor(hyper_params)
    speech_reco = SpeechRecognizer(hyper_params["language"])
    hyper_params["char_map"] = speech_reco.get_char_map()
    hyper_params["char_map_length"] = speech_reco.get_char_map_length()

    if prog_params["train_acoustic"]:
        # ONE shuffle / train-test split for the whole job (load_acoustic_dataset shuffles with an unseeded RNG):
        # rank 0 draws it and every rank shards the same permutation -- disjoint shards of equal size, no test
        # item leaking into another rank's training shard
        sets = None
        if grp.rank == 0:
            sets = speech_reco.load_acoustic_dataset(
                hyper_params["training_dataset_dirs"], hyper_params["test_dataset_dirs"],
                hyper_params["training_filelist_cache"],
                hyper_params["dataset_size_ordering"] in ("True", "First_run_only"), hyper_params["train_frac"])
        train_set, test_set = grp.broadcast_object(sets)
        if hyper_params["dataset_size_ordering"] == "Bucketed" and grp.world > 1:
            # GLOBAL length buckets, dealt across the ranks: optimiser step k is the same bucket on every rank, so the all-reduce
            # never waits for a rank that drew a longer mini-batch (bucketing each rank's shard on its own -- rounds 2 - 4 -- made
            # the step the maximum over `world` unrelated buckets).  The shuffle of the buckets is the job's, drawn by rank 0.
            seed = grp.broadcast_object(int.from_bytes(os.urandom(4), "little") if grp.rank == 0 else None)
            train_set = dataparallel.shard_bucketed(train_set, hyper_params["batch_size"], grp.rank, grp.world, seed)
            hyper_params["dataset_size_ordering"] = "Bucketed_by_job"      # (build_acoustic_training_rnn keeps the order)
        else:
            train_set = dataparallel.shard(train_set, grp.rank, grp.world)
        train_acoustic_rnn(train_set, test_set, hyper_params, prog_params)
    elif prog_params["train_language"]:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("--train_language runs in one process: the language model is not trained data-parallel")
        train_language_rnn(*load_language_dataset(speech_reco, hyper_params), hyper_params, prog_params)
    elif prog_params["file"] is not None:
        process_file(audio_processor, hyper_params, prog_params["file"])
    elif prog_params["evaluate"]:
        evaluate(hyper_params)
    elif prog_params["align"] is not None:
        align_file(audio_processor, hyper_params, prog_params["align"], _transcript(prog_params))
    elif prog_params["feature_stats"]:
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            sys.exit("--feature_stats runs in one process: statistics are not accumulated across data-parallel ranks")
        train_set, _ = speech_reco.load_acoustic_dataset(
            hyper_params["training_dataset_dirs"], hyper_params["test_dataset_dirs"], hyper_params["training_filelist_cache"],
            hyper_params["dataset_size_ordering"] in ("True", "First_run_only"), hyper_params["train_frac"])
        feature_stats(train_set, hyper_params)
    else:
        sys.exit("mode not supported by the MI355X build (see module docstring)")


def build_audio_processor(hyper_params):
    """The front end of every mode, from the config keys; fills in what the model is built from.  Low frame rate input (frame_stack /
    frame_skip): the model reads input_dim = frame_stack * D values per frame and runs out_seq_length = ceil(max_input_seq_length /
    frame_skip) frames; at 1 / 1 these are the feature width and max_input_seq_length themselves."""
    opts = pipeline_options(hyper_params)
    audio_processor = audioprocessor.AudioProcessor(hyper_params["max_input_seq_length"], hyper_params["signal_processing"],
                                                    load_sr=opts.pop("sample_rate"), **opts)
    hyper_params["input_dim"] = audio_processor.feature_size
    hyper_params["out_seq_length"] = audio_processor.out_seq_length
    hyper_params["spec_augment"] = spec_augment_policy(hyper_params, audio_processor)
    conv = conv_option(hyper_params)
    step = conv[3] if conv else audio_processor.frame_skip      # (the two are refused together: one of them is 1)
    model_frames_max = -(-hyper_params["out_seq_length"] // (conv[3] if conv else 1))
    if model_frames_max < hyper_params["max_target_seq_length"]:
        logging.warning("%d model frames (max_input_seq_length %d at %s %d) is below max_target_seq_length %d: "
                        "a transcript with more tokens than its utterance has frames is ignored by the loss",
                        model_frames_max, hyper_params["max_input_seq_length"], "conv_stride" if conv else "frame_skip", step,
                        hyper_params["max_target_seq_length"])
    return audio_processor


def conv_option(hyper_params):
    """AcousticModel.conv from the conv_* keys: None at conv_channels 0 (the default: no such layer), else (C, kt, kf, st, sf, G)
    with G the groups of a source frame -- static, delta and delta-delta of 40 mel bins for fbank, one group of n_mfcc for mfcc."""
    channels = int(hyper_params.get("conv_channels", 0) or 0)
    if channels == 0:
        return None
    (kt, kf), (st, sf) = hyper_params.get("conv_kernel", (11, 21)), hyper_params.get("conv_stride", (2, 2))
    return channels, int(kt), int(kf), int(st), int(sf), 3 if hyper_params["signal_processing"] == "fbank" else 1


def pipeline_options(hyper_params, dataset=False):
    """The input pipeline's keyword arguments from the config keys, THE place their defaults live: what AudioProcessor (which
    calls sample_rate load_sr), AcousticModel.build_dataset (dataset=True: with the decode-ahead depth and the feature cache)
    and the model's own attributes take.  The statistics file is read in global mode only."""
    get = hyper_params.get
    mode = get("feature_norm", "none")
    opts = dict(n_mfcc=get("n_mfcc", 20), sample_rate=get("sample_rate", 22050), frame_stack=get("frame_stack", 1),
                frame_skip=get("frame_skip", 1), feature_norm=mode, feature_norm_variance=get("feature_norm_variance", True),
                feature_stats=get("feature_norm_stats") if mode == "global" else None)
    if dataset:
        opts.update(prefetch=get("prefetch_batches", 2), feature_cache_mb=get("feature_cache_mb", 0))
    return opts


def spec_augment_policy(hyper_params, audio_processor):
    """AcousticModel.spec_augment from the spec_augment_* keys: None when they mask nothing (the default: nothing is launched),
    else the policy of ops.spec_augment plus the seed.  period: the bins of ONE source frame's frequency axis -- 40 mel bins for
    fbank (a bin is masked in the static, delta and delta-delta groups together), n_mfcc for mfcc; under frame_stack the same bin
    is masked in every stacked sub-frame."""
    get = lambda key, dflt=0: hyper_params.get("spec_augment_" + key, dflt)      # noqa: E731
    freq_on = get("freq_masks") > 0 and get("freq_width") > 0
    time_on = get("time_masks") > 0 and get("time_width") > 0 and get("time_permille", 1000) > 0
    if not (freq_on or time_on):
        return None
    period = 40 if audio_processor.feature_type == "fbank" else audio_processor.source_feature_size
    if get("freq_width") > period:
        raise ValueError("spec_augment_freq_width %d exceeds the %d bins of a frame" % (get("freq_width"), period))
    return dict(period=period, freq_masks=get("freq_masks"), freq_width=get("freq_width"), time_masks=get("time_masks"),
                time_width=get("time_width"), time_permille=get("time_permille", 1000), seed=get("seed"))


def speed_perturb_option(hyper_params):
    """AcousticDataset's speed_perturb from the speed_perturb_* keys: None when they are off (the default: nothing is launched),
    else (factors in permille, seed)."""
    factors = list(hyper_params.get("speed_perturb_factors") or [])
    if not factors or factors == [1000]:
        return None
    return factors, int(hyper_params.get("speed_perturb_seed", 0))


def augment_option(hyper_params, device="cuda"):
    """AcousticDataset's augment from the noise_* / reverb_* / augment_* keys: None when both parts are off (the default: nothing is
    read, launched or allocated), else (bank, reverb permille, noise permille, SNR range in tenths of a dB, seed) with the bank
    built from the two directories at sample_rate."""
    from rnn_speech_amd.audioprocessor import AugmentBank
    get = hyper_params.get
    reverb = int(round(1000 * get("reverb_prob", 0.0))) if get("reverb_dir") else 0
    noise = int(round(1000 * get("noise_prob", 0.0))) if get("noise_dir") else 0
    if reverb == 0 and noise == 0:
        return None
    bank = AugmentBank.from_dirs(pipeline_options(hyper_params)["sample_rate"], noise_dir=get("noise_dir") if noise else "",
                                 reverb_dir=get("reverb_dir") if reverb else "", device=device,
                                 max_taps=get("reverb_max_taps", 8192), noise_max_seconds=get("noise_max_seconds", 30.0),
                                 bank_mb=get("augment_bank_mb", 256))
    return bank, reverb, noise, tuple(get("noise_snr_db", (50, 200))), int(get("augment_seed", 0))


def _model_length(hyper_params):
    """Frames the model runs: max_input_seq_length in source frames, divided by frame_skip (rounded up)."""
    return hyper_params.get("out_seq_length", -(-hyper_params["max_input_seq_length"] // pipeline_options(hyper_params)["frame_skip"]))


def _acoustic_model(hyper_params, batch_size, training):
    """The model class the `objective` key names, constructed; objective : ctc (the default) imports nothing of the transducer."""
    args = (hyper_params["num_layers"], hyper_params["hidden_size"], batch_size, _model_length(hyper_params),
            hyper_params["max_target_seq_length"], hyper_params["input_dim"], hyper_params["batch_normalization"],
            hyper_params["char_map_length"])
    if hyper_params.get("objective", "ctc") != "transducer":
        return AcousticModel(*args)
    from rnn_speech_amd import transducer
    transducer.check_options(hyper_params, training)
    model = transducer.TransducerModel(*args)
    model.joint_size = hyper_params.get("transducer_joint_size", 512)
    model.pred_layers = hyper_params.get("transducer_pred_layers", 1)
    model.pred_hidden = hyper_params.get("transducer_pred_hidden", 0) or None
    return model


def _set_model_options(model, hyper_params):
    model.precision = hyper_params.get("precision", "f32")
    model.bidirectional = hyper_params.get("bidirectional", False)
    model.bidirectional_mode = hyper_params.get("bidirectional_mode", "top")
    model.lookahead_context = hyper_params.get("lookahead_context", 0)
    model.conv = conv_option(hyper_params)
    model.sync_batch_norm = hyper_params.get("sync_batch_norm", False)
    model.spec_augment = hyper_params.get("spec_augment")       # (build_audio_processor; only run_step with gradients masks)
    model.decode_blank_skip = hyper_params.get("decode_blank_skip", 0.0)      # (every beam decoder's input; 0: the decoders read every frame)
    opts = pipeline_options(hyper_params)                       # (evaluate_full builds its AudioProcessor from these five)
    for name in ("frame_stack", "frame_skip", "feature_norm", "feature_norm_variance", "feature_stats"):
        setattr(model, name, opts[name])


def build_acoustic_training_rnn(sess, hyper_params, prog_params, train_set, test_set):
    model = _acoustic_model(hyper_params, hyper_params["batch_size"], True)
    ds_args = (hyper_params["batch_size"], hyper_params["max_input_seq_length"],
               hyper_params["max_target_seq_length"], hyper_params["signal_processing"], hyper_params["char_map"])
    _set_model_options(model, hyper_params)
    model.train_decoder = hyper_params.get("train_decoder", "beam")
    model.train_decoder_lag = hyper_params.get("train_decoder_lag", 1)
    if hyper_params["dataset_size_ordering"] == "Bucketed":
        train_set[:] = bucketed_order(train_set, hyper_params["batch_size"])
    pipe = pipeline_options(hyper_params, dataset=True)
    # speed perturbation, noise and reverberation: the TRAINING dataset only
    train_dataset = model.build_dataset(train_set, *ds_args, speed_perturb=speed_perturb_option(hyper_params),
                                        augment=augment_option(hyper_params), **pipe)
    test_dataset = model.build_dataset(test_set, *ds_args, **pipe)
    t_iterator, v_iterator = model.add_datasets_input(train_dataset, test_dataset)
    sess.run(t_iterator.initializer)
    sess.run(v_iterator.initializer)
    model.create_training_rnn(hyper_params["dropout_input_keep_prob"], hyper_params["dropout_output_keep_prob"],
                              hyper_params["grad_clip"], hyper_params["learning_rate"],
                              hyper_params["lr_decay_factor"], use_iterator=True)
    model.add_tensorboard(sess, hyper_params["tensorboard_dir"], prog_params["tb_name"], prog_params["timeline"])
    model.initialize(sess)
    model.restore(sess, hyper_params["checkpoint_dir"] + "/acoustic/")
    if prog_params["learn_rate"] is not None:
        model.set_learning_rate(sess, prog_params["learn_rate"])
    return model, t_iterator, v_iterator


class PlateauSchedule(object):
    """The reference's learning-rate rule (stt.py:219-231): keep the mean training error rate of each
    checkpoint window; a new minimum restarts the history, 7 windows without one trigger a decay."""
    PATIENCE = 7

    def __init__(self):
        self.history = []

    def should_decay(self, window_error_rate):
        best_so_far = min(self.history, default=sys.maxsize)
        if window_error_rate <= best_so_far:
            self.history = []
        self.history.append(window_error_rate)
        if len(self.history) < self.PATIENCE:
            return False
        self.history = []
        return True


def _rebuild_training_input(model, sess, iterator, train_set, hp):
    """End of an epoch: reshuffle (unless the corpus is kept size-ordered) and rewind the iterator."""
    order = hp["dataset_size_ordering"]
    if order in ("False", "First_run_only", "Bucketed", "Bucketed_by_job"):
        if order == "Bucketed_by_job":    # data parallel: the job's global buckets in a new order, the same on every rank
            grp = dataparallel.current()
            seed = grp.broadcast_object(int.from_bytes(os.urandom(4), "little") if grp.rank == 0 else None)
            logging.info("Re-drawing the order of the job's length buckets (seed %d)", seed)
            train_set[:] = dataparallel.reshuffle_buckets(train_set, hp["batch_size"], seed)
        elif order == "Bucketed":         # extra mode of this build: similar lengths per batch, batches shuffled
            logging.info("Re-drawing the order of the length-bucketed mini-batches")
            train_set[:] = bucketed_order(train_set, hp["batch_size"])
        else:
            logging.info("Shuffling the training dataset")
            shuffle(train_set)
        sess.run(iterator.make_initializer(iterator.dataset.with_items(train_set)))   # keeps the feature cache
    else:
        logging.info("Reuse the same training dataset")
        sess.run(iterator.initializer)


def train_acoustic_rnn(train_set, test_set, hyper_params, prog_params):
    hp = hyper_params
    with Session() as sess:
        model, t_iterator, v_iterator = build_acoustic_training_rnn(sess, hp, prog_params, train_set, test_set)

        def evaluate(step):
            if step % hp["steps_per_evaluation"] == 0 and len(test_set) > 0:
                model.run_evaluation(sess)
                sess.run(v_iterator.initializer)

        try:
            _train_loop(model, sess, (hp["mini_batch_size"], hp["rnn_state_reset_ratio"]),
                        lambda: _rebuild_training_input(model, sess, t_iterator, train_set, hp), evaluate,
                        hp["checkpoint_dir"] + "/acoustic/", prog_params["max_epoch"], hp["steps_per_checkpoint"], "Model",
                        epoch_limit_note="Max number of epochs reached, exiting train step")
        finally:
            model.close()       # the asynchronous decoder's threads and pinned buffers: not left to __del__ at interpreter shutdown


def _train_loop(model, sess, step_args, rebuild, evaluate, ckpt_dir, epoch_limit, window, word, epoch_limit_note=None):
    """The reference's training loop (stt.py:171-236), for both models: windows of `window` optimiser steps
    (model.run_train_step(sess, *step_args)), checkpoint, evaluation, plateau rule, stop below a rate of 1e-7.  rebuild() makes the
    next epoch's input when one ends inside the limit; evaluate(step) is called after every window's checkpoint and decides for
    itself (None: nothing to evaluate on); `word` names the model in the decay line and `epoch_limit_note` is logged when the
    limit is reached inside a window."""
    schedule = PlateauSchedule()
    epoch = step = 0

    def out_of_epochs():
        return epoch_limit is not None and epoch > epoch_limit

    while not out_of_epochs():
        window_error = 0.0
        for _ in range(window):
            _loss, err, step, exhausted = model.run_train_step(sess, *step_args)
            window_error += err / window
            if exhausted:
                epoch += 1
                logging.info("End of epoch number : %d", epoch)
                if out_of_epochs():
                    if epoch_limit_note:
                        logging.info(epoch_limit_note)
                    break
                rebuild()
        model.save(sess, ckpt_dir)
        if evaluate is not None:
            evaluate(step)
        if schedule.should_decay(window_error):
            model.learning_rate_decay_op()
            logging.info("%s is not improving, decaying the learning rate", word)
            if model.get_learning_rate() < 1e-7:
                logging.info("Learning rate is too low, exiting")
                return
            model.save(sess, ckpt_dir)      # keep the decayed rate in the checkpoint
    logging.info("Max number of epochs reached, exiting training session")


def _forward_model(hyper_params, batch_size):
    model = _acoustic_model(hyper_params, batch_size, False)
    _set_model_options(model, hyper_params)
    model.create_forward_rnn()
    model.initialize(None)
    model.restore(None, hyper_params["checkpoint_dir"] + "/acoustic/")
    model.rescorer = build_rescorer(hyper_params)
    return model


def _language_model(hyper_params, training):
    from models.LanguageModel import LanguageModel
    hp = hyper_params
    model = LanguageModel(hp["lm_num_layers"], hp["lm_hidden_size"], hp["lm_batch_size"], hp["max_target_seq_length"],
                          hp["max_target_seq_length"], hp["char_map_length"], precision=hp.get("precision", "f32"))
    if training:
        model.create_training_rnn(hp["lm_dropout"], hp["lm_dropout"], hp["lm_grad_clip"], hp["lm_learning_rate"], hp["lm_lr_decay_factor"])
    else:
        model.create_forward_rnn()
    return model


def build_rescorer(hyper_params):
    """AcousticModel.rescorer from the lm_* keys: None at lm_weight 0 (the default: nothing is loaded, launched or allocated,
    whatever lm_fusion says), else the restored language model behind an n-best rescorer (lm_fusion : rescore) or inside the beam
    (lm_fusion : beam).  A missing checkpoint is an error that names the directory."""
    if not hyper_params.get("lm_weight", 0) > 0:
        return None
    from rnn_speech_amd.language_model import FusedDecoder, NbestRescorer
    model = _language_model(hyper_params, training=False)
    model.restore(None, hyper_params["checkpoint_dir"], must_exist=True)
    if hyper_params.get("lm_fusion", "rescore") == "beam":
        return FusedDecoder(model, hyper_params["lm_weight"], lm_length_bonus=hyper_params.get("lm_length_bonus", 0.0))
    return NbestRescorer(model.score, hyper_params["lm_weight"], hyper_params.get("lm_nbest", 16), hyper_params.get("lm_length_bonus", 0.0))


def load_language_dataset(speech_reco, hyper_params):
    """(train sentences, test sentences): the lines of lm_text_files (the last tenth held out), or the transcripts of the training
    and test corpora."""
    clean = dataprocessor.DataProcessor.clean_label
    files = hyper_params.get("lm_text_files") or []
    if files:
        lines = []
        for path in files:
            with open(path) as fh:
                lines += [clean(l) for l in fh if l.strip()]
        cut = max(1, len(lines) - len(lines) // 10)
        return lines[:cut], lines[cut:]
    train_set, test_set = speech_reco.load_acoustic_dataset(
        hyper_params["training_dataset_dirs"], hyper_params["test_dataset_dirs"], hyper_params["training_filelist_cache"],
        False, hyper_params["train_frac"])
    return [item[1] for item in train_set], [item[1] for item in test_set]


def train_language_rnn(train_set, test_set, hyper_params, prog_params):
    """--train_language: the loop of train_acoustic_rnn (_train_loop), one mini-batch per optimiser step, evaluation on the test
    sentences after every window, plateau rule on the window's token error rate."""
    from models.LanguageModel import LanguageModel
    hp = hyper_params
    if not train_set:
        sys.exit("--train_language: no training sentence (lm_text_files / training_dataset_dirs)")
    model = _language_model(hp, training=True)
    model.restore(None, hp["checkpoint_dir"])
    if prog_params["learn_rate"] is not None:
        model.set_learning_rate(None, prog_params["learn_rate"])
    ds_args = (hp["lm_batch_size"], hp["max_target_seq_length"], hp["char_map"])
    test_dataset = LanguageModel.build_dataset(test_set, *ds_args) if test_set else []
    model.add_dataset_input(LanguageModel.build_dataset(train_set, *ds_args))

    def rebuild():
        shuffle(train_set)
        model.add_dataset_input(LanguageModel.build_dataset(train_set, *ds_args))

    def evaluate(step):
        loss, err = model.evaluate_dataset(test_dataset)
        logging.info("Language model evaluation : loss %.5f nats per token (perplexity %.3f) - token error rate %.5f",
                     loss, float(np.exp(min(loss, 50.0))), err)

    _train_loop(model, None, (1,), rebuild, evaluate if test_dataset else None, hp["checkpoint_dir"], prog_params["max_epoch"],
                hp["steps_per_checkpoint"], "Language model")
    return model


_VAD_OPTIONS = ("floor_percentile", "margin_db", "range_db", "min_db", "min_speech_ms", "hangover_ms", "pad_ms")


def process_long_file(audio_processor, hyper_params, signal, sr):
    """--file with long_audio : segment, for a recording longer than the model's input: the voice-activity detector and the cut
    planner (AudioProcessor.segment) give spans of at most max_input_seq_length frames, which run through ONE forward model in
    mini-batches of min(batch_size, spans) rows -- the last one padded with empty rows -- and through the decoder the lm_* keys
    select, each span as an utterance of its own.  Logs start_s end_s text per span; prints and returns [the texts joined by spaces]."""
    vad = {name: hyper_params["vad_" + name] for name in _VAD_OPTIONS if "vad_" + name in hyper_params}
    seg = audio_processor.segment(signal, sr, **vad)
    texts = []
    if seg.spans:
        B = min(hyper_params["batch_size"], len(seg.spans))
        T = audio_processor.out_seq_length
        model = _forward_model(hyper_params, B)
        for i in range(0, len(seg.spans), B):
            part = seg.spans[i:i + B]
            feat, lengths = audio_processor.process_segments(seg.pcm, seg.n, seg.sr, part, rows=B)
            predictions = model.process_input(None, feat, [min(n, T) for n in lengths])
            for (start, count, _, _), p in zip(part, predictions):
                texts.append(dataprocessor.DataProcessor.get_labels_str(hyper_params["char_map"], p))
                logging.info("%.3f %.3f %s", start / float(seg.sr), (start + count) / float(seg.sr), texts[-1])
    transcribed_text = [" ".join(texts)]
    print(transcribed_text)
    return transcribed_text


def process_file(audio_processor, hyper_params, file):
    if hyper_params.get("long_audio", "truncate") == "segment":
        # (a file that fits is not segmented, whatever the key says: it takes the path below)
        signal, sr = decode_files([file])[0]
        if model_frames(len(signal), sr, audio_processor.load_sr, audio_processor.feature_type) > audio_processor.max_input_seq_length:
            return process_long_file(audio_processor, hyper_params, signal, sr)
    feat_vec, original_length = audio_processor.process_audio_file(file)
    T = audio_processor.out_seq_length
    if original_length > T:
        logging.warning("File too long: %d frames, truncated to %d", original_length, T)
    padded = np.zeros((T, 1, feat_vec.shape[1]), np.float32)
    padded[:len(feat_vec), 0] = feat_vec
    model = _forward_model(hyper_params, 1)
    predictions = model.process_input(None, padded, [min(original_length, T)])
    transcribed_text = [dataprocessor.DataProcessor.get_labels_str(hyper_params["char_map"], p) for p in predictions]
    print(transcribed_text)
    return transcribed_text


def _transcript(prog_params):
    if prog_params["transcript_file"] is not None:
        with open(prog_params["transcript_file"]) as fh:
            return fh.read()
    if prog_params["transcript"] is None:
        sys.exit("--align needs --transcript TEXT or --transcript_file PATH")
    return prog_params["transcript"]


def align_file(audio_processor, hyper_params, file, transcript):
    """--align: when was each word of a known transcript spoken?  The restored model at batch 1, the best CTC alignment of the
    transcript's tokens to the frames (AcousticModel.align), tokens grouped into words.  Prints one line per word:
    start_s end_s confidence word -- the times of the word's first and last frame, frame t being t * frame_hop_samples / sample_rate
    into the file (the front end's 10 ms hop times frame_skip, or times the front convolution's time stride: the start of the
    model frame's first source frame)."""
    feat_vec, original_length = audio_processor.process_audio_file(file)
    T = audio_processor.out_seq_length
    if original_length > T:
        logging.warning("File too long: %d frames, truncated to %d", original_length, T)
    padded = np.zeros((T, 1, feat_vec.shape[1]), np.float32)
    padded[:len(feat_vec), 0] = feat_vec
    char_map = hyper_params["char_map"]
    ids = dataprocessor.DataProcessor.get_str_labels(char_map, dataprocessor.DataProcessor.clean_label(transcript), add_eos=False)
    if len(ids) > hyper_params["max_target_seq_length"]:
        sys.exit("transcript too long: %d tokens, max_target_seq_length is %d" % (len(ids), hyper_params["max_target_seq_length"]))
    model = _forward_model(hyper_params, 1)
    tokens = model.align(None, padded, [min(original_length, T)], [ids])[0]
    if not tokens:
        sys.exit("the transcript cannot be aligned to this recording (more tokens than frames?)")
    frame_s = frame_seconds(audio_processor, conv_option(hyper_params))
    words = dataprocessor.DataProcessor.group_words(char_map, tokens)
    for word, first, last, conf in words:
        print("%.3f %.3f %.3f %s" % (first * frame_s, last * frame_s, conf, word))
    return words


def frame_seconds(audio_processor, conv=None):
    """Seconds between the starts of two model frames: what --align multiplies a frame index by.  Behind the front convolution
    (conv_option) a model frame is centred on every st-th source frame: the hop times its time stride."""
    return audio_processor.frame_hop_samples * (conv[3] if conv else 1) / float(audio_processor.load_sr)


def evaluate(hyper_params):
    if hyper_params["test_dataset_dirs"] is None:
        logging.fatal("Setting test_dataset_dirs in config file is mandatory for evaluation mode")
        sys.exit(1)
    _, test_set = SpeechRecognizer.load_acoustic_dataset(hyper_params["test_dataset_dirs"],
                                                         hyper_params["test_dataset_dirs"])
    if not test_set:
        logging.fatal("No files in test set during an evaluation mode")
        sys.exit(1)
    logging.info("Using %d size of test set", len(test_set))
    model = _forward_model(hyper_params, hyper_params["batch_size"])
    opts = pipeline_options(hyper_params)
    try:
        wer, cer = model.evaluate_full(None, test_set, hyper_params["max_input_seq_length"],
                                       hyper_params["signal_processing"], hyper_params["char_map"],
                                       n_mfcc=opts["n_mfcc"], sample_rate=opts["sample_rate"])
    finally:
        model.close()
    print("Resulting WER : {0:.3g} %".format(wer))
    print("Resulting CER : {0:.3g} %".format(cer))
    return wer, cer


def feature_stats(train_set, hyper_params):
    """--feature_stats: mean and variance of every feature dim over the training set, for `feature_norm : global`.  One walk through
    the dataset path the training takes (decode, resample, front end, truncation at max_input_seq_length) with the normalisation,
    the frame stacking and the feature cache OFF whatever the config says: the statistics are those of the raw 10 ms frames.  Per
    mini-batch the GPU reduces every row to its moments (ops.feature_moments) and the host merges them in float64.  Writes the
    file feature_norm_stats names and prints the number of frames."""
    from rnn_speech_amd.feature_norm import FeatureStats, describe_processor
    path = hyper_params.get("feature_norm_stats")
    if not path:
        sys.exit("--feature_stats needs feature_norm_stats (the file to write) in the configuration file")
    off = dict(frame_stack=1, frame_skip=1, feature_norm="none", feature_stats=None, feature_cache_mb=0)
    dataset = AcousticModel.build_dataset(train_set, hyper_params["batch_size"], hyper_params["max_input_seq_length"],
                                          hyper_params["max_target_seq_length"], hyper_params["signal_processing"],
                                          hyper_params["char_map"], **dict(pipeline_options(hyper_params, dataset=True), **off))
    stats = FeatureStats(describe_processor(dataset.audio))
    for feat, lengths, _ in dataset.batches():
        stats.accumulate(feat, lengths)
    if not stats.count > 0:
        sys.exit("--feature_stats: the training set holds no frame")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    stats.save(path)
    print("feature statistics of %d frames (%d dims) written to %s" % (stats.count, stats.mean.shape[0], path))
    return stats


_MODES = (("train_acoustic", "store_true", "train the acoustic model"),
          ("train_language", "store_true", "train the character language model ([lm_network_params]) that rescores n-best lists"),
          ("file", str, "transcribe one wav file"),
          ("record", "store_true", "live microphone mode -- not supported here"),
          ("evaluate", "store_true", "WER / CER of the restored model on the test manifest"),
          ("generate_text", "store_true", "reference stub -- not supported here"),
          ("align", str, "align a known transcript (--transcript / --transcript_file) to one audio file: a line per word"),
          ("feature_stats", "store_true", "write the training set's feature means and variances to feature_norm_stats (feature_norm : global)"))


def parse_args():
    """Same option names as the reference (stt.py:360-404); exactly one mode is required."""
    parser = argparse.ArgumentParser(description="MI355X-native rnn-speech command line")
    modes = parser.add_mutually_exclusive_group(required=True)
    for name, kind, text in _MODES:
        if kind == "store_true":
            modes.add_argument("--" + name, action="store_true", default=False, help=text)
        else:
            modes.add_argument("--" + name, type=kind, default=None, help=text)
    parser.add_argument("--config", default="config.ini", help="configuration file (same keys as the reference)")
    parser.add_argument("--tb_name", default=None, help="kept for compatibility (no TensorBoard here)")
    parser.add_argument("--max_epoch", type=int, default=None, help="stop after this many epochs")
    parser.add_argument("--learn_rate", type=float, default=None, help="override the stored learning rate")
    parser.add_argument("--timeline", action="store_true", help="log per-step timings")
    parser.add_argument("--XLA", action="store_true", help="kept for compatibility, ignored")
    parser.add_argument("--transcript", default=None, help="--align: the text spoken in the file")
    parser.add_argument("--transcript_file", default=None, help="--align: a file holding that text")
    ns = parser.parse_args()
    out = {name: getattr(ns, name) for name, _, _ in _MODES}
    out.update(config_file=ns.config, tb_name=ns.tb_name, max_epoch=ns.max_epoch, learn_rate=ns.learn_rate,
               timeline=ns.timeline, XLA=ns.XLA, transcript=ns.transcript, transcript_file=ns.transcript_file)
    return out


if __name__ == "__main__":
    main()
