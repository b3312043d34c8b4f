"""What a checkpoint of either model is, written once: the reference graph's variable names, the keys of the native .npz and the
model-side values it carries.  numpy only; `store` arguments are an engine.ParamStore (layout, flat buffers, adam_step).

The reference's Saver writes weights, biases, global_step and learning_rate (models/AcousticModel.py:518-522) -- no Adam slots, so
its resumed runs restart Adam cold.  The native .npz keeps those names (a reference checkpoint maps 1:1) and ADDS the optimiser
moments and the Adam step count under `adam/m/<name>`, `adam/v/<name>`, `adam/step`, plus whatever the caller hands in as `extra`
(the acoustic model's `rnn_state/h|c`).  A file with `adam/step` resumes the optimiser warm, one without restarts it
cold.
"""
import os

import numpy as np

TF_NAMES = {"input_w": "Input_Layer/input_w", "input_b": "Input_Layer/input_b",
            "output_w": "Output_layer/output_w", "output_b": "Output_layer/output_b",
            "lookahead_w": "Lookahead_Layer/lookahead_w",       # (the row convolution's taps; only a model with lookahead > 0 has them)
            "conv_w": "Conv_Layer/conv_w", "conv_b": "Conv_Layer/conv_b"}       # (the front convolution; only a model with conv_channels > 0)
# the parts of a transducer's store: the encoder and the prediction network keep their own names under a scope
PART_SCOPES = {"encoder/": "Encoder/", "prediction/": "Prediction/"}
TF_NAMES.update({"joint_w": "Joint_Layer/joint_w", "joint_b": "Joint_Layer/joint_b"})


def tf_name(name, layerwise=False):
    """ParamLayout name -> TensorFlow variable name: the plain stack (tf.nn.dynamic_rnn), the `bw_` stack of the "top" mode
    (tf.nn.bidirectional_dynamic_rnn) and, with `layerwise`, both stacks of the "layer" mode
    (tf.contrib.rnn.stack_bidirectional_dynamic_rnn)."""
    for prefix, scope in PART_SCOPES.items():       # a part of a composed store (transducer.TransducerEngine)
        if name.startswith(prefix):
            return scope + tf_name(name[len(prefix):], layerwise)
    if name in TF_NAMES:
        return TF_NAMES[name]
    d = "bw" if name.startswith("bw_") else "fw"
    kind, l = name[3:].split("_") if d == "bw" else name.split("_")
    if layerwise:
        return "stack_bidirectional_rnn/cell_%s/bidirectional_rnn/%s/basic_lstm_cell/%s" % (l, d, kind)
    if d == "bw":
        return "bidirectional_rnn/bw/multi_rnn_cell/cell_%s/basic_lstm_cell/%s" % (l, kind)
    return "rnn/multi_rnn_cell/cell_%s/basic_lstm_cell/%s" % (l, kind)


def pack(store, global_step, learning_rate, layerwise=False, optimizer=True, extra=None):
    """The dict np.savez takes: what the reference's Saver holds, with `optimizer` the Adam slots, then `extra` as it is."""
    arrays = {tf_name(k, layerwise): v for k, v in store.to_numpy().items()}
    arrays["global_step"] = np.int32(global_step)
    arrays["learning_rate"] = np.float32(learning_rate)
    if optimizer:
        for slot, flat in (("m", store.adam_m), ("v", store.adam_v)):
            for k, v in store.to_numpy(flat).items():
                arrays["adam/%s/%s" % (slot, tf_name(k, layerwise))] = v
        arrays["adam/step"] = np.int64(store.adam_step)
    arrays.update(extra or {})
    return arrays


def write(path, arrays):
    """`path` ends in .npz.  Never a half-written checkpoint: a temporary file beside it, then os.replace."""
    tmp = path[:-4] + ".tmp.npz"
    np.savez(tmp, **arrays)
    os.replace(tmp, path)


def unpack(z, store, layerwise=False):
    """The inverse of pack() on a mapping `z` (np.load's, or tf_bundle.read_bundle's dict): parameters into `store`, Adam warm
    when `adam/step` is there, else zero moments and step.  Returns (global_step, learning_rate, warm)."""
    names = store.layout.names()
    store.load_numpy({k: z[tf_name(k, layerwise)] for k in names})
    warm = "adam/step" in z
    if warm:
        store.load_numpy({k: z["adam/m/" + tf_name(k, layerwise)] for k in names}, flat=store.adam_m)
        store.load_numpy({k: z["adam/v/" + tf_name(k, layerwise)] for k in names}, flat=store.adam_v)
        store.adam_step = int(z["adam/step"])
    else:
        store.adam_m.zero_()
        store.adam_v.zero_()
        store.adam_step = 0
    return int(z["global_step"]), float(z["learning_rate"]), warm


class _Variable(object):
    def __init__(self, value):
        self.value = value

    def eval(self, session=None):
        return self.value


class TrainedModel(object):
    """What AcousticModel and LanguageModel keep beside their engine, under the reference classes' attribute names: the two
    "variables" a checkpoint carries and the hyper-parameters of create_training_rnn.  `session` arguments are ignored."""

    def __init__(self):
        self.engine = None
        self.rnn_created = False
        self.input_keep_prob = self.output_keep_prob = 1.0
        self.grad_clip = self.lr_decay_factor = 1.0
        self.learning_rate_var = _Variable(0.0)
        self.global_step = _Variable(0)

    def _set_training(self, input_keep_prob, output_keep_prob, grad_clip, learning_rate, lr_decay_factor):
        self.input_keep_prob, self.output_keep_prob = float(input_keep_prob), float(output_keep_prob)
        self.grad_clip, self.lr_decay_factor = float(grad_clip), float(lr_decay_factor)
        self.learning_rate_var.value = float(learning_rate)

    def get_learning_rate(self):
        return self.learning_rate_var.value

    def set_learning_rate(self, sess, learning_rate):
        self.learning_rate_var.value = float(learning_rate)

    def learning_rate_decay_op(self):
        self.learning_rate_var.value *= self.lr_decay_factor
        return self.learning_rate_var.value
