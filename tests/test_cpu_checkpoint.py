"""checkpoint.py and engine.ParamStore, no GPU needed: both models' native checkpoints against files written by the code BEFORE the
module existed (tests/golden/checkpoint_*.npz, tools/make_golden.py --checkpoints), the variable-name table, strict loading, and
Engine.check() asking every workspace before it raises."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dp_oracle_engine import CpuLanguageModel, OracleAcousticModel  # noqa: E402
from rnn_speech_amd import checkpoint, lib, ops, stacks  # noqa: E402
from rnn_speech_amd.engine import Engine, ParamLayout  # noqa: E402


def _acoustic():
    model = OracleAcousticModel(2, 8, 2, 10, 4, 5, False, 80)
    model.create_training_rnn(1.0, 1.0, 1.0, 1e-3, 0.5)
    return model


def _language():
    model = CpuLanguageModel(1, 8, 2, 6, 6, 80)
    model.create_training_rnn(1.0, 1.0, 1.0, 1e-3, 0.5)
    return model


def _place_acoustic(golden, directory, drop=()):
    """The golden file as the checkpoint of `directory` (marker file included), without the keys that start with `drop`."""
    z = np.load(golden)
    np.savez(os.path.join(directory, "acousticmodel.ckpt-42.npz"), **{k: z[k] for k in z.files if not k.startswith(drop)})
    with open(os.path.join(directory, "checkpoint"), "w") as fh:
        fh.write('model_checkpoint_path: "acousticmodel.ckpt-42"\n')


def _place_language(golden, directory, drop=()):
    z = np.load(golden)
    os.makedirs(os.path.join(directory, "language"))
    np.savez(CpuLanguageModel.checkpoint_path(directory), **{k: z[k] for k in z.files if not k.startswith(drop)})


def _saved_acoustic(directory):
    with open(os.path.join(directory, "checkpoint")) as fh:
        return os.path.join(directory, fh.read().split('"')[1] + ".npz")


CASES = {"acoustic": (_acoustic, "checkpoint_acoustic.npz", _place_acoustic, _saved_acoustic, 29),
         "language": (_language, "checkpoint_language.npz", _place_language, CpuLanguageModel.checkpoint_path, 21)}
STATE = ("adam/", "rnn_state/")


def _assert_same_file(new_path, golden_path):
    """Key set, dtypes and every array; per named tensor, as saved (the flat buffers' padding is not in the file)."""
    new, gold = np.load(new_path), np.load(golden_path)
    assert sorted(new.files) == sorted(gold.files)
    for k in gold.files:
        assert new[k].dtype == gold[k].dtype and new[k].shape == gold[k].shape, k
        assert np.array_equal(new[k], gold[k]), k


@pytest.mark.parametrize("which", sorted(CASES))
def test_restoring_the_golden_file_and_saving_again_gives_the_same_file(which, golden_dir, tmp_path):
    make, name, place, saved, n_keys = CASES[which]
    golden = os.path.join(golden_dir, name)
    gold = np.load(golden)
    assert len(gold.files) == n_keys
    assert (gold["global_step"].dtype, gold["learning_rate"].dtype, gold["adam/step"].dtype) == (np.int32, np.float32, np.int64)
    # (the fixture is worth something: distinct scalars, non-zero moments and state)
    assert len({int(gold["global_step"]), int(gold["adam/step"]), 0}) == 3 and float(gold["learning_rate"]) != 1e-3
    assert all(np.any(gold[k] != 0) for k in gold.files if k.startswith(STATE))
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir()
    dst.mkdir()
    place(golden, str(src))
    model = make()
    model.restore(None, str(src))
    assert model.global_step.value == int(gold["global_step"]) and model.engine.adam_step == int(gold["adam/step"])
    assert np.float32(model.get_learning_rate()) == gold["learning_rate"]
    model.save(None, str(dst))
    _assert_same_file(saved(str(dst)), golden)
    assert [f for f in os.listdir(os.path.dirname(saved(str(dst)))) if ".tmp" in f] == []      # the temporary file was renamed


@pytest.mark.parametrize("which", sorted(CASES))
def test_a_reference_style_checkpoint_restarts_adam_cold(which, golden_dir, tmp_path):
    make, name, place, _, _ = CASES[which]
    gold = np.load(os.path.join(golden_dir, name))
    place(os.path.join(golden_dir, name), str(tmp_path), drop=STATE)
    model = make()
    eng = model.engine
    eng.adam_m.fill_(0.5)            # a model that has trained: the restore has to clear this
    eng.adam_v.fill_(0.25)
    eng.adam_step = 3
    model.restore(None, str(tmp_path))
    assert eng.adam_step == 0 and not eng.adam_m.any() and not eng.adam_v.any()
    assert model.global_step.value == int(gold["global_step"])
    for k, v in eng.to_numpy().items():
        assert np.array_equal(v, gold[checkpoint.tf_name(k)]), k
    if which == "acoustic":
        assert not eng.state_h.any() and not eng.state_c.any()


def test_without_save_optimizer_state_the_file_holds_the_reference_keys_only(golden_dir, tmp_path):
    golden = os.path.join(golden_dir, "checkpoint_acoustic.npz")
    src, dst = tmp_path / "src", tmp_path / "dst"
    src.mkdir()
    dst.mkdir()
    _place_acoustic(golden, str(src))
    model = _acoustic()
    model.restore(None, str(src))
    model.save_optimizer_state = False
    model.save(None, str(dst))
    new, gold = np.load(_saved_acoustic(str(dst))), np.load(golden)
    assert sorted(new.files) == sorted(k for k in gold.files if not k.startswith(STATE))
    assert not any(k.startswith(STATE) for k in new.files) and len(new.files) == 10
    for k in new.files:
        assert new[k].dtype == gold[k].dtype and np.array_equal(new[k], gold[k]), k


# ParamLayout(2, 8, 5, 80) name -> TensorFlow variable name, as AcousticModel._tf_name gave them before checkpoint.py (written out by
# running that commit's function; LanguageModel._tf_name agreed on the plain stack)
_DENSE = {"input_w": "Input_Layer/input_w", "input_b": "Input_Layer/input_b",
          "output_w": "Output_layer/output_w", "output_b": "Output_layer/output_b"}
_PLAIN = dict(_DENSE, **{"kernel_0": "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel",
                         "bias_0": "rnn/multi_rnn_cell/cell_0/basic_lstm_cell/bias",
                         "kernel_1": "rnn/multi_rnn_cell/cell_1/basic_lstm_cell/kernel",
                         "bias_1": "rnn/multi_rnn_cell/cell_1/basic_lstm_cell/bias"})
NAME_TABLES = {
    "plain": (dict(), _PLAIN),
    "top": (dict(bidirectional=True), dict(_PLAIN, **{
        "bw_kernel_0": "bidirectional_rnn/bw/multi_rnn_cell/cell_0/basic_lstm_cell/kernel",
        "bw_bias_0": "bidirectional_rnn/bw/multi_rnn_cell/cell_0/basic_lstm_cell/bias",
        "bw_kernel_1": "bidirectional_rnn/bw/multi_rnn_cell/cell_1/basic_lstm_cell/kernel",
        "bw_bias_1": "bidirectional_rnn/bw/multi_rnn_cell/cell_1/basic_lstm_cell/bias"})),
    "layer": (dict(bidirectional=True, bidirectional_mode="layer"), dict(_DENSE, **{
        "kernel_0": "stack_bidirectional_rnn/cell_0/bidirectional_rnn/fw/basic_lstm_cell/kernel",
        "bias_0": "stack_bidirectional_rnn/cell_0/bidirectional_rnn/fw/basic_lstm_cell/bias",
        "kernel_1": "stack_bidirectional_rnn/cell_1/bidirectional_rnn/fw/basic_lstm_cell/kernel",
        "bias_1": "stack_bidirectional_rnn/cell_1/bidirectional_rnn/fw/basic_lstm_cell/bias",
        "bw_kernel_0": "stack_bidirectional_rnn/cell_0/bidirectional_rnn/bw/basic_lstm_cell/kernel",
        "bw_bias_0": "stack_bidirectional_rnn/cell_0/bidirectional_rnn/bw/basic_lstm_cell/bias",
        "bw_kernel_1": "stack_bidirectional_rnn/cell_1/bidirectional_rnn/bw/basic_lstm_cell/kernel",
        "bw_bias_1": "stack_bidirectional_rnn/cell_1/bidirectional_rnn/bw/basic_lstm_cell/bias"})),
}


@pytest.mark.parametrize("mode", sorted(NAME_TABLES))
def test_every_layout_name_maps_to_its_tensorflow_variable(mode):
    kw, table = NAME_TABLES[mode]
    layout = ParamLayout(2, 8, 5, 80, **kw)
    assert sorted(layout.names()) == sorted(table)
    assert {n: checkpoint.tf_name(n, layerwise=layout.layerwise) for n in layout.names()} == table
    assert len(set(table.values())) == len(table)


@pytest.mark.parametrize("which", sorted(CASES))
def test_loading_is_strict_about_names_and_shapes(which):
    eng = CASES[which][0]().engine
    with pytest.raises(KeyError, match="nonsense.*layout has input_w, input_b, kernel_0"):
        eng.load_numpy({"nonsense": np.zeros(3, np.float32)})
    words = {"acoustic": r"the model \(L=2, H=8, D=5, C=80\) needs \(8,\)",
             "language": r"the language model \(L=1, H=8, V=80\) needs \(8,\)"}[which]
    with pytest.raises(ValueError, match=r"checkpoint tensor input_b has shape \(1,\), " + words):
        eng.load_numpy({"input_b": np.zeros(1, np.float32)})       # (copy_ would broadcast it)
    with pytest.raises(ValueError, match="input_b"):
        eng.load_numpy({"input_b": np.zeros(1, np.float32)}, flat=eng.adam_m)


class _TwoStacks(object):
    """What Engine.check() reads of a bidirectional "top" engine: its driver, and of that the two stacks' workspaces."""
    check, healthy = Engine.check, Engine.healthy

    def __init__(self):
        self.stack = object.__new__(stacks.JoinedStack)
        self.stack.fw, self.stack.bw = object.__new__(stacks.UniStack), object.__new__(stacks.UniStack)
        self.stack.fw.ws, self.stack.bw.ws = "ws", "ws_b"


@pytest.mark.parametrize("fault_on_b", (False, True))
def test_check_asks_both_workspaces_and_a_fault_is_not_hidden_behind_a_timeout(monkeypatch, fault_on_b):
    asked = []
    errors = {"ws": lib.DataflowTimeout("time-out on ws")}
    if fault_on_b:
        errors["ws_b"] = lib.AmdSpeechError("sticky fault on ws_b")

    def status(ws):
        asked.append(ws)
        if ws in errors:
            raise errors[ws]

    monkeypatch.setattr(ops, "lstm_status", status)
    eng = _TwoStacks()
    with pytest.raises(lib.AmdSpeechError) as ex:
        eng.check()
    assert asked == ["ws", "ws_b"]                 # the second workspace is asked although the first timed out
    assert ex.value is errors["ws_b" if fault_on_b else "ws"]
    if fault_on_b:                                 # not recoverable: healthy() raises it, it does not answer False
        with pytest.raises(lib.AmdSpeechError) as ex:
            eng.healthy()
        assert ex.value is errors["ws_b"] and not isinstance(ex.value, lib.DataflowTimeout)
    else:
        assert eng.healthy() is False
    assert asked == ["ws", "ws_b"] * 2
    errors.clear()
    assert eng.healthy() is True
