"""stt._train_loop under both of its callers, no GPU needed: train_acoustic_rnn and train_language_rnn drive a scripted model that
returns given (loss, error rate, step, exhausted) tuples and records what is asked of it.  The expected call sequences are written
out by hand from the two loops this one replaced; they differ in the evaluation cadence only (and in two log lines)."""
import logging

import pytest

import stt
from rnn_speech_amd import labels

WINDOW = 2          # steps_per_checkpoint


class ScriptedModel(object):
    def __init__(self, script, rate, decay):
        self.script, self.rate, self.decay, self.events, self.step_args = list(script), rate, decay, [], set()

    def run_train_step(self, *args):
        self.events.append("step")
        self.step_args.add(args)
        return self.script.pop(0)

    def save(self, sess, directory):
        self.events.append("save " + directory)

    def learning_rate_decay_op(self):
        self.events.append("decay")
        self.rate *= self.decay

    def get_learning_rate(self):
        return self.rate

    def set_learning_rate(self, sess, rate):
        self.rate = rate

    # what only one of the two callers uses
    def run_evaluation(self, sess):
        self.events.append("eval")

    def close(self):
        self.events.append("close")

    def restore(self, sess, directory):
        self.events.append("restore " + directory)

    def add_dataset_input(self, dataset):
        self.events.append("input")

    def evaluate_dataset(self, dataset):
        self.events.append("eval")
        return 1.0, 0.5


def _script(window_errors, exhausted_at):
    """One (loss, err, step, exhausted) per optimiser step: WINDOW steps per entry of window_errors, steps count from 1."""
    steps = [err for err in window_errors for _ in range(WINDOW)]
    return [(1.0, err, n, n in exhausted_at) for n, err in enumerate(steps, 1)]


def _run_acoustic(monkeypatch, script, rate, max_epoch, test_set=("utterance",), steps_per_evaluation=4):
    model = ScriptedModel(script, rate, 0.5)

    class Iterator(object):
        def initializer(self):
            model.events.append("reinit")

    monkeypatch.setattr(stt, "build_acoustic_training_rnn", lambda sess, *a: (model, Iterator(), Iterator()))
    monkeypatch.setattr(stt, "_rebuild_training_input", lambda *a: model.events.append("rebuild"))
    hp = {"checkpoint_dir": "ck", "steps_per_checkpoint": WINDOW, "steps_per_evaluation": steps_per_evaluation,
          "mini_batch_size": 3, "rnn_state_reset_ratio": 0.25}
    stt.train_acoustic_rnn(["train"], list(test_set), hp, {"max_epoch": max_epoch})
    assert len(model.step_args) == 1
    (sess, mini_batch_size, reset_ratio), = model.step_args
    assert isinstance(sess, stt.Session) and (mini_batch_size, reset_ratio) == (3, 0.25)
    return model


def _run_language(monkeypatch, script, rate, max_epoch, test_set=("a fox",)):
    model = ScriptedModel(script, rate, 0.5)
    monkeypatch.setattr(stt, "_language_model", lambda hp, training: model)
    hp = {"checkpoint_dir": "ck", "steps_per_checkpoint": WINDOW, "lm_batch_size": 2, "max_target_seq_length": 20,
          "char_map": labels.ENGLISH_CHAR_MAP, "lm_lr_decay_factor": 0.5}
    got = stt.train_language_rnn(["the fox", "the red fox", "fox"], list(test_set), hp, {"max_epoch": max_epoch, "learn_rate": None})
    assert got is model                                             # also when the rate fell too low
    assert model.step_args == {(None, 1)}                           # one mini-batch per optimiser step, no session
    return model


# Sixteen windows: error 0.5, a worse one, a new minimum (restarts the history), six without improvement (the seventh entry: decay,
# 3e-7 -> 1.5e-7, saved again), a first entry of the new history, six worse ones (decay -> 7.5e-8 < 1e-7: exit, no second save).
# The epoch ends at step 3 (inside window 2) and at step 8 (the last step of window 4).
PLATEAU = dict(script=_script([0.5, 0.6, 0.4] + [0.45] * 6 + [0.45] + [0.5] * 6, exhausted_at=(3, 8)), rate=3e-7, max_epoch=None)


def test_the_acoustic_loop_evaluates_when_the_step_is_a_multiple_of_steps_per_evaluation(monkeypatch, caplog):
    with caplog.at_level(logging.INFO):
        model = _run_acoustic(monkeypatch, **PLATEAU)
    save = "save ck/acoustic/"
    plain = ["step", "step", save]                                  # windows that end on step 2, 6, 10, ..: 4 does not divide it
    evaluated = plain + ["eval", "reinit"]                          # ... on step 4, 8, 12, ..
    assert model.events == (
        plain                                                       # 1
        + ["step", "rebuild", "step", save, "eval", "reinit"]       # 2: the epoch ends in mid-window, the window goes on
        + plain                                                     # 3
        + ["step", "step", "rebuild", save, "eval", "reinit"]       # 4
        + (plain + evaluated) * 2                                   # 5 - 8
        + plain + ["decay", save]                                   # 9: the seventh window of its history
        + evaluated + (plain + evaluated) * 3                       # 10 - 16
        + ["decay"]                                                 # ... and the rate is below 1e-7
        + ["close"])
    assert model.rate == 7.5e-8 and model.script == []
    assert caplog.text.count("Model is not improving, decaying the learning rate") == 2 and "Language model" not in caplog.text
    assert caplog.text.count("Learning rate is too low, exiting") == 1 and "exiting training session" not in caplog.text
    assert caplog.text.count("End of epoch number") == 2


def test_the_language_loop_evaluates_after_every_window(monkeypatch, caplog):
    with caplog.at_level(logging.INFO):
        model = _run_language(monkeypatch, **PLATEAU)
    window = ["step", "step", "save ck", "eval"]
    assert model.events == (
        ["restore ck", "input"]
        + window                                                    # 1
        + ["step", "input", "step", "save ck", "eval"]              # 2: a new epoch's input in mid-window
        + window                                                    # 3
        + ["step", "step", "input", "save ck", "eval"]              # 4
        + window * 4                                                # 5 - 8
        + window + ["decay", "save ck"]                             # 9
        + window * 7                                                # 10 - 16
        + ["decay"])
    assert model.rate == 7.5e-8 and model.script == []
    assert caplog.text.count("Language model is not improving, decaying the learning rate") == 2
    assert "is not improving" not in caplog.text.replace("Language model is not improving", "")
    assert caplog.text.count("Learning rate is too low, exiting") == 1
    assert caplog.text.count("Language model evaluation : loss 1.00000 nats per token (perplexity 2.718) - token error rate 0.50000") == 16


# Epoch limit 1: the first epoch ends on step 2 (the input is rebuilt), the second on step 3, inside window 2 -- the window is cut
# short, its checkpoint is still written, and the loop ends.
LIMIT = dict(script=_script([0.5, 0.5], exhausted_at=(2, 3)), rate=1e-3, max_epoch=1)


@pytest.mark.parametrize("test_set,steps_per_evaluation,evals", ((("utterance",), 4, 0), (("utterance",), 1, 2), ((), 1, 0)))
def test_the_acoustic_loop_stops_at_the_epoch_limit(monkeypatch, caplog, test_set, steps_per_evaluation, evals):
    with caplog.at_level(logging.INFO):
        model = _run_acoustic(monkeypatch, test_set=test_set, steps_per_evaluation=steps_per_evaluation, **LIMIT)
    save, ev = "save ck/acoustic/", ["eval", "reinit"] * (evals // 2)      # (never without a test set, whatever the step)
    assert model.events == ["step", "step", "rebuild", save] + ev + ["step", save] + ev + ["close"]
    assert len(model.script) == 1 and model.rate == 1e-3           # the fourth scripted step was never asked for
    assert caplog.text.count("Max number of epochs reached, exiting train step") == 1
    assert caplog.text.count("Max number of epochs reached, exiting training session") == 1


@pytest.mark.parametrize("test_set,evals", ((("a fox",), 1), ((), 0)))
def test_the_language_loop_stops_at_the_epoch_limit(monkeypatch, caplog, test_set, evals):
    with caplog.at_level(logging.INFO):
        model = _run_language(monkeypatch, test_set=test_set, **LIMIT)
    ev = ["eval"] * evals                                           # (after every window when there are test sentences)
    assert model.events == ["restore ck", "input", "step", "step", "input", "save ck"] + ev + ["step", "save ck"] + ev
    assert len(model.script) == 1
    assert "exiting train step" not in caplog.text                  # (the acoustic loop's line only)
    assert caplog.text.count("Max number of epochs reached, exiting training session") == 1

