"""The forward dataflow kernel's x-product workers at every value of AMDSPEECH_FLOW_FWD_WORKERS -- unset / 2: a block and a half per
recurrence wave (full roles + half roles, lstm_fwd_flow2<4, 0, 1, ., 1>), 1: one block (full roles only), 0: none -- each in a child
process (tests/flow_fwd_split_child.py: the switch is read once per process).  Every value is held to the SAME bounds against the
float64 reference of tests/lstm_stack_ref.py: the ones tests/test_gpu_fullsize.py uses on this path (outputs and state 1e-4 of the
tensor's maximum, per-utterance loss 1e-3, every gradient tensor 2e-3).  The half split need not be bit-equal to the others (the
partial sums of gates f and o are added in another order); it has to stay inside the same bounds.  The plan query says which kernel ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_BOUND, LOSS_BOUND, GRAD_BOUND = 1e-4, 1e-3, 2e-3      # tests/test_gpu_fullsize.py
SWITCH = {"default": None, "2": "2", "1": "1", "0": "0"}
HALVES = {"default": 3, "2": 3, "1": 2, "0": 0}            # amdspeech_lstm_plan_xw_halves where the half roles fit


def _child(mode, switch, tmp_path):
    env = dict(os.environ)
    env.pop("AMDSPEECH_FLOW_FWD_WORKERS", None)
    if SWITCH[switch] is not None:
        env["AMDSPEECH_FLOW_FWD_WORKERS"] = SWITCH[switch]
    dest = str(tmp_path / ("%s_%s.json" % (mode, switch)))
    r = subprocess.run([sys.executable, os.path.join(HERE, "flow_fwd_split_child.py"), mode, dest], env=env, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0, "child %s / %s failed (%d):\n%s\n%s" % (mode, switch, r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    with open(dest) as fh:
        return json.load(fh)


def _judge(name, fig, halves):
    print("%-32s T %4d halves %d  h %.2e c %.2e gates %.2e logits %.2e loss %.2e  grads worst %.2e (%s)" % (
        name, fig["T"], fig["plan"]["xw_halves"], fig["h"], fig["c"], fig["gates"], fig["logits"], fig["loss_rows"],
        max(fig["grads"].values()), max(fig["grads"], key=fig["grads"].get)))
    bad = []
    if fig["plan"]["fwd_path"] != "flow" or fig["plan"]["xw_halves"] != halves or fig["plan"]["mv"] != (1 if halves else 0):
        bad.append("%s: plan %r, expected the flow path with xw_halves = %d" % (name, fig["plan"], halves))
    if not fig["finite"]:
        bad.append("%s: non-finite results" % name)
    for kind in ("h", "c", "gates", "logits"):
        if not fig[kind] < OUT_BOUND:
            bad.append("%s: %s off by %.2e (bound %.1e)" % (name, kind, fig[kind], OUT_BOUND))
    if not fig["loss_rows"] < LOSS_BOUND:
        bad.append("%s: loss off by %.2e (bound %.1e)" % (name, fig["loss_rows"], LOSS_BOUND))
    for k, e in fig["grads"].items():
        if not e < GRAD_BOUND:
            bad.append("%s: gradient %s off by %.2e (bound %.1e)" % (name, k, e, GRAD_BOUND))
    return bad


@pytest.mark.parametrize("switch", ["default", "1", "0"])
def test_headline_shape_and_a_shorter_then_longer_call_on_one_workspace(switch, tmp_path):
    """3x512 / D40 / B32: T = 1001 with equal lengths, then 301 frames with ragged lengths (rows of 301, 300, 1 and 0 frames) and
    T = 1001 again on the SAME workspace: the second long call finds frames 301.. of the tile history -- full and half tiles --
    with the tag the short call did not flip."""
    res = _child("headline", switch, tmp_path)
    bad = []
    for name in ("T1001-equal", "T301-ragged-same-workspace", "T1001-equal-again"):
        bad += _judge(name, res[name], HALVES[switch])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("switch", ["default", "2", "1", "0"])
def test_short_sequences_second_shape_and_the_shapes_without_half_roles(switch, tmp_path):
    """3x512 / B32 at T = 1, 2, 3, 9 (and ragged at 9), 2x512 / B16 ragged; and by the plan query: no half roles (and no other
    change) where no XCD is spare, at H < 512 and at precisions 1 and 2, whatever the switch says."""
    res = _child("small", switch, tmp_path)
    plans = res.pop("_plans")
    bad = []
    for name in sorted(res):
        bad += _judge(name, res[name], HALVES[switch])
    for name, plan in plans.items():
        print(name, plan)
        if plan["fwd_path"] != "flow" or plan["xw_halves"] != 0 or plan["mv"] != 0:
            bad.append("%s: plan %r, expected the flow path without x-product workers" % (name, plan))
    if plans["no-spare-xcd"]["L"] * plans["no-spare-xcd"]["nmt"] != 8:
        bad.append("no-spare-xcd: %r is not a shape with 8 recurrence groups" % plans["no-spare-xcd"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("switch", ["default", "1"])
def test_ten_steps_twice_give_identical_bits(switch, tmp_path):
    """cfg2's shape, ragged lengths, dropout on: loss, logits, the h and c histories and the gates of ten steps, run twice."""
    res = _child("repro", switch, tmp_path)
    assert res["plan"]["xw_halves"] == HALVES[switch], res["plan"]
    assert res["steps"] == 10 and res["identical"], res
