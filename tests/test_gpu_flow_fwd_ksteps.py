"""The extended half roles of the forward dataflow kernel (csrc/lstm_flow_fwd.h: lstm_fwd_flow2<4, 0, 1, ., 1, ME>): the half role
of an x-product worker also takes the last ME k-steps of the K block below its own, for gates f and o, and the recurrence wave
multiplies those two N tiles of that block for the other k-steps only.  Each value of AMDSPEECH_FLOW_FWD_WORKERS runs in a child
process (tests/flow_fwd_ksteps_child.py: the switch is read once per process).
  * float64 parity (tests/lstm_stack_ref.py) at the smallest shapes that take half roles, with W_ih reduced to exactly the x units
    that changed hands, to their complement in that K block, and dense: h, c, gates and logits within 1e-4 of the tensor's maximum,
    the bound of tests/test_gpu_fullsize.py for this path.  A dropped, doubled or mis-assigned k-step is an error of order one in
    the first two settings.
  * the plan queries under every value of the switch;
  * bit reproducibility: ten steps twice, and two consecutive launches of one mini-batch.  The ten steps keep their parameters,
    like tests/test_gpu_flow_fwd_split.py's: the weight gradients are summed with f32 atomics, so after an Adam step two runs
    differ in the last bits of the parameters with ANY forward kernel (measured here and under AMDSPEECH_FLOW_FWD_WORKERS=2:
    the child reports that case as `with_apply_identical`, False for both)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_BOUND = 1e-4      # tests/test_gpu_fullsize.py


def _child(mode, switch, tmp_path):
    env = dict(os.environ)
    env.pop("AMDSPEECH_FLOW_FWD_WORKERS", None)
    if switch is not None:
        env["AMDSPEECH_FLOW_FWD_WORKERS"] = switch
    dest = str(tmp_path / ("%s_%s.json" % (mode, switch)))
    r = subprocess.run([sys.executable, os.path.join(HERE, "flow_fwd_ksteps_child.py"), mode, dest], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, "child %s / %s failed (%d):\n%s\n%s" % (mode, switch, r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    with open(dest) as fh:
        return json.load(fh)


def test_float64_parity_on_the_x_units_that_changed_hands(tmp_path):
    res = _child("parity", None, tmp_path)
    assert len(res) == 2 * 3 * 3
    bad = []
    for name in sorted(res):
        fig = res[name]
        print("%-28s ksteps %d  h %.2e c %.2e gates %.2e logits %.2e" % (name, fig["plan"]["xw_ksteps"], fig["h"], fig["c"],
                                                                         fig["gates"], fig["logits"]))
        if fig["plan"]["fwd_path"] != "flow" or fig["plan"]["xw_halves"] != 3 or not fig["plan"]["xw_ksteps"] > 0:
            bad.append("%s: plan %r, expected the flow path with extended half roles" % (name, fig["plan"]))
        if not fig["finite"]:
            bad.append("%s: non-finite results" % name)
        for kind in ("h", "c", "gates", "logits"):
            if not fig[kind] < OUT_BOUND:
                bad.append("%s: %s off by %.2e (bound %.1e)" % (name, kind, fig[kind], OUT_BOUND))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("switch", [None, "2", "1", "0"])
def test_plan_queries(switch, tmp_path):
    plans = _child("plans", switch, tmp_path)
    halves = {None: 3, "2": 3, "1": 2, "0": 0}[switch]
    for name in ("3x512-B32", "2x512-B20", "1x512-B16"):
        p = plans[name]
        print(switch, name, p)
        assert p["fwd_path"] == "flow" and p["xw_halves"] == halves, (switch, name, p)
        if switch is None:
            assert 0 < p["xw_ksteps"] < 4, (name, p)
        else:
            assert p["xw_ksteps"] == 0, (switch, name, p)
    for name in ("no-spare-xcd", "H256", "precision1", "precision2"):
        p = plans[name]
        assert p["fwd_path"] == "flow" and p["xw_halves"] == 0 and p["xw_ksteps"] == 0 and p["mv"] == 0, (switch, name, p)
    assert plans["no-spare-xcd"]["nmt"] * 2 == 8


def test_ten_steps_twice_and_two_consecutive_launches_give_identical_bits(tmp_path):
    res = _child("repro", None, tmp_path)
    assert res["plan"]["xw_halves"] == 3 and res["plan"]["xw_ksteps"] > 0, res["plan"]
    assert res["finite"], res
    print("ten steps twice: identical %s; with an Adam step behind each (not asserted): %s" % (res["identical"], res["with_apply_identical"]))
    assert res["steps"] == 10 and res["identical"], res
    assert res["consecutive_identical"], res
