"""float64 parity of amdspeech_ctc_loss_fwd_bwd per recursion kernel, at full-width targets: every case of tests/ctc_ref.py through
ops.ctc_loss_fwd_bwd -- the plan first (ops.ctc_plan must name the kernel the case was written for), then the loss, every slice of
dlogits and the invariants against bounds that come from the CPU emulation of the kernel's arithmetic (ctc_ref.py, "Bounds").
The two fallback settings of the ladder (AMDSPEECH_CTC_SHIFT=0, and with AMDSPEECH_CTC_PAIR=0) are read once per process, so their
cases run in a fresh child process each."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def current_mode():
    shift = os.environ.get("AMDSPEECH_CTC_SHIFT", "1") != "0"
    pair = os.environ.get("AMDSPEECH_CTC_PAIR", "1") != "0"
    return "default" if shift else ("shift0" if pair else "pair0")


MODE = current_mode()
NAMES = [c["name"] for c in R.CASES if MODE in c["plan"]]
# one case per recursion kernel for the reused-workspace check (in the fallback modes: the kernel the mode brings in)
REUSE = {"default": ["wave-full", "shift-full", "pair-full-255", "edge4-full", "edge-R3-repeats", "edge20-long"],
         "shift0": ["shift-full"], "pair0": ["shift-full", "pair-full-255"]}[MODE]


@pytest.fixture(scope="module")
def ops():
    from rnn_speech_amd import ops as o
    return o


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def run(ops, ev, ws=None):
    loss, d = ops.ctc_loss_fwd_bwd(dev(ev["logits"]), dev(ev["dense"], torch.int32), dev(ev["lengths"], torch.int32), ws=ws)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), d.cpu().numpy()


def assert_plan(ops, c):
    plan = ops.ctc_plan(c["T"], c["B"], c["C"], c["U"])
    kernel, rmax = c["plan"][MODE]
    assert (plan["kernel"], plan["rmax"]) == (kernel, rmax), (c["name"], MODE, plan)
    assert plan["smax"] == 2 * c["U"] + 1 and plan["threads"] == (64 if kernel == "wave" else 256)
    return plan


@pytest.mark.parametrize("name", NAMES)
def test_ctc_case(ops, name):
    c = R.by_name(name)
    assert_plan(ops, c)
    ev = R.evaluated(name, MODE)
    loss, d = run(ops, ev)
    fails, worst = R.judge(ev, loss, d)
    print("CTCPATH %s %s %s worst error/bound %.3f" % (name, MODE, ev["fam"], worst))
    assert not fails, "%s [%s, %s]:\n  " % (name, MODE, ev["fam"]) + "\n  ".join(fails[:12])


@pytest.mark.parametrize("name", REUSE)
def test_ctc_reused_workspace_gives_the_same_bits(ops, name):
    """alpha / beta are written only for s < S, t < len: whatever an earlier call (or nobody) left in the workspace beyond that must
    not reach a result.  A fresh workspace, one filled with NaN, and one a full-width mini-batch of the same shape ran in before."""
    c = R.by_name(name)
    assert_plan(ops, c)
    ev = R.evaluated(name, MODE)
    T, B, C, U = c["T"], c["B"], c["C"], c["U"]
    fresh = ops.CtcWorkspace(T, B, C, U)
    fresh.buf.zero_()
    loss0, d0 = run(ops, ev, fresh)
    nan = ops.CtcWorkspace(T, B, C, U)
    nan.buf.view(torch.float32).fill_(float("nan"))
    loss1, d1 = run(ops, ev, nan)
    assert np.array_equal(loss0, loss1) and np.array_equal(d0, d1)
    # a full-width mini-batch first: every row min(U, T) labels over all T frames
    rng = np.random.RandomState(5)
    n = min(U, T)
    dense = np.zeros((B, U), np.int32)
    dense[:, :n] = 1 + (np.arange(n)[None, :] + np.arange(B)[:, None]) % (C - 2) if C > 3 else 1
    if C > 3:       # adjacent labels differ, so n frames suffice
        assert (dense[:, 1:n] != dense[:, :n - 1]).all()
    used = ops.CtcWorkspace(T, B, C, U)
    first_loss, _ = ops.ctc_loss_fwd_bwd(dev(rng.randn(T, B, C).astype(np.float32)), dev(dense, torch.int32), dev(np.full(B, T, np.int32), torch.int32), ws=used)
    if C > 3:
        assert (first_loss.cpu().numpy() > 0).all()
    loss2, d2 = run(ops, ev, used)
    assert np.array_equal(loss0, loss2) and np.array_equal(d0, d2)


if MODE == "default":      # (the child processes of the last test run the cases alone)
    def test_label_width_2560_is_refused_without_a_launch(ops):
        from rnn_speech_amd import lib
        T, B, C, U = 4, 2, 80, 2560
        with pytest.raises(lib.AmdSpeechError, match="2559"):
            ops.ctc_plan(T, B, C, U)
        logits = torch.zeros(T, B, C, device="cuda")
        d = torch.full_like(logits, 7.0)
        loss = torch.full((B,), 7.0, device="cuda")
        ws = ops.CtcWorkspace(T, B, C, U)
        ws.buf.fill_(0x55)
        with pytest.raises(lib.AmdSpeechError, match="2559"):
            ops.ctc_loss_fwd_bwd(logits, torch.ones(B, U, dtype=torch.int32, device="cuda"), torch.full((B,), T, dtype=torch.int32, device="cuda"),
                                 ws=ws, loss=loss, dlogits=d)
        torch.cuda.synchronize()
        assert (d == 7.0).all() and (loss == 7.0).all() and (ws.buf == 0x55).all()      # nothing ran
        with pytest.raises(lib.AmdSpeechError, match="too large"):
            ops.ctc_plan(T, B, 4097, 10)


    @pytest.mark.parametrize("mode", ["shift0", "pair0"])
    def test_ctc_cases_under_the_fallback_switches(mode):
        """The cases that name a plan for AMDSPEECH_CTC_SHIFT=0 (two frames per LDS exchange from 129 states on) and for
        AMDSPEECH_CTC_SHIFT=0 AMDSPEECH_CTC_PAIR=0 (one frame per exchange, RMAX 2), in a fresh child process with its own time limit."""
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-k",
                              "test_ctc_case or test_ctc_reused_workspace"],
                             env=dict(os.environ, **R.MODES[mode]), capture_output=True, text=True, timeout=900)
        for line in out.stdout.splitlines():
            if "CTCPATH" in line:
                print(line[line.index("CTCPATH"):])
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
        n = sum(1 for c in R.CASES if mode in c["plan"])
        assert out.stdout.count("CTCPATH ") == n, (n, out.stdout[-2000:])
