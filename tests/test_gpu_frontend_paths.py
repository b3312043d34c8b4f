"""Float64 parity of the audio front end per kernel variant: every case of tests/frontend_ref.py -- the plan first
(ops.frontend_plan must name the kernels and the geometry the case was written for), then the cached workspace filled with 0xFF
bytes (a read of a frame nobody wrote shows as NaN), the call, and per row: the frame count, the stage quantity (the clamped
log-mel recovered through the inverse DCT at n_mfcc = 128; fbank: the static dims, and the delta dims on their own) against
float64 within 8 x the float32 emulation's error, the final features within 2e-3, exact zeros past the utterance, nothing
non-finite.  AMDSPEECH_FRONTEND_MFMA is read once per process, so the cases that name a plan for the vector-ALU kernels run again
in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MODE = "fallback" if os.environ.get("AMDSPEECH_FRONTEND_MFMA", "1") == "0" else "default"
NAMES = [c["name"] for c in R.CASES if MODE in c["plan"]]


@pytest.fixture(scope="module")
def ops():
    from rnn_speech_amd import ops as o
    return o


def assert_plan(ops, c):
    plan = ops.frontend_plan(**R.plan_args(c))
    diff = {k: (v, plan[k]) for k, v in c["plan"][MODE].items() if plan[k] != v}
    assert not diff, (c["name"], MODE, diff, plan)
    assert plan == R.expected_plan(c["mode"], c["sr"], c["n_mfcc"], c["B"], c["n_max"], c["t_max"], mfma=MODE == "default"), (c["name"], plan)
    return plan


def poison_workspace(ops, c, device):
    """The workspace ops.frontend caches for this call, created here if need be, every byte 0xFF."""
    from rnn_speech_amd import lib
    imode = ops.MODE_MFCC if c["mode"] == "mfcc" else ops.MODE_FBANK
    key = (imode, c["B"], c["n_max"], c["sr"], device)
    ws = ops._frontend_ws.get(key)
    if ws is None:
        nbytes = lib.load().amdspeech_frontend_workspace_bytes(imode, c["B"], c["n_max"], c["sr"])
        assert nbytes > 0
        ops._frontend_ws.clear()
        ws = ops._frontend_ws[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    ws.fill_(0xFF)
    return ws


def run_case(ops, c):
    """-> (list of failures, worst stage error, worst delta error, worst feature error)"""
    pcm_host, rows = R.batch(c["name"])
    pcm = torch.from_numpy(pcm_host).cuda()
    ws = poison_workspace(ops, c, pcm.device)
    feat, lengths = ops.frontend(pcm, rows, c["sr"], c["mode"], c["t_max"], c["n_mfcc"])
    torch.cuda.synchronize()
    assert ops._frontend_ws[(ops.MODE_MFCC if c["mode"] == "mfcc" else ops.MODE_FBANK, c["B"], c["n_max"], c["sr"], pcm.device)] is ws
    D = c["n_mfcc"] if c["mode"] == "mfcc" else 120
    assert feat.shape == (c["t_max"], c["B"], D)
    feat = feat.cpu().numpy()
    fails = []
    if not np.isfinite(feat).all():
        fails.append("%d non-finite features" % int((~np.isfinite(feat)).sum()))
    b_feat, b_stage, b_delta = R.bounds(c)
    worst = [0.0, 0.0, 0.0]
    for b, ref in enumerate(R.reference(c["name"])):
        want = R.num_frames(c["mode"], c["sr"], rows[b])
        if lengths[b] != want or want != len(ref["feat"]):
            fails.append("row %d: %d frames reported, %d expected, %d in the reference" % (b, lengths[b], want, len(ref["feat"])))
            continue
        n = min(want, c["t_max"])
        if feat[n:, b].any():
            fails.append("row %d: %d non-zero values past frame %d" % (b, int(np.count_nonzero(feat[n:, b])), n))
        e_feat, e_stage, e_delta = R.row_errors(c, ref, feat[:n, b])
        for i, (e, bound, what) in enumerate(((e_feat, b_feat, "features"), (e_stage, b_stage, "stage quantity"), (e_delta, b_delta, "delta dims"))):
            if e is None or bound is None:
                continue
            worst[i] = max(worst[i], e)
            if not e <= bound:          # (<=: where float32 itself is exact, as the deltas of digital silence are, the bound is 0)
                fails.append("row %d (%d samples, %d frames): %s off by %.3g > %.3g" % (b, rows[b], want, what, e, bound))
    if c["kinds"] == ["silence"]:
        if c["mode"] == "mfcc":          # c0 = -100 sqrt(128), the rest 0
            if not (np.abs(feat[:, 0, 0] + 100.0 * np.sqrt(128.0)).max() < R.FEATURE_TOL and np.abs(feat[:, 0, 1:]).max() < R.FEATURE_TOL):
                fails.append("silence: c0 %.6g, rest up to %.3g" % (feat[0, 0, 0], np.abs(feat[:, 0, 1:]).max()))
        elif not np.abs(feat).max() <= 1.1e-8:
            fails.append("silence: |x| up to %.3g" % np.abs(feat).max())
    return fails, worst


@pytest.mark.parametrize("name", NAMES)
def test_frontend_case(ops, name):
    c = R.by_name(name)
    plan = assert_plan(ops, c)
    fails, (w_feat, w_stage, w_delta) = run_case(ops, c)
    stage = "%.3g" % w_stage if c["stage"] else "-"
    if c["mode"] == "fbank":
        stage += "/%.3g" % w_delta
    print("FRONTPATH %s %d/%d dct=%d worst_stage=%s worst_feature=%.3g" % (name, plan["frames_kernel"], plan["maxq"], plan["dct_kernel"], stage, w_feat))
    assert not fails, "%s [%s]:\n  " % (name, MODE) + "\n  ".join(fails[:12])


if MODE == "default":      # (the child process of this test runs the cases alone)
    def test_frontend_cases_under_the_vector_alu_switch():
        """The cases that name a plan for AMDSPEECH_FRONTEND_MFMA=0 (the vector-ALU frame kernel and DCT at the matrix-core kernels'
        shapes), in a fresh child process with its own time limit."""
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-k", "test_frontend_case"],
                             env=dict(os.environ, **R.FALLBACK_ENV), capture_output=True, text=True, timeout=600)
        for line in out.stdout.splitlines():
            if "FRONTPATH" in line:
                print(line[line.index("FRONTPATH"):], "[fallback]")
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
        n = sum(1 for c in R.CASES if "fallback" in c["plan"])
        assert out.stdout.count("FRONTPATH ") == n, (n, out.stdout[-2000:])
