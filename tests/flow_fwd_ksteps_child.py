"""Child process of tests/test_gpu_flow_fwd_ksteps.py (AMDSPEECH_FLOW_FWD_WORKERS is read once per process):
`python flow_fwd_ksteps_child.py <mode> <out.json>` runs one mode on the GPU and writes figures as JSON; the parent asserts.  The
figures are relative errors max|got - ref| / max|ref| per tensor against the float64 reference of tests/lstm_stack_ref.py, as in
tests/flow_fwd_split_child.py, whose helpers this file uses."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_fwd_split_child as S  # noqa: E402

S.D = 20                          # (the input width of these shapes; the helpers read it at call time)
KB, MV = 4, 1                     # H = 512: K blocks of 16 rows per recurrence wave and half; blocks the full roles take


def x_unit_mask(H, me, which):
    """[H rows of W_ih, 4H columns]: True where the weight stays.  Row k is k-step k % 4 of K block k // 16 (pack_fwd_kernel /
    packed_off: k = kb * 16 + 4 * kq + m), block (k // 16) % KB of its recurrence wave; column g * H + u is gate g (i, j, f, o).
    "owned": what the extended half role adds -- k-steps 4-ME .. 3 of block KB-2-MV, gates f and o; "kept": the rest of that block for
    those gates, which the recurrence wave still multiplies; "dense": everything."""
    m = np.zeros((H, 4 * H), bool)
    if which == "dense":
        m[:] = True
        return m
    k = np.arange(H)
    in_block = (k // 16) % KB == KB - 2 - MV
    rows = in_block & ((k % 4 >= 4 - me) if which == "owned" else (k % 4 < 4 - me))
    m[rows, 2 * H:] = True
    return m


def plan_numbers(ws, head=None):
    from rnn_speech_amd import ops
    plan = ops.lstm_plan(ws, head=head)
    return dict(fwd_path=plan["fwd_path"], mv=plan["mv"], nmt=plan["nmt"], xw_halves=ops.lstm_plan_xw_halves(ws, head=head),
                xw_ksteps=ops.lstm_plan_xw_ksteps(ws, head=head))


def mode_parity():
    """1x512 / B16 and 2x512 / B20 (1 and 4 recurrence groups), D = 20, T in {1, 2, 5}, no dropout; W_ih of every layer masked to
    the x units the extended half role owns / their complement in that K block / dense."""
    out = {}
    for (L, H, B) in ((1, 512, 16), (2, 512, 20)):
        for T in (1, 2, 5):
            for which in ("owned", "kept", "dense"):
                eng, p = S.new_engine(L, H, B, T, seed=77)
                me = plan_numbers(eng._ws, head=eng._head)["xw_ksteps"]
                rng = np.random.RandomState(5)
                keep = x_unit_mask(H, max(me, 1), which)      # (me = 0 never reaches the comparison: the parent rejects the plan first)
                for l in range(L):
                    k = p["kernel_%d" % l].copy()
                    if which != "dense":                      # few rows stay: weights of order one keep the pre-activations of order one
                        k[:H] = (rng.randn(H, 4 * H) * 0.5).astype(np.float32) * keep
                    p["kernel_%d" % l] = k
                eng.load_numpy(p)
                lengths = np.full(B, T, np.int32)
                x, dense = S.make_batch(T, B, 100 + T, lengths)
                fig, _ = S.step_and_compare(eng, p, x, dense, lengths, L, B, H)
                fig["plan"]["xw_ksteps"] = me
                fig.pop("grads")
                out["%dx%d-B%d-T%d-%s" % (L, H, B, T, which)] = fig
    return out


def mode_plans():
    from rnn_speech_amd import ops
    out = {}
    for name, (T, B, H, L, pr) in {"3x512-B32": (16, 32, 512, 3, 0), "2x512-B20": (5, 20, 512, 2, 0), "1x512-B16": (5, 16, 512, 1, 0),
                                   "no-spare-xcd": (8, 64, 512, 2, 0), "H256": (16, 32, 256, 3, 0),
                                   "precision1": (16, 32, 512, 3, 1), "precision2": (16, 32, 512, 3, 2)}.items():
        ws = ops.LstmWorkspace(T, B, H, L, precision=pr)
        out[name] = plan_numbers(ws)
    return out


def _bits(eng, L, B, H):
    return (eng.loss.cpu().numpy().copy(), eng.logits.cpu().numpy().copy()) + S.bit_sums(eng, L, B, H)


def mode_repro():
    """3x512 / B32 / T40, ragged lengths with rows of 1 and 0 frames, dropout 0.8 / 0.5: ten steps (a fresh dropout seed each) twice
    on fresh engines, and two consecutive forward launches of one mini-batch (the tile history carries the other parity in the
    second).  The parameters stay put between the ten steps, as in tests/flow_fwd_split_child.py: the weight gradients are summed
    with f32 atomics, so an Adam step makes two runs differ in the last bits of every parameter whatever the forward kernel does
    (`with_apply_identical` reports that case and is not asserted)."""
    L, H, B, T = 3, 512, 32, 40
    lengths = S.ragged(T, B, 9)
    x, dense = S.make_batch(T, B, 0, np.maximum(lengths, 1))
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()

    def ten_steps(apply):
        eng, _p = S.new_engine(L, H, B, T, seed=3)
        got = []
        with eng.on_stream():
            for i in range(10):
                eng.zero_grads()
                eng.mini_batch(dx, dlen, dlab, 0.8, 0.5, 7 + i, max_len=T)
                if apply:
                    eng.apply(1e-3, 1.0)
                torch.cuda.synchronize()
                eng.check()
                got.append(_bits(eng, L, B, H))
        return got

    def equal(r0, r1):
        return all(np.array_equal(a, b) for s0, s1 in zip(r0, r1) for a, b in zip(s0, s1))

    runs = [ten_steps(False), ten_steps(False)]
    with_apply = [ten_steps(True), ten_steps(True)]
    eng, _p = S.new_engine(L, H, B, T, seed=3)
    pair = []
    with eng.on_stream():
        for _ in range(2):
            eng.zero_grads()
            eng.mini_batch(dx, dlen, dlab, 0.8, 0.5, 7, max_len=T)
            torch.cuda.synchronize()
            eng.check()
            pair.append(_bits(eng, L, B, H))
    twice = all(np.array_equal(a, b) for a, b in zip(*pair))
    return dict(identical=bool(equal(*runs)), steps=len(runs[0]), with_apply_identical=bool(equal(*with_apply)),
                consecutive_identical=bool(twice), plan=plan_numbers(eng._ws, head=eng._head),
                finite=bool(np.isfinite(pair[0][0]).all() and np.isfinite(pair[0][1]).all()))


if __name__ == "__main__":
    mode, dest = sys.argv[1], sys.argv[2]
    result = {"parity": mode_parity, "plans": mode_plans, "repro": mode_repro}[mode]()
    with open(dest, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
