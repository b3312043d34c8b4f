"""Child process of tests/test_gpu_flow_fwd_split.py: AMDSPEECH_FLOW_FWD_WORKERS is read once per process, so every value of the
switch runs here, in a process of its own.  `python flow_fwd_split_child.py <mode> <out.json>` runs one mode on the GPU, compares
with the float64 reference of tests/lstm_stack_ref.py (input and output Linear and the CTC stage of tests/ctc_ref.py around it)
and writes every figure as JSON; the parent asserts.  Nothing here decides a bound: the figures are relative errors
max|got - ref| / max|ref| per tensor (the metric of tests/test_gpu_fullsize.py), the parent holds them to that file's bounds."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctc_ref  # noqa: E402
import lstm_stack_ref as R  # noqa: E402

D, C, U = 40, 80, 161


def make_batch(T, B, seed, lengths):
    """x [T,B,D], dense labels [B,U] (labels 1..C-2, then the end mark C-1; at most T // 2 of them, so every row is feasible)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, D).astype(np.float32)
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = max(1, min(int(lengths[b]) // 2, rng.randint(80, U)))
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    return x, dense


def ragged(T, B, seed):
    """One row of T, one of T - 1, one of 1, one of 0, the rest random (the rule of lstm_stack_ref.make_lengths)."""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, size=B).astype(np.int32)
    for pos, val in ((0, T), (1, T - 1), (2, 1), (3, 0)):
        if pos < B:
            lengths[pos] = max(val, 0)
    return lengths


def reference(p, x, dense, lengths, L):
    """float64: h / c (the state after every frame) [L,T,B,H], gates [L,T,B,4,H], logits, loss, the gradient of sum_b loss_b."""
    p = {k: v.astype(np.float64) for k, v in p.items()}
    T, B, _ = x.shape
    H = p["input_b"].shape[0]
    x64 = x.astype(np.float64)
    z0 = x64 @ p["input_w"] + p["input_b"]
    K = np.stack([p["kernel_%d" % l] for l in range(L)])
    bias = np.stack([p["bias_%d" % l] for l in range(L)])
    res = R.forward(z0, K, bias, lengths)
    ztop = res["ztop"].numpy()
    logits = ztop @ p["output_w"] + p["output_b"]
    loss, dlog = ctc_ref.reference(logits, dense, lengths)
    bw = R.backward(res["cache"], torch.as_tensor((dlog.reshape(T * B, -1) @ p["output_w"].T).reshape(T, B, H)))
    layers = res["cache"]["layers"]
    c = torch.stack([torch.cat([st["cprev"][1:], res["cT"][l][None]]) for l, st in enumerate(layers)])
    gates = torch.stack([torch.stack([st["i"], st["j"], st["f"], st["o"]], dim=2) for st in layers])
    dz0 = bw["dz0"].numpy()
    g = {"output_w": ztop.reshape(T * B, H).T @ dlog.reshape(T * B, -1), "output_b": dlog.reshape(T * B, -1).sum(0),
         "input_w": x64.reshape(T * B, -1).T @ dz0.reshape(T * B, H), "input_b": dz0.reshape(T * B, H).sum(0)}
    for l in range(L):
        g["kernel_%d" % l], g["bias_%d" % l] = bw["dK"][l].numpy(), bw["db"][l].numpy()
    return dict(h=res["h"].numpy(), c=c.numpy(), gates=gates.numpy(), logits=logits, loss=np.asarray(loss), grads=g)


def rel(got, ref, mask=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if mask is not None:
        got, ref = got * mask, ref * mask
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))


def histories(eng, L, B, H):
    """h and c after every frame [L,T,B,H] and the gates [L,T,B,4,H] of the last forward call, from the workspace."""
    from rnn_speech_amd import lib as _l
    ws, T = eng._ws, eng._Tr
    bh = B * H
    out = []
    for which in (_l.WS_HFINAL, _l.WS_CFINAL):
        first = ws._offset(which) - T * bh + bh          # [L][T+1][B][H]: slot t + 1 is the state after frame t
        out.append(torch.as_strided(ws.buf, (L, T, B, H), ((T + 1) * bh, bh, H, 1), first).cpu().numpy())
    gates = torch.as_strided(ws.buf, (L, T, B, 4, H), (T * bh * 4, bh * 4, 4 * H, H, 1), ws._offset(_l.WS_GATES)).cpu().numpy()
    return out[0], out[1], gates


def bit_sums(eng, L, B, H):
    """The h and c histories and the gates of the last forward call as exact integer sums of their bit patterns (1.2 GB per step at
    the headline shape: too much to keep): plain and weighted by position, on the device."""
    from rnn_speech_amd import lib as _l
    ws, T = eng._ws, eng._Tr
    bh = B * H
    out = []
    for which, n in ((_l.WS_HFINAL, (T + 1) * bh * L), (_l.WS_CFINAL, (T + 1) * bh * L), (_l.WS_GATES, L * T * bh * 4)):
        first = ws._offset(which) - (T * bh if which != _l.WS_GATES else 0)
        bits = ws.buf[first:first + n].view(torch.int32)
        weight = (torch.arange(n, device=bits.device, dtype=torch.int32) % 8191) + 1
        out.append(np.asarray([int(torch.sum(bits, dtype=torch.int64)), int(torch.sum(bits * weight, dtype=torch.int64))]))
    return tuple(out)


def new_engine(L, H, B, T, seed=1234):
    from rnn_speech_amd.engine import Engine
    eng = Engine(L, H, D, C, B, T, U, seed=seed)
    rng = np.random.RandomState(3)
    p = eng.to_numpy()
    for k in p:                               # non-zero biases exercise the bias paths (tests/test_gpu_fullsize.py)
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    return eng, p


def plan_of(eng):
    from rnn_speech_amd import ops
    plan = ops.lstm_plan(eng._ws, head=eng._head)
    return dict(fwd_path=plan["fwd_path"], mv=plan["mv"], xw_parts=plan["xw_parts"], nmt=plan["nmt"],
                xw_halves=ops.lstm_plan_xw_halves(eng._ws, head=eng._head), fused_head=eng._head is not None)


def step_and_compare(eng, p, x, dense, lengths, L, B, H, ref=None, max_len=None):
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    with eng.on_stream():
        eng.zero_grads()
        eng.mini_batch(dx, dlen, dlab, max_len=max_len)
    torch.cuda.synchronize()
    eng.check()
    T = eng._Tr
    if ref is None:
        ref = reference(p, x[:T], dense, lengths, L)
    h, c, gates = histories(eng, L, B, H)
    live = (np.arange(T)[:, None] < np.asarray(lengths)[None, :])
    fig = dict(plan=plan_of(eng), T=int(T),
               h=rel(h, ref["h"]), c=rel(c, ref["c"]), gates=rel(gates, ref["gates"], live[None, :, :, None, None]),
               logits=rel(eng.logits.cpu().numpy()[:T], ref["logits"]))
    loss = eng.loss.cpu().numpy().astype(np.float64)
    fig["loss"] = float(np.abs(loss - ref["loss"]).max() / (np.abs(ref["loss"]).max() + 1e-300))
    fig["loss_rows"] = float(np.max(np.abs(loss - ref["loss"]) / (np.abs(ref["loss"]) + 1e-300) * (ref["loss"] != 0)))
    g = eng.to_numpy(eng.grads)
    fig["grads"] = {k: rel(g[k], ref["grads"][k]) for k in ref["grads"]}
    fig["finite"] = bool(np.isfinite(h).all() and np.isfinite(gates).all() and all(np.isfinite(v).all() for v in g.values()))
    return fig, ref


def mode_headline():
    """3x512 / D40 / B32 on ONE engine and workspace: T = 1001 with equal lengths, then a shorter call (301 frames, ragged lengths),
    then T = 1001 again -- the tags of the tile history (full and half tiles) have to survive the shorter call in between."""
    L, H, B, T = 3, 512, 32, 1001
    eng, p = new_engine(L, H, B, T)
    full = np.full(B, T, np.int32)
    x, dense = make_batch(T, B, 0, full)
    out = {}
    out["T1001-equal"], ref_full = step_and_compare(eng, p, x, dense, full, L, B, H)
    short = ragged(301, B, 11)
    _, dense_s = make_batch(T, B, 1, np.maximum(short, 1))
    out["T301-ragged-same-workspace"], _ = step_and_compare(eng, p, x, dense_s, short, L, B, H, max_len=301)
    out["T1001-equal-again"], _ = step_and_compare(eng, p, x, dense, full, L, B, H, ref=ref_full)
    return out


def mode_small():
    """3x512 / B32 at T in {1, 2, 3, 9} (the prologue and the clamped frame indices of both roles), ragged at T = 9; 2x512 / B16;
    and the shapes that must NOT take the half roles: no spare XCD (L x nmt = 8), H < 512, precisions 1 and 2 (plan only)."""
    from rnn_speech_amd import ops
    out = {}
    for T in (1, 2, 3, 9):
        L, H, B = 3, 512, 32
        eng, p = new_engine(L, H, B, T)
        lengths = np.full(B, T, np.int32)
        x, dense = make_batch(T, B, 20 + T, lengths)
        out["3x512-B32-T%d" % T], _ = step_and_compare(eng, p, x, dense, lengths, L, B, H)
        if T == 9:
            lengths = ragged(T, B, 5)
            x, dense = make_batch(T, B, 31, np.maximum(lengths, 1))
            out["3x512-B32-T9-ragged"], _ = step_and_compare(eng, p, x, dense, lengths, L, B, H)
    L, H, B, T = 2, 512, 16, 65
    eng, p = new_engine(L, H, B, T)
    lengths = ragged(T, B, 7)
    x, dense = make_batch(T, B, 41, np.maximum(lengths, 1))
    out["2x512-B16-T65-ragged"], _ = step_and_compare(eng, p, x, dense, lengths, L, B, H)
    plans = {}
    for name, (T, B, H, L, pr) in {"no-spare-xcd": (8, 64, 512, 2, 0), "H256": (16, 32, 256, 3, 0), "H384": (16, 32, 384, 2, 0),
                                   "precision1": (16, 32, 512, 3, 1), "precision2": (16, 32, 512, 3, 2)}.items():
        ws = ops.LstmWorkspace(T, B, H, L, precision=pr)
        plan = ops.lstm_plan(ws)
        plans[name] = dict(fwd_path=plan["fwd_path"], mv=plan["mv"], nmt=plan["nmt"], L=L, xw_halves=ops.lstm_plan_xw_halves(ws))
    out["_plans"] = plans
    return out


def mode_repro():
    """The same 10 steps (cfg2's shape, ragged lengths, dropout on) twice on fresh engines: the forward results repeat bit for bit
    (the gradients are summed with f32 atomics: tests/test_gpu_fullsize.py)."""
    L, H, B, T = 3, 512, 32, 1001
    rng = np.random.RandomState(0)
    lengths = rng.randint(600, T + 1, size=B).astype(np.int32)
    x, dense = make_batch(T, B, 0, lengths)
    dx, dlen, dlab = torch.as_tensor(x).cuda(), torch.as_tensor(lengths).cuda(), torch.as_tensor(dense).cuda()
    runs = []
    for _ in range(2):
        eng, _p = new_engine(L, H, B, T, seed=3)
        got = []
        with eng.on_stream():
            for i in range(10):
                eng.zero_grads()
                eng.mini_batch(dx, dlen, dlab, 0.8, 0.5, 7 + i, max_len=int(lengths.max()))
                torch.cuda.synchronize()
                eng.check()
                got.append((eng.loss.cpu().numpy().copy(), eng.logits.cpu().numpy().copy()) + bit_sums(eng, L, B, H))
        runs.append(got)
        plan = plan_of(eng)
    same = all(np.array_equal(a, b) for s0, s1 in zip(*runs) for a, b in zip(s0, s1))
    return dict(identical=bool(same), plan=plan, steps=len(runs[0]))


if __name__ == "__main__":
    mode, dest = sys.argv[1], sys.argv[2]
    result = {"headline": mode_headline, "small": mode_small, "repro": mode_repro}[mode]()
    with open(dest, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
