"""The transducer's launches against what they replace, in one process (warm-up and repeats as tools/lookahead_bench.py does them):
event-timed averages of back-to-back calls on one stream after two uncounted ones.  One JSON line; a measurement, not a gate.

    python tools/transducer_bench.py [--repeats 10] [--step-windows 5] [--out profiles/transducer_bench_line.json]

At the workload shape -- the headline model at frame_stack 3 / frame_skip 3: B 32, T 334, U+1 162, J 512, C 80, target lengths
~U[60, 161] -- and at T 1001 (no low frame rate):
  joint_fwd / joint_bwd   against the composition from this project's own kernels on a MATERIALISED z: torch.tanh of the broadcast sum,
                          then ops.linear_fwd / ops.linear_bwd on z [N, J], (1 - z^2), and the two sums.  The composition runs every
                          node; the fused calls run the live ones, so both the time and the fraction of the 157.3 TFLOP/s f32 peak
                          on 2 N_live J C flops (three times that for the backward) are given.
  loss                    against ops.ctc_loss_fwd_bwd at the same T and U.
  greedy                  ms and launches per mini-batch.
  step                    the full transducer optimiser step against the CTC step of the same 3 x 512 encoder (T 334 only).
The kernels' own time per launch comes from a separate run under the profiler (rocprofv3 --kernel-trace --stats -- python
tools/transducer_bench.py --kernels-only)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, U, J, C, L, H, D = 32, 161, 512, 80, 3, 512, 120
PEAK_F32 = 157.3e12


def timed(fn, n):
    fn()
    fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def labels(rng):
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(60, 162)
        dense[b, :n] = rng.randint(1, C - 1, size=n)
        if n < U:
            dense[b, n] = C - 1
    return dense


def kernels(T, repeats, composition=True):
    from rnn_speech_amd import ops
    rng = np.random.RandomState(T)
    dev = "cuda"
    f = torch.randn(T, B, J, device=dev)
    g = torch.randn(U + 1, B, J, device=dev)
    w = torch.randn(J, C, device=dev) / J ** 0.5
    bias = torch.zeros(C, device=dev)
    lengths = torch.as_tensor(rng.randint(T * 3 // 4, T + 1, size=B).astype(np.int32)).cuda()
    dense = torch.as_tensor(labels(rng)).cuda()
    targets, n, tok, tok_len = ops.rnnt_targets(dense, C)
    live = int(((lengths.long()) * (n.long() + 1)).sum())
    N = B * T * (U + 1)
    lat = torch.empty(B, T, U + 1, C, device=dev)
    loss = torch.zeros(B, device=dev)
    ws = ops.rnnt_workspace(T, B, U, J, C, f.device)
    dw, db = torch.zeros_like(w), torch.zeros_like(bias)
    df, dg = torch.empty_like(f), torch.empty_like(g)
    out = {"T": T, "nodes": N, "live_nodes": live, "workspace_mb": round(ws.numel() / 2 ** 20, 1)}
    out["joint_fwd_ms"] = timed(lambda: ops.rnnt_joint_fwd(f, g, w, bias, lengths, n, logits=lat), repeats)
    out["joint_fwd_peak_fraction"] = 2.0 * live * J * C / (out["joint_fwd_ms"] * 1e-3) / PEAK_F32

    # the loss overwrites the logits in place in the product; here it reads a kept copy of them and writes the lattice buffer, so the
    # call is timed alone on the same input every time
    ops.rnnt_joint_fwd(f, g, w, bias, lengths, n, logits=lat)
    kept = lat.clone()
    out["loss_ms"] = timed(lambda: ops.rnnt_loss_fwd_bwd(kept, targets, n, lengths, loss=loss, dlogits=lat, ws=ws), repeats)
    del kept
    out["joint_bwd_ms"] = timed(lambda: ops.rnnt_joint_bwd(lat, f, g, w, lengths, n, dw, db, df=df, dg=dg, ws=ws), repeats)
    out["joint_bwd_peak_fraction"] = 6.0 * live * J * C / (out["joint_bwd_ms"] * 1e-3) / PEAK_F32
    # CTC at the same T and U
    cl = torch.randn(T, B, C, device=dev)
    cws = ops.CtcWorkspace(T, B, C, U, device=dev)
    cd, closs = torch.empty_like(cl), torch.zeros(B, device=dev)
    out["ctc_loss_ms"] = timed(lambda: ops.ctc_loss_fwd_bwd(cl, dense, lengths, ws=cws, loss=closs, dlogits=cd), repeats)
    if composition:
        z = torch.empty(B, T, U + 1, J, device=dev)
        ft, gt = f.transpose(0, 1).unsqueeze(2), g.transpose(0, 1).unsqueeze(1)
        comp = torch.empty(N, C, device=dev)

        def fwd_comp():
            torch.add(ft, gt, out=z)
            torch.tanh(z, out=z)
            ops.linear_fwd(z.view(N, J), w, bias, out=comp)

        out["joint_fwd_composed_ms"] = timed(fwd_comp, max(2, repeats // 3))
        dz = torch.empty(N, J, device=dev)
        dl = lat.view(N, C)

        def bwd_comp():
            ops.linear_bwd(z.view(N, J), w, dl, dw, db, need_dx=True, dx=dz)
            d4 = dz.view(B, T, U + 1, J)
            d4.addcmul_(d4 * z, z, value=-1.0)                 # dz (1 - z^2) with one temporary
            torch.sum(d4, dim=2, out=df.transpose(0, 1))
            torch.sum(d4, dim=1, out=dg.transpose(0, 1))

        out["joint_bwd_composed_ms"] = timed(bwd_comp, max(2, repeats // 3))
        out["z_gb"] = round(N * J * 4 / 2 ** 30, 2)
        del z, dz, comp
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def steps(T, windows, steps_per=5):
    from rnn_speech_amd.engine import Engine
    from rnn_speech_amd.transducer import TransducerEngine
    rng = np.random.RandomState(1)
    x = torch.randn(T, B, D, device="cuda")
    lengths = torch.as_tensor(rng.randint(T * 3 // 4, T + 1, size=B).astype(np.int32)).cuda()
    dense = torch.as_tensor(labels(rng)).cuda()
    ctc = Engine(L, H, D, C, B, T, U)
    rnnt = TransducerEngine(L, H, D, C, B, T, U, joint_size=J, pred_layers=1, pred_hidden=H)

    def step(eng):
        def run():
            with eng.on_stream():
                eng.zero_grads()
                eng.mini_batch(x, lengths, dense, keep_in=0.8, keep_out=0.5, seed=1)
                eng.apply(3e-4, 1.0)
        return run

    res = {"ctc": [], "transducer": []}
    for _ in range(windows + 2):
        for name, eng in (("ctc", ctc), ("transducer", rnnt)):
            res[name].append(timed(step(eng), steps_per))
    ctc.check(); rnnt.check()
    out = {"T": T, "ctc_step_ms": round(float(np.median(res["ctc"][2:])), 3), "transducer_step_ms": round(float(np.median(res["transducer"][2:])), 3)}
    with rnnt.on_stream():
        rnnt.forward(x, lengths)
        out["greedy_ms"] = round(timed(lambda: rnnt.greedy_decode(lengths), 3), 3)
    out["greedy_launches"] = (T + U) * 2 + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step-windows", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    line = {"shape": {"B": B, "U": U, "J": J, "C": C}, "kernels": [kernels(334, a.repeats, not a.kernels_only)]}
    if not a.kernels_only:
        line["kernels"].append(kernels(1001, a.repeats))
        line["step"] = steps(334, a.step_windows)
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
