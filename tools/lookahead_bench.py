"""ms per optimiser step without and with the lookahead convolution at the headline shape: 3 x 512, 40-dim features, batch 32, 1001
frames, exact f32, dropout keep 0.8 / 0.5, features and labels resident in HBM.  A step is forward, CTC, backward -> clip + Adam on
one stream.  Three settings alternate in one process: `off` (context 0, the default path with the fused CTC head), `off_unfused`
(context 0 with the CTC stage as launches of its own -- what AMDSPEECH_FUSED_CTC=0 selects and what the layer forces, so the fair
parent of the third) and `context_N` (--context, default 20).  A window of --steps steps of each in turn; median of --windows windows
after --warmup windows.  One JSON line.  A measurement, not a gate.

    python tools/lookahead_bench.py [--context 20] [--steps 10] [--windows 5] [--warmup 3]

The kernels' own time per launch comes from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lookahead_bench.py --kernels-only 50

--kernels-only N: at 1001 x 32 x 512 and 998 x 64 x 1024, for context 5, 20 and 32, N forward and N backward calls alone, each beside
N plain device-to-device copies of one [T,B,H] tensor (x -> y: the yardstick of the forward pass, which reads x and writes y once;
the backward pass moves four such tensors at best).  The copies of a shape are `copy_TxBxH` in the JSON line; in OUT's
kernel_stats.csv they are the runtime's copy kernel, the walks are lookahead_conv_kernel<V, 1> (forward), <V, -1> (dx),
lookahead_dw_kernel and lookahead_dw_reduce_kernel.  The JSON line also carries event-timed averages of the same calls (back to
back, not serialised), so that each shape's and context's figure can be told apart where the profiler pools them by kernel name.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, C, B, T, U = 3, 512, 40, 80, 32, 1001, 161
KERNEL_SHAPES = ((1001, 32, 512), (998, 64, 1024))
KERNEL_CONTEXTS = (5, 20, 32)


def synth_labels(rng):
    """80 .. 160 tokens and an EOS per utterance, as bench.py draws them."""
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(80, 161)
        dense[b, :n - 1] = rng.randint(1, C - 1, size=n - 1)
        dense[b, n - 1] = C - 1
    return dense


def timed(fn, n):
    """Average ms of n back-to-back calls of fn on the current stream (after two calls that are not counted)."""
    fn()
    fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def kernels_only(n):
    from rnn_speech_amd import ops
    out = {"calls": n, "ms": {}, "plans": {}}
    for (t, b, h) in KERNEL_SHAPES:
        tag = "%dx%dx%d" % (t, b, h)
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(t, b, h, device="cuda", generator=gen)
        dy = torch.randn(t, b, h, device="cuda", generator=gen)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        lengths = torch.full((b,), t, dtype=torch.int32, device="cuda")
        out["ms"]["copy_" + tag] = timed(lambda: y.copy_(x), n)
        for context in KERNEL_CONTEXTS:
            w = torch.randn(context + 1, h, device="cuda", generator=gen)
            dw = torch.zeros_like(w)
            ws = ops.LookaheadWorkspace(t, b, h, context)
            out["plans"]["%s_c%d" % (tag, context)] = ops.lookahead_plan(t, b, h, context)
            out["ms"]["fwd_%s_c%d" % (tag, context)] = timed(lambda: ops.lookahead_fwd(x, w, lengths, out=y), n)
            out["ms"]["bwd_%s_c%d" % (tag, context)] = timed(lambda: ops.lookahead_bwd(x, w, dy, lengths, dx=dx, dw=dw, ws=ws), n)
    torch.cuda.synchronize()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--context", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=0)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.kernels_only)
    from rnn_speech_amd import engine
    from rnn_speech_amd.engine import Engine

    rng = np.random.RandomState(100)
    x = torch.from_numpy(rng.randn(T, B, D).astype(np.float32)).cuda()
    lengths = torch.full((B,), T, dtype=torch.int32).cuda()
    dlab = torch.from_numpy(synth_labels(rng)).cuda()
    name = "context_%d" % a.context
    engines = {"off": Engine(L, H, D, C, B, T, U, seed=1234)}
    engines["off_unfused"] = engines["off"]
    engines[name] = Engine(L, H, D, C, B, T, U, seed=1234, lookahead=a.context)
    modes = ("off", "off_unfused", name)
    torch.cuda.synchronize()
    torch.cuda.set_stream(engines["off"].stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    fused_default = engine._FUSED_CTC
    heads = {}

    def step(mode, i):
        eng = engines[mode]
        engine._FUSED_CTC = fused_default and mode != "off_unfused"      # (the host decision AMDSPEECH_FUSED_CTC=0 makes)
        eng.zero_grads()
        eng.mini_batch(x, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)
        heads[mode] = eng.kernel_path()["fused_ctc_head"]

    def window(mode, w):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.steps):
            step(mode, w * a.steps + i)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / a.steps

    ms = {mode: [] for mode in modes}
    for w in range(a.warmup + a.windows):
        for mode in modes:
            t = window(mode, w)
            if w >= a.warmup:
                ms[mode].append(t)
    engine._FUSED_CTC = fused_default
    for eng in (engines["off"], engines[name]):
        eng.check()
        loss = eng.loss.cpu().numpy()
        assert np.isfinite(loss).all() and (loss > 0).all()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"shape": "%dx%d, %d-dim, batch %d, %d frames, f32, dropout 0.8/0.5" % (L, H, D, B, T),
           "ms_per_step": med, "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "fused_ctc_head": heads, "ratio_to_off": {k: med[k] / med["off"] for k in modes[1:]},
           "ratio_to_off_unfused": med[name] / med["off_unfused"], "steps_per_window": a.steps, "windows": a.windows,
           "warmup_windows": a.warmup}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
