"""ms per optimiser step without and with the front time-frequency convolution at the headline shape: 3 x 512, 40-dim features
(one group of 40 bins), batch 32, 1001 frames, exact f32, dropout keep 0.8 / 0.5, features and labels resident in HBM.  A step is
forward, CTC, backward -> clip + Adam on one stream.  Three settings alternate in one process: `off` (no layer, the default path),
`conv_st1` (32 channels, kernel 11 x 21, stride 1 x 2: what the layer costs at the full frame rate) and `conv_st2` (stride 2 x 2:
what the halved recurrence returns).  A window of --steps steps of each in turn; median of --windows windows after --warmup windows.
One JSON line.  A measurement, not a gate.

    python tools/conv_front_bench.py [--steps 10] [--windows 5] [--warmup 3]

The kernels' own time per launch comes from a separate run under the profiler, which serialises kernels and so says nothing about
the step:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/conv_front_bench.py --kernels-only 20

--kernels-only N: at 1001 x 32 and 998 x 64 frames of fbank shape (3 groups of 40 bins), for (32, 11, 21, 2, 2) and (32, 5, 5, 2, 1),
N forward and N backward calls alone, each beside N calls of the yardstick: the project's own exact-f32 GEMM (ops.gemm) on an
explicitly materialised [T' B F', k_pad] x [k_pad, C] product for the forward pass, and its transposed counterpart
[k_pad, T' B F'] x [T' B F', C] for the weight gradient -- what the layer would cost with the patches already gathered in memory.
The JSON line carries event-timed averages of the calls (back to back, not serialised), their ratio to the yardstick and their
share of the f32 matrix peak (157.3 TFLOP/s) on 2 K C flops per output position, so that each shape's figure can be told apart where
the profiler pools them by kernel name (conv2d_fwd_kernel<NB>, conv2d_dw_kernel<NB>, conv2d_reduce_kernel).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, H, D, C, B, T, U = 3, 512, 40, 80, 32, 1001, 161
KERNEL_SHAPES = ((1001, 32), (998, 64))
KERNEL_LAYERS = ((32, 11, 21, 2, 2), (32, 5, 5, 2, 1))
G, F = 3, 40
PEAK_F32_MATRIX = 157.3e12


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
    out = {"calls": n, "ms": {}, "ratio_to_gemm": {}, "share_of_f32_matrix_peak": {}, "plans": {}}
    for (t, b) in KERNEL_SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn(t, b, G * F, device="cuda", generator=gen)
        lengths = torch.full((b,), t, dtype=torch.int32, device="cuda")
        for (c, kt, kf, st, sf) in KERNEL_LAYERS:
            tag = "%dx%d_%dx%dx%d_s%dx%d" % (t, b, c, kt, kf, st, sf)
            plan = ops.conv2d_plan(t, b, G, F, c, kt, kf, st, sf)
            out["plans"][tag] = plan
            K, k_pad = plan["k"], plan["k_pad"]
            w = torch.randn(K, c, device="cuda", generator=gen) * (1.0 / K ** 0.5)
            bias = torch.zeros(c, device="cuda")
            y, lo = ops.conv2d_fwd(x, w, bias, lengths, G, (kt, kf), (st, sf))
            dy = torch.randn(y.shape, device="cuda", generator=gen)
            dw, db = torch.zeros_like(w), torch.zeros_like(bias)
            ws = ops.Conv2dWorkspace(t, b, G, F, c, kt, kf, st, sf)
            m = plan["t_out"] * b * plan["f_out"]
            flops = 2.0 * K * c * m
            ms = out["ms"]
            ms["fwd_" + tag] = timed(lambda: ops.conv2d_fwd(x, w, bias, lengths, G, (kt, kf), (st, sf), out=y, lengths_out=lo), n)
            ms["bwd_" + tag] = timed(lambda: ops.conv2d_bwd(x, y, dy, lengths, G, (kt, kf), (st, sf), dw, db, ws=ws), n)
            # the yardstick: the patches as a matrix in memory, the project's own GEMM on it
            a = torch.randn(m, k_pad, device="cuda", generator=gen)
            wp = torch.randn(k_pad, c, device="cuda", generator=gen)
            ym, dwp = torch.empty(m, c, device="cuda"), torch.empty(k_pad, c, device="cuda")
            dym = dy.view(m, c)
            ms["gemm_fwd_" + tag] = timed(lambda: ops.gemm(a, wp, out=ym), n)
            ms["gemm_dw_" + tag] = timed(lambda: ops.gemm(a, dym, trans_a=True, out=dwp), n)
            del a
            out["ratio_to_gemm"]["fwd_" + tag] = ms["fwd_" + tag] / ms["gemm_fwd_" + tag]
            out["ratio_to_gemm"]["bwd_" + tag] = ms["bwd_" + tag] / ms["gemm_dw_" + tag]
            for k in ("fwd_", "bwd_", "gemm_fwd_", "gemm_dw_"):
                out["share_of_f32_matrix_peak"][k + tag] = flops / (ms[k + tag] * 1e-3) / PEAK_F32_MATRIX
    torch.cuda.synchronize()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", type=int, default=0)
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.kernels_only)
    from rnn_speech_amd.engine import Engine

    rng = np.random.RandomState(100)
    x = torch.from_numpy(rng.randn(T, B, D).astype(np.float32)).cuda()
    lengths = torch.full((B,), T, dtype=torch.int32).cuda()
    dlab = torch.from_numpy(synth_labels(rng)).cuda()
    engines = {"off": Engine(L, H, D, C, B, T, U, seed=1234),
               "conv_st1": Engine(L, H, D, C, B, T, U, seed=1234, conv=(32, 11, 21, 1, 2, 1)),
               "conv_st2": Engine(L, H, D, C, B, T, U, seed=1234, conv=(32, 11, 21, 2, 2, 1))}
    modes = tuple(engines)
    torch.cuda.synchronize()
    torch.cuda.set_stream(engines["off"].stream)          # a real (non-NULL) stream for the whole job (Engine.on_stream)
    paths = {}

    def step(mode, i):
        eng = engines[mode]
        eng.zero_grads()
        eng.mini_batch(x, lengths, dlab, 0.8, 0.5, seed=i + 1)
        eng.apply(3e-4, 1.0)
        paths[mode] = eng.kernel_path()

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
    for eng in engines.values():
        eng.check()
        loss = eng.loss.cpu().numpy()
        assert np.isfinite(loss).all() and (loss > 0).all()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"shape": "%dx%d, %d-dim, batch %d, %d frames, f32, dropout 0.8/0.5; conv 32 x 11 x 21, frequency stride 2" % (L, H, D, B, T),
           "ms_per_step": med, "ms_per_step_min_max": {k: [float(np.min(v)), float(np.max(v))] for k, v in ms.items()},
           "kernel_path": paths, "ratio_to_off": {k: med[k] / med["off"] for k in modes[1:]}, "steps_per_window": a.steps,
           "windows": a.windows, "warmup_windows": a.warmup}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
