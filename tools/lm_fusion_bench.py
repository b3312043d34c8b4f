"""First-pass fusion: the step kernel and the fused decoder, measured on one GPU.  One JSON line.  A measurement, not a gate.

  step      amdspeech_lm_step, microseconds per call at N = 1, 32, 256, 3200 rows for a 2 x 256 and a 2 x 512 model, V 80, every row
            from its own parent slot, beside the same step composed from what the library had before it -- embed_fwd, a torch gather
            of the parent rows, amdspeech_gemm_f32 for the gates, torch pointwise gates, linear_fwd, torch log_softmax --
            alternating in one process (windows of --reps calls, median of --windows windows after --warmup).  With each figure
            the bytes of weights a call streams (L * 2H * 4H * 4 + H * V * 4) and its 2 * N * L * 2H * 4H flops.
  decode    one mini-batch of 32 x 1001 frames, C 80, beam width 100, 16 host threads, synthetic peaked posteriors (seeded normal
            logits times 3): NbestRescorer (lm_nbest 16, the n-best pass) against FusedDecoder with the same 2 x 256 model; the
            share of the fused time inside the step callback and the mean rows per step call.

    python tools/lm_fusion_bench.py [--reps 50] [--windows 5] [--warmup 2] [--skip-decode] [--frames 1001]

Kernel times come from a separate run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/lm_fusion_bench.py --steps-only 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V = 80
ROWS = (1, 32, 256, 3200)
MODELS = ((2, 256), (2, 512))


def timed(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps          # microseconds per call


def alternate(pair, reps, windows, warmup):
    us = {k: [] for k in pair}
    for w in range(warmup + windows):
        for k, fn in pair.items():
            t = timed(fn, reps)
            if w >= warmup:
                us[k].append(t)
    return {k: float(np.median(v)) for k, v in us.items()}, {k: [float(np.min(v)), float(np.max(v))] for k, v in us.items()}


def step_setup(L, H, N, seed=0):
    """(fused step, composed step) as closures on one engine's parameters and one state pool: rows 0 .. N-1 step from the slots
    N .. 2N-1 (a permutation) into the slots 0 .. N-1."""
    from rnn_speech_amd import ops
    from rnn_speech_amd.language_model import LmEngine
    eng = LmEngine(L, H, V, 1, 2, seed=1234)
    lay, p = eng.layout, eng.p
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pool_h = torch.randn(2 * N, L, H, device="cuda", generator=gen) * 0.5
    pool_c = torch.randn(2 * N, L, H, device="cuda", generator=gen) * 0.5
    rng = np.random.RandomState(seed)
    parent = torch.as_tensor((N + rng.permutation(N)).astype(np.int32)).cuda()
    token = torch.as_tensor(rng.randint(0, V - 1, size=N).astype(np.int32)).cuda()
    dest = torch.arange(N, dtype=torch.int32, device="cuda")
    logq = torch.empty(N, V, device="cuda")

    def fused():
        ops.lm_step(parent, token, dest, pool_h, pool_c, p("input_w"), p("input_b"), p("kernel_0"), lay.kernel_stride, p("bias_0"),
                    lay.bias_stride, p("output_w"), p("output_b"), logq=logq)

    par64, dst64 = parent.long(), dest.long()
    tok2 = token.view(N, 1).contiguous()
    ones = torch.ones(N, dtype=torch.int32, device="cuda")
    x0 = torch.empty(1, N, H, device="cuda")
    gates = torch.empty(N, 4 * H, device="cuda")
    logits = torch.empty(N, V, device="cuda")
    out = {}

    def composed():
        ops.embed_fwd(tok2, ones, p("input_w"), p("input_b"), x0)
        x = x0.view(N, H)
        for l in range(L):
            a = torch.cat([x, pool_h[par64, l]], dim=1)
            ops.gemm(a, p("kernel_%d" % l), bias=p("bias_%d" % l), out=gates)
            i, j, f, o = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
            c = pool_c[par64, l] * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
            x = (torch.tanh(c) * torch.sigmoid(o)).contiguous()
            pool_c[dst64, l] = c
            pool_h[dst64, l] = x
        ops.linear_fwd(x, p("output_w"), p("output_b"), out=logits)
        out["logq"] = torch.log_softmax(logits, dim=1)

    return fused, composed, logq, out


def bench_steps(a):
    from rnn_speech_amd import ops
    rows = []
    for L, H in MODELS:
        for N in ROWS:
            fused, composed, logq, out = step_setup(L, H, N)
            fused()
            composed()
            torch.cuda.synchronize()
            diff = float((logq - out["logq"]).abs().max().cpu())
            us, span = alternate({"lm_step": fused, "composed": composed}, a.reps, a.windows, a.warmup)
            rows.append({"model": "%dx%d" % (L, H), "N": N, "plan": ops.lm_step_plan(N, L, H, V), "us": us, "us_min_max": span,
                         "weight_bytes": L * 2 * H * 4 * H * 4 + H * V * 4, "flops": 2 * N * L * 2 * H * 4 * H,
                         "max_abs_diff_logq": diff})
    return rows


def bench_decode(a):
    from rnn_speech_amd import ops
    from rnn_speech_amd.language_model import FusedDecoder, LanguageModel, rescore_nbest
    T, B, C, width, threads = a.frames, 32, V, 100, 16
    rng = np.random.RandomState(3)
    lg = (rng.randn(T, B, C) * 3.0).astype(np.float32)
    lengths = np.full(B, T, np.int32)
    model = LanguageModel(2, 256, 64, T, T, C, seed=1234)
    model.create_forward_rnn()
    fused = FusedDecoder(model, 0.5, width, max_threads=threads)

    def rescorer(logits, lens, beam_width, merge):      # NbestRescorer's two steps, the decode capped at the same thread count
        nbest = ops.ctc_beam_search_nbest(logits, lens, 16, beam_width, merge, max_threads=threads)
        return rescore_nbest(*nbest, scorer=model.score, lm_weight=0.5)[:2]

    out = {}
    for name, fn in (("rescore", rescorer), ("fused", fused)):
        times = []
        for _ in range(a.decode_reps + 1):
            if fused.stepper is not None:
                st = fused.stepper
                st.calls, st.rows, st.seconds = 0, 0, 0.0
            t0 = time.perf_counter()
            ids, out_len = fn(lg, lengths, width, True)
            times.append(time.perf_counter() - t0)
        out[name] = {"seconds": float(np.median(times[1:])), "seconds_all": times, "mean_tokens": float(out_len.mean())}
    st = fused.stepper
    out["fused"].update({"callback_seconds": st.seconds, "callback_share": st.seconds / times[-1], "step_calls": st.calls,
                         "mean_rows_per_call": st.rows / max(st.calls, 1)})
    out["shape"] = "%d x %d frames, C %d, width %d, %d threads, 2x256 model, lm_weight 0.5" % (B, T, C, width, threads)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--decode-reps", type=int, default=2)
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--steps-only", type=int, default=0)
    a = ap.parse_args()
    if a.steps_only:
        for L, H in MODELS:
            for N in ROWS:
                fused = step_setup(L, H, N)[0]
                for _ in range(a.steps_only):
                    fused()
        torch.cuda.synchronize()
        print(json.dumps({"steps_only": a.steps_only, "models": MODELS, "rows": ROWS}))
        return
    out = {"step": bench_steps(a), "reps_per_window": a.reps, "windows": a.windows, "warmup_windows": a.warmup}
    if not a.skip_decode:
        out["decode"] = bench_decode(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
