"""ms per training step (forward, CTC, backward, clip + Adam) of the two bidirectional forms at one shape each:
bidirectional_mode = layer (stack_bidirectional_dynamic_rnn, amdspeech_lstm_bidir_*) against top (two stacks joined in front of the
output layer).  Exact f32 by default (--precision bf16x3: split-precision MFMA products), synthetic features, every utterance
full length.

    python tools/bidir_layer_bench.py [--steps 10] [--warmup 3] [--shape cfg5|3x512|all] [--mode layer|top|both]
                                      [--precision f32|bf16x3|both]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {      # L, H, D, B, T
    "cfg5": (5, 1024, 120, 64, 998),
    "3x512": (3, 512, 120, 32, 1001),
}


def run(shape, mode, steps, warmup, precision="f32", C=80, U=100):
    from rnn_speech_amd.engine import Engine
    L, H, D, B, T = SHAPES[shape]
    eng = Engine(L, H, D, C, B, T, U, seed=1, bidirectional=True, bidirectional_mode=mode, precision=precision)
    rng = np.random.RandomState(0)
    x = torch.as_tensor(rng.randn(T, B, D).astype(np.float32)).cuda()
    lengths = torch.full((B,), T, dtype=torch.int32).cuda()
    dense = np.zeros((B, U), np.int32)
    dense[:, :U - 1] = rng.randint(1, C - 1, size=(B, U - 1))
    dense[:, U - 1] = C - 1
    dense = torch.as_tensor(dense).cuda()
    times = []
    with eng.on_stream():
        for i in range(warmup + steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.zero_grads()
            eng.mini_batch(x, lengths, dense, max_len=T)
            eng.apply(3e-4, 1.0)
            b.record()
            b.synchronize()
            if i >= warmup:
                times.append(a.elapsed_time(b))
    eng.check()
    path = eng.kernel_path()
    return {"shape": shape, "mode": mode, "L": L, "H": H, "B": B, "T": T, "ms_per_step": float(np.median(times)),
            "ms_min": float(np.min(times)), "steps": steps, "layer_recurrence": path.get("layer_recurrence"), "paired": path["paired"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=sorted(SHAPES) + ["all"])
    ap.add_argument("--mode", default="both", choices=["layer", "top", "both"])
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16x3", "both"])
    a = ap.parse_args()
    shapes = sorted(SHAPES) if a.shape == "all" else [a.shape]
    modes = ["layer", "top"] if a.mode == "both" else [a.mode]
    precisions = ["f32", "bf16x3"] if a.precision == "both" else [a.precision]
    for s in shapes:
        for p in precisions:
            for m in modes:
                r = run(s, m, a.steps, a.warmup, p)
                if a.precision != "f32":      # (the default invocation prints what it always printed)
                    r["precision"] = p
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
