"""Blank-frame skipping (ops.ctc_blank_skip, config key decode_blank_skip), measured on one GPU.  One JSON line.  A measurement, not
a gate.  The posteriors are SYNTHETIC: seeded peaky patterns (tests/blank_skip_ref.peaky_posteriors) with 50 %, 75 % and 90 % of the
frames inside runs of blank frames; nothing here says what a trained model would give, and no error rate is measured.

  kernel    the three launches of one call at [1001, 32, 80] and [998, 64, 80], microseconds per call, beside a device-to-device copy of
            the same [T, B, C] tensor, alternating in one process: windows of --reps calls between device events, the median of
            --windows windows after --warmup.  With each figure the frames kept and the bytes the call moves (the logits read once
            by the row kernel, the kept rows read again and the whole output written by the gather, a flag byte and a source index
            per frame).
  decode    wall time of one mini-batch of 32 x 1001 frames, C 80, beam width 100, 16 host threads, with the skip off and on,
            alternating in one process, the median of --decode-reps runs each after one warm-up: ops.ctc_beam_search, the n-best
            pass with rescoring (lm_nbest 16) and the fused decoder, both with the 2 x 256 model of tools/lm_fusion_bench.py.  On =
            what AcousticModel._decoder_input does: the call, the new lengths to the host, the decoder on compact[:max].  With
            every time the frames handed to the decoder, the device-to-host bytes of its logits and, for the fused decoder, the step
            calls and the rows they carried.

    python tools/blank_skip_bench.py [--reps 50] [--windows 5] [--warmup 2] [--decode-reps 3] [--skip-decode] [--theta 0.95]

Kernel times come from a separate run under the profiler (profiles/blank_skip_kernel_stats.csv):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/blank_skip_bench.py --calls-only 200
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1001, 32, 80), (998, 64, 80))
SHARES = (0.5, 0.75, 0.9)


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


def bench_kernel(a):
    import blank_skip_ref as R
    from rnn_speech_amd import ops
    rows = []
    for T, B, C in SHAPES:
        for share in SHARES:
            x, lengths, _ = R.peaky_posteriors(T, B, C, share, seed=int(100 * share))
            lengths[:] = T
            logits, dlen = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
            out, new_len, src = ops.ctc_blank_skip(logits, dlen, a.theta)
            copy = torch.empty_like(logits)

            def skip():
                ops.ctc_blank_skip(logits, dlen, a.theta, out=out, new_lengths=new_len, src_frame=src)

            def d2d():
                copy.copy_(logits)

            us, span = alternate({"blank_skip": skip, "copy": d2d}, a.reps, a.windows, a.warmup)
            kept = int(new_len.sum().cpu())
            nbytes = T * B * C * 4 + kept * C * 4 + T * B * C * 4 + 2 * T * B + 2 * T * B * 4
            rows.append({"shape": [T, B, C], "blank_share": share, "kept_frames": kept, "kept_share": kept / float(T * B),
                         "longest_row": int(new_len.max().cpu()), "plan": ops.ctc_blank_skip_plan(T, B, C), "us": us, "us_min_max": span,
                         "bytes_moved": nbytes, "copy_bytes": 2 * T * B * C * 4,
                         "gbytes_per_s": {"blank_skip": nbytes / us["blank_skip"] / 1e3, "copy": 2 * T * B * C * 4 / us["copy"] / 1e3}})
    return rows


def bench_decode(a):
    import blank_skip_ref as R
    from rnn_speech_amd import ops
    from rnn_speech_amd.language_model import FusedDecoder, LanguageModel, rescore_nbest
    T, B, C, width, threads = a.frames, 32, 80, 100, 16
    model = LanguageModel(2, 256, 64, T, T, C, seed=1234)
    model.create_forward_rnn()
    fused = FusedDecoder(model, 0.5, width, max_threads=threads)

    def beam(logits, lens):
        return ops.ctc_beam_search(logits, lens, width, True, max_threads=threads)[:2]

    def rescore(logits, lens):
        nbest = ops.ctc_beam_search_nbest(logits, lens, 16, width, True, max_threads=threads)
        return rescore_nbest(*nbest, scorer=model.score, lm_weight=0.5)[:2]

    def fuse(logits, lens):
        return fused(logits, lens, width, True)

    out = {"shape": "%d x %d frames, C %d, width %d, %d threads, 2x256 model, lm_weight 0.5, theta %g" % (B, T, C, width, threads, a.theta),
           "posteriors": "synthetic (seeded peaky patterns)", "rows": []}
    for share in SHARES:
        x, lengths, _ = R.peaky_posteriors(T, B, C, share, seed=int(100 * share))
        logits, dlen = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
        bufs = ops.ctc_blank_skip(logits, dlen, a.theta)

        def off():
            return logits, dlen

        def on():
            compact, new_len, _ = ops.ctc_blank_skip(logits, dlen, a.theta, out=bufs[0], new_lengths=bufs[1], src_frame=bufs[2])
            lens = new_len.cpu()
            return compact[:max(int(lens.max()), 1)], lens

        for name, fn in (("beam", beam), ("rescore", rescore), ("fused", fuse)):
            row = {"decoder": name, "blank_share": share}
            times, answers = {"off": [], "on": []}, {}
            for rep in range(a.decode_reps + 1):
                for key, prep in (("off", off), ("on", on)):
                    if fused.stepper is not None:
                        st = fused.stepper
                        st.calls, st.rows, st.seconds = 0, 0, 0.0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lg, ln = prep()
                    ids, out_len = fn(lg, ln)
                    dt = time.perf_counter() - t0
                    if rep > 0:
                        times[key].append(dt)
                    answers[key] = [list(ids[b, :out_len[b]]) for b in range(B)]
                    row[key] = {"frames_handed": int(lg.shape[0]), "logits_d2h_bytes": int(lg.shape[0]) * B * C * 4}
                    if name == "fused":
                        st = fused.stepper
                        row[key].update({"step_calls": st.calls, "step_rows": st.rows, "callback_seconds": st.seconds})
            for key in ("off", "on"):
                row[key].update({"seconds": float(np.median(times[key])), "seconds_all": times[key]})
            row["speedup"] = row["off"]["seconds"] / row["on"]["seconds"]
            row["same_paths"] = answers["off"] == answers["on"]
            out["rows"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=1001)
    ap.add_argument("--decode-reps", type=int, default=3)
    ap.add_argument("--theta", type=float, default=0.95)
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--calls-only", type=int, default=0)
    a = ap.parse_args()
    if a.calls_only:                                  # for a run under the profiler: nothing but the calls, at the headline shape
        import blank_skip_ref as R
        from rnn_speech_amd import ops
        T, B, C = SHAPES[0]
        x, lengths, _ = R.peaky_posteriors(T, B, C, 0.75, seed=75)
        logits, dlen = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
        bufs = ops.ctc_blank_skip(logits, dlen, a.theta)
        for _ in range(a.calls_only):
            ops.ctc_blank_skip(logits, dlen, a.theta, out=bufs[0], new_lengths=bufs[1], src_frame=bufs[2])
        torch.cuda.synchronize()
        print(json.dumps({"calls_only": a.calls_only, "shape": [T, B, C], "blank_share": 0.75}))
        return
    out = {"kernel": bench_kernel(a), "reps_per_window": a.reps, "windows": a.windows, "warmup_windows": a.warmup}
    if not a.skip_decode:
        out["decode"] = bench_decode(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
