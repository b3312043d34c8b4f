"""The long-recording kernels (csrc/vad.hip) at the two shapes that matter, and the --file path on a ten-minute recording.  A
measurement, not a gate; every mode prints one JSON line.

    python tools/vad_bench.py --kernels 50
        B = 1 x one hour of 16 kHz and B = 32 x 10 s of 22.05 kHz, synthetic, resident in HBM: N calls each of vad_energy, vad_flags
        (vad_select_kernel + vad_flags_kernel) and gather_spans, timed with device events around the N calls, and the bytes each
        kernel has to move, from the shapes:
            vad_energy_kernel    4 per sample read once + 4 per frame written        (1 / 63 of the samples is read twice: not counted)
            vad_select_kernel    4 passes x 4 per frame read + 12 per row written
            vad_flags_kernel     3 passes x 4 per frame read + 4 per frame written and read back (workspace) + 1 per frame written
            gather_spans_kernel  4 per word gathered read + 4 per word of the [S, w_out] block written
        energy_share_of_hbm = bytes / time / 6.3e12 (the achievable HBM figure of the MI355X).  The one-hour row (230 MB) fits the
        256 MiB Infinity Cache: calls after the first may be served on-die, which the figure then says.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/vad_bench.py --kernels 50
        the time per launch of each kernel, in a run of its own (OUT's kernel_stats.csv); tracing slows the host, the event times of
        that run mean nothing.
    python tools/vad_bench.py --file-minutes 10
        wall time of what `stt.py --file` does with long_audio : segment on a synthetic recording of bursts and pauses, with the
        headline 3 x 512 model (untrained: the times do not depend on the weights, the beam's time does on how peaked the
        logits are -- an untrained model is the beam's expensive case), split into decode / detection and planning / gather and
        features / forward / beam decoding, each ended by a device synchronise, and as a fraction of the audio's duration.  The
        forward share is a process_input call with the greedy device decoder, the beam's share the difference to the same call
        with the host beam decoder.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12
SHAPES = {"hour_16k": (1, 3600 * 16000, 160), "batch32_22k": (32, 10 * 22050, 220)}


def synth_rows(B, n, rate, seed=0):
    """Bursts of tone and noise between pauses 40 dB down, on the device: [B, n] float32."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / rate
    rows = []
    for b in range(B):
        gate = (torch.sin(2 * np.pi * t / (2.3 + 0.1 * b)) > -0.2).float()
        rows.append((0.1 * torch.sin(2 * np.pi * (220.0 + 10 * b) * t) + 0.03 * torch.randn(n, device="cuda", generator=g)) * (0.01 + 0.99 * gate))
    return torch.stack(rows).contiguous()


def timed(calls, fn):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / calls


def kernels(calls):
    from rnn_speech_amd import ops, segmenter
    out = {}
    for name, (B, n, hop) in SHAPES.items():
        rate = hop * 100 if hop != 220 else 22050
        pcm = synth_rows(B, n, rate)
        lengths = [n] * B
        plan = ops.vad_plan(B, n, hop)
        F = plan["f_max"]
        energy = ops.vad_energy(pcm, lengths, hop)
        speech, stats = ops.vad_flags(energy, [F] * B)
        budget = segmenter.frame_budget(rate, hop, rate, "mfcc", 1001)
        spans = []
        for b in range(B):
            spans += [(b,) + sp[:2] for sp in segmenter.plan_spans(speech[b].cpu().numpy(), energy[b].cpu().numpy(), n, hop, budget, 10)]
        rows, starts, counts = ([sp[i] for sp in spans] for i in range(3))
        width = max(counts + [1])
        block = torch.empty(len(spans), width, device="cuda")
        t_energy = timed(calls, lambda: ops.vad_energy(pcm, lengths, hop, out=energy))
        t_flags = timed(calls, lambda: ops.vad_flags(energy, [F] * B, speech=speech, stats=stats))
        t_gather = timed(calls, lambda: ops.gather_spans(pcm, lengths, rows, starts, counts, width, out=block))
        bytes_energy = 4 * B * n + 4 * B * F
        out[name] = {"B": B, "samples_per_row": n, "hop": hop, "plan": plan, "spans": len(spans), "span_width": width,
                     "bytes": {"vad_energy_kernel": bytes_energy, "vad_select_kernel": 16 * B * F + 12 * B,
                               "vad_flags_kernel": (12 + 8 + 1) * B * F, "gather_spans_kernel": 4 * sum(counts) + 4 * len(spans) * width},
                     "event_seconds_per_call": {"vad_energy": t_energy, "vad_flags(select+flags)": t_flags, "gather_spans": t_gather},
                     "energy_bytes_per_second": bytes_energy / t_energy, "energy_share_of_hbm": bytes_energy / t_energy / HBM_ACHIEVABLE,
                     "speech_share": float(speech.float().mean())}
    print(json.dumps({"calls": calls, "hbm_achievable_bytes_per_second": HBM_ACHIEVABLE, "shapes": out}))


def file_path(minutes):
    import stt
    from models.SpeechRecognizer import SpeechRecognizer
    from rnn_speech_amd import hyperparams, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sr, n = 16000, int(minutes * 60 * 16000)
    sig = synth_rows(1, n, sr, seed=1)[0].cpu().numpy()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "long.wav")
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())
        src = open(os.path.join(root, "config.ini")).read()
        src = src.replace("checkpoint_dir : data/checkpoints/", "checkpoint_dir : %s/ckpt" % d).replace("sample_rate : 22050", "sample_rate : 16000")
        src = src.replace("long_audio : truncate", "long_audio : segment")
        cfg = os.path.join(d, "config.ini")
        with open(cfg, "w") as fh:
            fh.write(src)
        hp = hyperparams.HyperParameterHandler(cfg).get_hyper_params()
        ap = stt.build_audio_processor(hp)
        reco = SpeechRecognizer(hp["language"])
        hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            return got, time.perf_counter() - t0

        vad = {name: hp["vad_" + name] for name in stt._VAD_OPTIONS}
        ap.segment(sig[:sr * 30], sr, **vad)                               # warm-up: code objects, pinned block, workspaces
        (signal, got_sr), t_decode = clock(lambda: ops.audio_decode(path))
        seg, t_detect = clock(lambda: ap.segment(signal, got_sr, **vad))
        B = min(hp["batch_size"], len(seg.spans))
        model = stt._forward_model(hp, B)
        T = ap.out_seq_length
        t_features = t_forward = t_beam = 0.0
        batches = [seg.spans[i:i + B] for i in range(0, len(seg.spans), B)]
        for k, part in enumerate(batches[:1] + batches):                   # the first batch twice: once as warm-up
            (feat, lengths), tf = clock(lambda: ap.process_segments(seg.pcm, seg.n, seg.sr, part, rows=B))
            lens = [min(v, T) for v in lengths]
            model.decoder = "greedy"                                       # forward pass and the best path on the device ...
            _, tg = clock(lambda: model.process_input(None, feat, lens))
            model.decoder = "beam"                                         # ... against the same forward pass and the host beam
            _, tb = clock(lambda: model.process_input(None, feat, lens))
            if k:
                t_features, t_forward, t_beam = t_features + tf, t_forward + tg, t_beam + max(tb - tg, 0.0)
        model.close()
        total = t_decode + t_detect + t_features + t_forward + t_beam
        audio = n / float(sr)
        print(json.dumps({"audio_seconds": audio, "spans": len(seg.spans), "batches": len(batches), "batch_rows": B,
                          "seconds": {"decode": t_decode, "detection_and_planning": t_detect, "gather_and_features": t_features,
                                      "forward_with_greedy_decode": t_forward, "beam_decoding": t_beam, "total": total},
                          "fraction_of_audio": total / audio, "stats_db": seg.stats}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--file-minutes", type=float, default=0.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vad_bench.py measures on the GPU: no device found")
    if a.kernels:
        kernels(a.kernels)
    if a.file_minutes:
        file_path(a.file_minutes)


if __name__ == "__main__":
    main()
