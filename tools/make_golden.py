#!/usr/bin/env python3
"""Generate tests/golden/* by IMPORTING the reference (only possible in the build
container, where /root/reference exists).  The reference itself never travels:
only inputs + expected outputs are committed.

What can be imported: the label codec, the fbank numpy body (with
a stub `librosa` whose `feature.delta` follows librosa>=0.6 semantics), the
WER/CER static methods (with a stub `tensorflow`), and the config reader.
TensorFlow and librosa themselves are absent, so LSTM/CTC/MFCC have no
reference-generated vectors ("parity unpinned" -- see oracle/*.py headers).

Usage:  python tools/make_golden.py
        python tools/make_golden.py --checkpoints <checkout of 9bbf15b>     (checkpoint_*.npz only; needs no reference)
        AMDSPEECH_LIB=<libamdspeech.so of the parent commit> python tools/make_golden.py --gemm-plans     (gemm_plans.npz only; no reference, no GPU)
        python tools/make_golden.py --engine-calls     (engine_calls.json only; on the MI355X, from the engine of the parent commit; no reference)
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import scipy.signal

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def _stub_modules():
    librosa = types.ModuleType("librosa")
    feature = types.ModuleType("librosa.feature")

    def delta(data, width=9, order=1, axis=-1, mode="interp"):
        return scipy.signal.savgol_filter(data, width, deriv=order, axis=axis, mode=mode,
                                          polyorder=order)
    feature.delta = delta
    librosa.feature = feature
    sys.modules["librosa"] = librosa
    sys.modules["librosa.feature"] = feature
    sys.modules["mutagen"] = types.ModuleType("mutagen")
    tf = types.ModuleType("tensorflow")
    tfp = types.ModuleType("tensorflow.python")
    tfc = types.ModuleType("tensorflow.python.client")
    tfc.timeline = types.ModuleType("tensorflow.python.client.timeline")
    sys.modules.update({"tensorflow": tf, "tensorflow.python": tfp,
                        "tensorflow.python.client": tfc,
                        "tensorflow.python.client.timeline": tfc.timeline})


def synth_signal(seed, n, sr):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / float(sr)
    sig = 0.1 * rng.randn(n)
    for f0, a in ((220.0, 0.3), (1330.0, 0.2), (3100.0, 0.1)):
        sig += a * np.sin(2 * np.pi * f0 * (1 + 0.1 * seed) * t)
    return sig.astype(np.float32)


def main():
    warnings.simplefilter("ignore")
    os.makedirs(OUT, exist_ok=True)
    _stub_modules()
    sys.path.insert(0, REF)
    from util.dataprocessor import DataProcessor
    from models.SpeechRecognizer import ENGLISH_CHAR_MAP
    from util.audioprocessor import AudioProcessor
    from models.AcousticModel import AcousticModel
    from util.hyperparams import HyperParameterHandler  # noqa: F401

    # ---- label codec --------------------------------------------------------
    texts = ["What ! I'm not looking for... I'll do it...", "it'll", "'d", "the brown lazy fox",
             "northanger abbey", "She's the boss' daughter, isn't she?", "o'clock  well-being",
             "aardvark bookkeeper success mississippi", "we've they'll i'm don't", "", "a",
             "hello world 42 times", "x_y-z: ok!"]
    enc = []
    for txt in texts:
        cleaned = DataProcessor.clean_label(txt)
        ids = DataProcessor.get_str_labels(ENGLISH_CHAR_MAP, cleaned)
        ids_noeos = DataProcessor.get_str_labels(ENGLISH_CHAR_MAP, cleaned, add_eos=False)
        back = DataProcessor.get_labels_str(ENGLISH_CHAR_MAP, ids)
        enc.append({"text": txt, "cleaned": cleaned, "ids": ids, "ids_noeos": ids_noeos,
                    "decoded": back})
    rng = np.random.RandomState(7)
    dec = []
    for _ in range(12):
        ids = [int(v) for v in rng.randint(-2, 83, size=rng.randint(0, 30))]
        dec.append({"ids": ids, "decoded": DataProcessor.get_labels_str(ENGLISH_CHAR_MAP, ids)})
    with open(os.path.join(OUT, "labels.json"), "w") as f:
        json.dump({"char_map": list(ENGLISH_CHAR_MAP), "encode": enc, "decode": dec}, f, indent=1)

    # ---- fbank (reference numpy body) --------------------------------------
    for tag, sr, n in (("16k", 16000, 16000 + 123), ("22k", 22050, 22050 + 77), ("8k", 8000, 6000)):
        sig = synth_signal(3, n, sr)
        ap = AudioProcessor(10 ** 6, "fbank")
        feat, length = ap.process_signal(sig, sr)
        np.savez_compressed(os.path.join(OUT, "fbank_%s.npz" % tag), sig=sig, sr=np.int64(sr),
                            feat=np.asarray(feat, np.float64), length=np.int64(length))
    # truncation contract: features cut to max_input_seq_length, length is not
    ap = AudioProcessor(50, "fbank")
    sig = synth_signal(5, 16000, 16000)
    feat, length = ap.process_signal(sig, 16000)
    np.savez_compressed(os.path.join(OUT, "fbank_trunc.npz"), sig=sig, sr=np.int64(16000),
                        feat=np.asarray(feat, np.float64), length=np.int64(length),
                        max_len=np.int64(50))

    # ---- WER / CER -----------------------------------------------------------
    pairs = [("who is there", "is there"), ("who is there", ""), ("", "who is there"),
             ("who is there", "whois there"), ("who is there", "who i thre"),
             ("it now contained only shanetoclare his two wides and a solitary chicken",
              "it now contained only chanticleer his two wives and a solitary chicken"),
             ("a b c d e f", "a x c d f g h"), ("same same", "same same")]
    wc = [{"a": a, "b": b, "wer": int(AcousticModel.calculate_wer(a, b)),
           "cer": int(AcousticModel.calculate_cer(a, b))} for a, b in pairs]
    with open(os.path.join(OUT, "wer_cer.json"), "w") as f:
        json.dump(wc, f, indent=1)

    # ---- config reader -------------------------------------------------------
    import configparser
    cp = configparser.ConfigParser()
    cp.read(os.path.join(REF, "config.ini"))
    ini = {s: dict(cp.items(s)) for s in cp.sections()}
    with open(os.path.join(OUT, "config_ini.json"), "w") as f:
        json.dump(ini, f, indent=1, sort_keys=True)
    print("golden fixtures written to", OUT)


def corpus_walk_golden():
    """The reference's own DataProcessor (util/dataprocessor.py) over the synthetic trees of
    tests/corpus_fixture.py.  `mutagen` is absent, so File(path).info.length is stubbed with a header read
    (that pins listing, cleaning, type probing and filtering -- not the durations themselves); `sox` is absent,
    so the TED-LIUM segment wavs are pre-cut."""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(OUT)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    import corpus_fixture
    from rnn_speech_amd.corpus import audio_duration

    class _Info(object):
        def __init__(self, n):
            self.length = n

    class _File(object):
        def __init__(self, path):
            self.info = _Info(audio_duration(path))
    sys.modules["mutagen"].File = _File
    sys.path.insert(0, REF)
    from util import dataprocessor as ref_dp
    root = tempfile.mkdtemp()
    try:
        dirs, _ = corpus_fixture.build_trees(root, ted_segments=True)
        out = {"types": {os.path.basename(d): ref_dp.DataProcessor.get_type(d) for d in dirs}, "datasets": {}}
        for d in dirs + [",".join(dirs)]:
            data = ref_dp.DataProcessor(d).get_dataset()
            key = ",".join(os.path.basename(x) for x in d.split(","))
            out["datasets"][key] = sorted([os.path.relpath(os.path.normpath(a), root), t, round(float(n), 6)]
                                          for a, t, n in data)
    finally:
        shutil.rmtree(root)
    with open(os.path.join(OUT, "corpus_walk.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("corpus_walk.json:", {k: len(v) for k, v in out["datasets"].items()})


def checkpoint_goldens(root):
    """tests/golden/checkpoint_{acoustic,language}.npz: the native checkpoints as the code in `root` writes them.  `root` is a
    checkout of commit 9bbf15b, the last one whose two models packed their checkpoints themselves (git worktree add <dir> 9bbf15b)
    -- never the tree under test: tests/test_cpu_checkpoint.py holds the current save() against these files.  Both models run on
    CPU buffers (the acoustic one on tests/dp_oracle_engine.py, the language one on the host methods of its engine)."""
    import shutil
    import tempfile
    import torch
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from dp_oracle_engine import OracleAcousticModel
    from rnn_speech_amd import language_model as lm
    from rnn_speech_amd.engine import ParamLayout

    class CpuLmEngine(object):
        to_numpy, load_numpy = lm.LmEngine.to_numpy, lm.LmEngine.load_numpy

        def __init__(self, L, H, V):
            self.L, self.H, self.V, self.layout, self.adam_step = L, H, V, ParamLayout(L, H, V, V), 0
            self.params, self.grads, self.adam_m, self.adam_v = (torch.zeros(self.layout.total) for _ in range(4))

    class CpuLanguageModel(lm.LanguageModel):
        def _create(self):
            self.engine, self.rnn_created = CpuLmEngine(self.num_layers, self.hidden_size, self.num_labels), True

    def fill(model, seed, step, adam_step, rate):
        rng, eng = np.random.RandomState(seed), model.engine
        for flat, sign in ((eng.params, -0.5), (eng.adam_m, -0.5), (eng.adam_v, 0.0)):      # (per tensor: the pads stay zero)
            eng.load_numpy({k: (rng.rand(*s) + sign + 1e-3).astype(np.float32) for k, (_, s) in eng.layout.slots.items()}, flat=flat)
        eng.adam_step, model.global_step.value = adam_step, step
        model.set_learning_rate(None, rate)
        return rng

    tmp = tempfile.mkdtemp()
    am = OracleAcousticModel(2, 8, 2, 10, 4, 5, False, 80)
    am.create_training_rnn(1.0, 1.0, 1.0, 1e-3, 0.5)
    rng = fill(am, 21, step=42, adam_step=17, rate=3.25e-4)
    am.engine.state_h.copy_(torch.as_tensor(rng.randn(2, 2, 8).astype(np.float32)))
    am.engine.state_c.copy_(torch.as_tensor(rng.randn(2, 2, 8).astype(np.float32)))
    am.save(None, tmp)
    shutil.copyfile(os.path.join(tmp, "acousticmodel.ckpt-42.npz"), os.path.join(OUT, "checkpoint_acoustic.npz"))
    language = CpuLanguageModel(1, 8, 2, 6, 6, 80)
    language.create_training_rnn(1.0, 1.0, 1.0, 1e-3, 0.5)
    fill(language, 22, step=9, adam_step=5, rate=7.5e-4)
    language.save(None, tmp)
    shutil.copyfile(language.checkpoint_path(tmp), os.path.join(OUT, "checkpoint_language.npz"))
    shutil.rmtree(tmp)
    for name in ("checkpoint_acoustic.npz", "checkpoint_language.npz"):
        print(name, len(np.load(os.path.join(OUT, name)).files), "keys")


def gemm_plan_sweep():
    """The rows of tests/golden/gemm_plans.npz (tests/gemm_ref.py: SWEEP_COLUMNS).  Every K; of the 14 x 14 (M, N) pairs the diagonal and
    every pair with (i + 2 j) % 7 == 0 (the full grid is ~1.2 M calls: past the size a committed file may have) -- every value still
    stands on both axes; every call option; the plain placement and one of the six others in turn.  The case table of gemm_ref goes in
    whole, so that no (family, variant) it names can be thinned away."""
    import gemm_ref as R
    MN = (1, 2, 40, 80, 96, 97, 124, 127, 128, 129, 256, 512, 1024, 4096)
    KS = (1, 16, 31, 32, 64, 80, 255, 256, 1024, 2048, 4095, 4096, 19860, 32032, 63872)
    # (pad of lda, ldb, ldc; element offset of A, B, C): ld = cols / cols + 1 / cols + 4, an address aligned to 16 / to 4 only
    PLACES = ((0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (4, 4, 4, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 1, 0),
              (0, 0, 1, 0, 0, 1))
    rows, turn = [R.sweep_row(c) for c in R.CASES if c["entry"] not in R.UNPLANNED], 0
    for i, M in enumerate(MN):
        for j, N in enumerate(MN):
            if i != j and (i + 2 * j) % 7 != 0:
                continue
            for K in KS:
                for ta in (0, 1):
                    for tb in (0, 1):
                        cols = (M if ta else K, K if tb else N, N)
                        options = [(p, bias, acc, 0, 1) for p in (0, 1, 2) for bias in (0, 1) for acc in (0, 1)]
                        if not tb:      # fused column sums: exact f32, B stored [K][N]
                            options += [(0, bias, acc, 1, 1) for bias in (0, 1) for acc in (0, 1)]
                        if ta and not tb:      # the grouped entry
                            options += [(0, 0, acc, 0, count) for acc in (0, 1) for count in (2, 10)]
                        for precision, bias, acc, colsum, count in options:
                            turn += 1
                            for place in (PLACES[0], PLACES[1 + turn % 6]):
                                ld = tuple(c + p for c, p in zip(cols, place[:3]))
                                rows.append((R.SWEEP_GEMM, precision, ta, tb, M, N, K) + ld + place[3:] + (bias, acc, colsum, count))
                        for pad in (0, 1, 4):
                            rows.append((R.SWEEP_PACKED, 2, ta, tb, M, N, K, cols[0] + pad, cols[1] + pad, N, 0, 0, 0, 0, 0, 0, 1))
    return np.asarray(rows, np.int32)


def gemm_plan_goldens(child_out=None):
    """tests/golden/gemm_plans.npz: what ops.gemm_plan / ops.gemm_bf16_packed_plan answer over gemm_plan_sweep(), with the switches at
    their defaults (in this process) and with AMDSPEECH_GEMM_DIRECT=0 AMDSPEECH_GEMM_KC_DIRECT=0 (read once per process: a child).
    Needs no GPU -- the query dereferences nothing -- and no reference.  Run it on the build of the commit BEFORE a change of the
    planning code (AMDSPEECH_LIB=<that build's libamdspeech.so>), never on the tree under test."""
    import subprocess
    import tempfile
    root = os.path.dirname(OUT)
    sys.path[:0] = [os.path.dirname(root), root]
    import gemm_ref as R
    from rnn_speech_amd import lib, ops
    fields = [n for n, _ in lib.GemmPlanInfo._fields_]
    calls, messages = gemm_plan_sweep(), []
    plans, status = R.sweep_answers(ops, calls, fields, messages)
    if child_out is not None:      # (the child: its answers and message classes go back through a file)
        np.savez(child_out, plans=plans, status=status, messages=np.asarray(messages, dtype=str))
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fallback.npz")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--gemm-plans-child", path], env=dict(os.environ, **R.FALLBACK_ENV))
        child = np.load(path)
        child_messages = [str(m) for m in child["messages"]]
        for m in child_messages:
            if m not in messages:
                messages.append(m)
        fb_status = np.asarray([-1 if s < 0 else messages.index(child_messages[s]) for s in child["status"]], np.int32)
        fb_plans = child["plans"]
    np.savez_compressed(os.path.join(OUT, R.SWEEP_FILE), columns=np.asarray(R.SWEEP_COLUMNS, dtype=str), fields=np.asarray(fields, dtype=str),
                        families=np.asarray(lib.GEMM_FAMILIES, dtype=str), messages=np.asarray(messages, dtype=str), calls=calls,
                        plans_default=plans, status_default=status, plans_fallback=fb_plans, status_fallback=fb_status)
    seen = sorted({(lib.GEMM_FAMILIES[f], int(v)) for f, v in plans[status < 0][:, :2]})
    print(R.SWEEP_FILE, len(calls), "calls,", int((status >= 0).sum()), "refused,", os.path.getsize(os.path.join(OUT, R.SWEEP_FILE)), "bytes")
    print("message classes:", messages)
    print("variants:", seen)


def engine_call_goldens(out_path=None):
    """tests/golden/engine_calls.json: what tests/engine_calls.py records for every configuration of its CONFIGS, one line per entry.
    Needs the MI355X and no reference.  Run it on the engine.py / language_model.py / ops.py of the commit BEFORE a change of the
    engine's structure, never on the tree under test: tests/test_gpu_engine_calls.py holds the current engine against this file."""
    root = os.path.dirname(OUT)
    sys.path[:0] = [os.path.dirname(root), root]
    import engine_calls
    recorded = {}
    for name in engine_calls.CONFIGS:
        recorded[name] = engine_calls.record(name)
        print(name, len(recorded[name]), "entries", flush=True)
    path = out_path or os.path.join(OUT, "engine_calls.json")
    engine_calls.dump(recorded, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if "--engine-calls" in sys.argv:      # python tools/make_golden.py --engine-calls [file]     (on the MI355X, at the parent commit's engine)
        rest = sys.argv[sys.argv.index("--engine-calls") + 1:]
        engine_call_goldens(rest[0] if rest else None)
        sys.exit(0)
    if "--gemm-plans" in sys.argv or "--gemm-plans-child" in sys.argv:      # AMDSPEECH_LIB=<parent build> python tools/make_golden.py --gemm-plans
        gemm_plan_goldens(sys.argv[sys.argv.index("--gemm-plans-child") + 1] if "--gemm-plans-child" in sys.argv else None)
        sys.exit(0)
    if "--checkpoints" in sys.argv:      # python tools/make_golden.py --checkpoints <checkout of 9bbf15b>
        checkpoint_goldens(os.path.abspath(sys.argv[sys.argv.index("--checkpoints") + 1]))
        sys.exit(0)
    if "--corpus-only" not in sys.argv:
        main()
    else:
        _stub_modules()
    corpus_walk_golden()
