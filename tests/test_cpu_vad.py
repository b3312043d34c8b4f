"""Long recordings, the part that needs no GPU: the numpy restatement of the detector (tests/vad_ref.py) against its own checks, the
cut planner (rnn_speech_amd/segmenter.py) against an independent reference and its invariants, the frame budget against the
library's own host-side length functions, the config keys, the plan query, and stt.process_file's choice of path with stub models."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

import vad_ref as R
from rnn_speech_amd import hyperparams, lib, ops, segmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the numpy emulation
def test_energy_reference_on_hand_made_rows():
    h = 4
    x = np.array([1, 1, 1, 1, 2, 2, 2, 2, 3, np.nan, np.nan], np.float32)
    ref = R.energy_ref(x, 9, h)                                       # blocks 4, 16, 9 (one sample): F = 3
    want = 10 * np.log10(np.array([(4 + 16) / 8.0, (16 + 9) / 8.0, 9 / 8.0]))      # the divisor stays 2 h at the ragged end
    assert np.allclose(ref, want, rtol=0, atol=1e-12)
    assert len(R.energy_ref(x, 0, h)) == 0
    assert R.energy_ref(np.zeros(8, np.float32), 8, h).tolist() == [-120.0, -120.0]          # digital silence
    x[5] = np.inf
    assert R.energy_ref(x, 9, h).tolist()[:2] == [-120.0, -120.0] and np.isfinite(R.energy_ref(x, 9, h)[2])
    tol = R.energy_tolerance(np.array([-120.0, -1.0, 0.0, 30.0]), 441)
    assert np.all(tol < 1e-5) and tol[2] == pytest.approx(4.34294 * 882 * 2.0 ** -53, rel=1e-4)
    for name in R.ENERGY_CASES:
        pcm, lengths, hop, fields = R.energy_case(name)
        plan = ops.vad_plan(len(lengths), pcm.shape[1], hop)
        assert plan == R.expected_plan(len(lengths), pcm.shape[1], hop), name
        assert {k: plan[k] for k in fields} == fields, (name, plan)
        assert all(np.isnan(pcm[b, n:]).all() and np.isfinite(pcm[b, :n]).all() for b, n in enumerate(lengths))
    assert {R.ENERGY_CASES[c][3]["load_vec"] for c in R.ENERGY_CASES} == {1, 4}
    assert [R.hop_of(r) for r in (8000, 16000, 22050, 44100)] == [80, 160, 220, 441]


@pytest.mark.parametrize("min_run", (1, 2, 5, 9))
def test_opening_keeps_exactly_the_long_runs(min_run):
    rng = np.random.RandomState(min_run)
    raw = rng.rand(600) < 0.7
    out = R.opening(raw, min_run)
    assert R.runs_of(out) == [(a, b) for a, b in R.runs_of(raw) if b - a >= min_run]
    assert not np.any(out & ~raw)


def test_threshold_edge_cases_and_hangover():
    d = R.DEFAULTS
    loud, stats = R.flags_ref(np.full(50, -30.0, np.float32), 50, **d)
    assert loud.all() and stats.tolist() == [-30.0, -30.0, -40.0]            # the cap peak - margin: a stationary row is all speech
    quiet, stats = R.flags_ref(np.full(50, -90.0, np.float32), 50, **d)
    assert not quiet.any() and stats.tolist() == [-90.0, -90.0, -100.0]      # ... and none of it below min_db
    speech, stats = R.flags_ref(np.zeros(0, np.float32), 0, **d)
    assert len(speech) == 0 and stats.tolist() == [-120.0] * 3
    e = np.full(100, -80.0, np.float32)
    e[40:44], e[60:65] = -20.0, -20.0
    speech, stats = R.flags_ref(e, 100, **dict(d, hangover=3))
    assert R.runs_of(speech) == [(57, 68)] and stats.tolist() == [-80.0, -20.0, -70.0]       # four frames cleared, five kept and widened
    assert R.flags_ref(e, 100, **dict(d, hangover=1024))[0].all()
    for name, (energy, opts) in R.flags_cases().items():                     # the synthetic rows really hold what their names say
        speech, stats = R.flags_ref(energy, len(energy), **dict(d, **opts))
        assert speech.dtype == np.uint8 and stats[0] <= stats[1], name
    near = R.flags_cases()["last_pass_tie"][0]
    assert len(np.unique(near.view(np.uint32) >> 8)) == 1 and len(np.unique(near)) == 5


# ---------------------------------------------------------------- the planner
def _random_rows(seed, F):
    rng = np.random.RandomState(seed)
    speech = np.zeros(F, np.uint8)
    t = 0
    while t < F:
        gap, run = rng.randint(1, 60), rng.randint(1, 400 if rng.rand() < 0.3 else 40)
        speech[t + gap:t + gap + run] = 1
        t += gap + run
    energy = np.round(rng.randn(F) * 3.0).astype(np.float32) - 40.0          # rounded: ties inside the cut windows
    return speech, energy


@pytest.mark.parametrize("seed", range(12))
def test_planner_on_random_rows(seed):
    speech, energy = _random_rows(seed, 1500 + 37 * seed)
    budget, pad = (90, 10) if seed % 2 else (57, 0)
    got = segmenter.plan_frames(speech, energy, budget, pad)
    assert got == R.planner_ref(speech, energy, budget, pad)
    R.check_plan_invariants(speech, got, budget)
    l_max = budget - 2 * pad
    cuts = set()                                                              # the forced cuts: each on its window's LAST minimum
    for a, b in R.runs_of(speech):
        while b - a > l_max:
            window = energy[a + l_max // 2:a + l_max + 1]
            a = a + l_max // 2 + int(max(np.flatnonzero(window == window.min())))
            cuts.add(a)
    inside = lambda x: any(a < x < b for a, b in R.runs_of(speech))
    assert {x for seg in got for x in seg if inside(x)} <= cuts               # a segment ends inside a region only at such a cut
    assert all(b - a <= l_max for a, b in R.runs_of(speech)) or cuts


def test_planner_on_hand_made_rows():
    F, budget, pad = 400, 100, 10                                            # Lmax = 80
    energy = np.full(F, -40.0, np.float32)
    none = np.zeros(F, np.uint8)
    assert segmenter.plan_frames(none, energy, budget, pad) == [] and segmenter.plan_spans(none, energy, F * 160, 160, budget, pad) == []
    exact = none.copy()
    exact[100:180] = 1                                                       # one region of exactly Lmax: one segment of the whole budget
    assert segmenter.plan_frames(exact, energy, budget, pad) == [(90, 190)]
    longer = none.copy()
    longer[100:181] = 1                                                      # Lmax + 1: a forced cut, on the LAST of the equal minima
    assert segmenter.plan_frames(longer, energy, budget, pad) == [(90, 180), (180, 191)]
    energy[150] = -50.0
    assert segmenter.plan_frames(longer, energy, budget, pad) == [(90, 150), (150, 191)]     # ... or on the window's minimum
    close = none.copy()
    close[0:30], close[34:60], close[70:120] = 1, 1, 1                        # two phrases share a row; padding clipped at 0 and mid-gap
    assert segmenter.plan_frames(close, energy, budget, pad) == [(0, 65), (65, 130)]
    ends = none.copy()
    ends[395:400] = 1
    assert segmenter.plan_frames(ends, energy, budget, pad) == [(385, 400)]
    assert segmenter.plan_spans(ends, energy, 400 * 160 - 100, 160, budget, pad) == [(385 * 160, 15 * 160 - 100, 385, 400)]
    assert segmenter.plan_spans(ends, energy, 400 * 160 - 100, 160, budget, pad) == R.spans_ref(ends, energy, 400 * 160 - 100, 160, budget, pad)
    with pytest.raises(ValueError, match="budget"):
        segmenter.plan_frames(none, energy, 21, 10)
    # a span below the front end's minimum is widened where the row allows; a row below it yields nothing
    tiny = np.zeros(10, np.uint8)
    tiny[9] = 1
    assert segmenter.plan_spans(tiny, energy[:10], 95, 10, 8, 0, min_samples=40) == [(55, 40, 9, 10)]
    assert segmenter.plan_spans(tiny, energy[:10], 95, 10, 8, 0, min_samples=96) == []


@pytest.mark.parametrize("load_sr", (16000, 22050))
@pytest.mark.parametrize("mode", ("mfcc", "fbank"))
def test_budget_honours_the_front_end(mode, load_sr):
    handle = lib.load()
    imode = ops.MODE_MFCC if mode == "mfcc" else ops.MODE_FBANK
    for rate in (8000, 11025, 16000, 22050, 44100):
        for max_frames in (90, 1001):
            hop = R.hop_of(rate)
            budget = segmenter.frame_budget(rate, hop, load_sr, mode, max_frames)

            def frames(n):
                m = handle.amdspeech_resample_rows_num_samples(n, rate, load_sr, 1000)
                return handle.amdspeech_frontend_num_frames(imode, m, load_sr)
            assert budget > 0 and frames(budget * hop) <= max_frames < frames((budget + 1) * hop), (rate, max_frames, budget)
    # the two modes count frames differently (1001 against 998 for 10 s at 16 kHz), and so do their budgets
    assert segmenter.frame_budget(16000, 160, 16000, "mfcc", 1001) == 1000 and segmenter.frame_budget(16000, 160, 16000, "fbank", 1001) == 1003
    short = segmenter.min_span_samples(16000, 16000, mode, 20)
    assert segmenter.model_frames(short, 16000, 16000, mode) >= (9 if mode == "fbank" else 1)


# ---------------------------------------------------------------- config keys
_KEYS = {"long_audio": "truncate", "vad_floor_percentile": 10, "vad_margin_db": 10.0, "vad_range_db": 50.0, "vad_min_db": -70.0,
         "vad_min_speech_ms": 50.0, "vad_hangover_ms": 200.0, "vad_pad_ms": 100.0}


def test_config_keys(tmp_path):
    src = open(os.path.join(ROOT, "config.ini")).read()
    hp = hyperparams.read_config_file(os.path.join(ROOT, "config.ini"))
    assert {k: hp[k] for k in _KEYS} == _KEYS
    assert not set(_KEYS) & set(hyperparams._STRUCTURAL)
    old = tmp_path / "old.ini"                                               # an older file, without the keys
    old.write_text("\n".join(l for l in src.splitlines() if not re.match(r"(long_audio|vad_\w+) :", l)) + "\n")
    assert "\nlong_audio :" not in old.read_text() and "\nvad_pad_ms :" not in old.read_text()
    hp = hyperparams.read_config_file(str(old))
    assert {k: hp[k] for k in _KEYS} == _KEYS
    seg = tmp_path / "seg.ini"
    seg.write_text(src.replace("long_audio : truncate", "long_audio : segment").replace("vad_min_db : -70", "vad_min_db : -55.5"))
    hp = hyperparams.read_config_file(str(seg))
    assert hp["long_audio"] == "segment" and hp["vad_min_db"] == -55.5
    bad = {"long_audio": "chunk", "vad_floor_percentile": "101", "vad_margin_db": "nan", "vad_range_db": "-1", "vad_min_db": "inf",
           "vad_min_speech_ms": "-5", "vad_hangover_ms": "10241", "vad_pad_ms": "x"}
    for key, value in bad.items():
        line = [l for l in src.splitlines() if l.startswith(key + " :")]
        assert len(line) == 1
        p = tmp_path / ("bad_%s.ini" % key)
        p.write_text(src.replace(line[0], "%s : %s" % (key, value)))
        with pytest.raises(ValueError, match=key):
            hyperparams.read_config_file(str(p))


# ---------------------------------------------------------------- the plan query and the header
def test_plan_query_and_header():
    handle = lib.load()
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_vad_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.VadPlanInfo._fields_]
    assert ctypes.sizeof(lib.VadPlanInfo) == 4 * len(lib.VadPlanInfo._fields_)
    hour = ops.vad_plan(1, 57600000, 160)                                    # one hour at 16 kHz, ONE row: the grid must fill the chip
    cus = handle.amdspeech_device_cu_count()
    assert hour["workgroups"] >= (cus if cus > 0 else 256) and hour["workgroups"] == hour["tiles_per_row"] == 5715
    assert hour == R.expected_plan(1, 57600000, 160) and hour["load_vec"] == 4 and hour["f_max"] == 360000
    assert ops.vad_plan(1, 441000, 441)["load_vec"] == 1 and ops.vad_plan(32, 220500, 220)["workgroups"] == 32 * 16
    info = lib.VadPlanInfo()
    for args, text in (((0, 100, 10), b"bad shape"), ((1, 0, 10), b"bad shape"), ((1, 100, 0), b"hop"), ((1, 100, -3), b"hop"),
                       ((3, 2 ** 31 - 1, 1), b"do not fit")):
        assert handle.amdspeech_vad_plan(*args, ctypes.byref(info)) != 0 and text in handle.amdspeech_last_error(), args
    assert handle.amdspeech_vad_plan(1, 100, 10, None) != 0 and b"null" in handle.amdspeech_last_error()
    assert [handle.amdspeech_vad_num_frames(n, 160) for n in (0, 1, 159, 160, 161)] == [0, 1, 1, 1, 2]
    assert handle.amdspeech_vad_num_frames(-1, 160) < 0 and handle.amdspeech_vad_num_frames(5, 0) < 0
    assert handle.amdspeech_vad_workspace_bytes(2, 1601, 160) == 2 * 11 * 4 and handle.amdspeech_vad_workspace_bytes(2, 1601, 0) == 0
    with pytest.raises(lib.AmdSpeechError, match="hop"):
        ops.vad_plan(1, 100, 0)


# ---------------------------------------------------------------- stt.process_file picks its path
class _Processor(object):
    """What process_file reads of an AudioProcessor, with the long-recording calls recorded."""
    out_seq_length = max_input_seq_length = 90
    load_sr, feature_type = 16000, "mfcc"

    def __init__(self, frames, spans=()):
        self.frames, self.spans, self.calls = frames, list(spans), []

    def process_audio_file(self, file):
        self.calls.append(("process_audio_file", file))
        return np.ones((min(self.frames, 90), 7), np.float32), self.frames

    def segment(self, signal, sr, **vad):
        from rnn_speech_amd.audioprocessor import Segments
        self.calls.append(("segment", len(signal), sr, vad))
        return Segments("pcm", len(signal), sr, 160, self.spans, (-60.0, -20.0, -50.0))

    def process_segments(self, pcm, n, sr, spans, rows=None):
        self.calls.append(("process_segments", len(spans), rows))
        return np.zeros((90, rows, 7), np.float32), [int(sp[1]) // 160 for sp in spans] + [0] * (rows - len(spans))


class _Model(object):
    def __init__(self, log, batch_size):
        self.log, self.batch_size = log, batch_size

    def process_input(self, session, inputs, lengths):
        self.log.append((self.batch_size, np.asarray(inputs).shape, list(lengths)))
        return [[1 + (n % 3)] if n else [] for n in lengths]                 # one token per row, from its length


def _stt(monkeypatch, models):
    import stt
    monkeypatch.setattr(stt, "_forward_model", lambda hp, B: models.append(_Model([], B)) or models[-1])
    monkeypatch.setattr(stt.dataprocessor.DataProcessor, "get_labels_str", staticmethod(lambda char_map, p: "".join("abc"[i - 1] for i in p)))
    return stt


@pytest.mark.parametrize("key", (None, "truncate"))
def test_process_file_truncates_by_default(monkeypatch, key, capsys):
    models = []
    stt = _stt(monkeypatch, models)
    monkeypatch.setattr(stt, "decode_files", lambda files: pytest.fail("the default path decodes through process_audio_file only"))
    proc = _Processor(frames=400)
    hp = {"char_map": None, "batch_size": 4}
    if key:
        hp["long_audio"] = key
    assert stt.process_file(proc, hp, "long.wav") == ["a"]                   # min(400, 90) = 90 frames: token 1 + 90 % 3
    assert proc.calls == [("process_audio_file", "long.wav")] and [m.batch_size for m in models] == [1]
    assert models[0].log == [(1, (90, 1, 7), [90])]
    assert capsys.readouterr().out.strip() == "['a']"


def test_process_file_segments_only_what_does_not_fit(monkeypatch, caplog):
    models = []
    stt = _stt(monkeypatch, models)
    hp = {"char_map": None, "batch_size": 2, "long_audio": "segment", "vad_pad_ms": 50.0, "vad_min_db": -60.0}
    monkeypatch.setattr(stt, "decode_files", lambda files: [(np.zeros(8000, np.float32), 16000)])       # half a second: it fits
    proc = _Processor(frames=51)
    assert stt.process_file(proc, hp, "short.wav") == ["a"]
    assert proc.calls == [("process_audio_file", "short.wav")]
    monkeypatch.setattr(stt, "decode_files", lambda files: [(np.zeros(64000, np.float32), 16000)])      # four seconds: it does not
    spans = [(0, 160 * 40, 0, 40), (160 * 50, 160 * 80, 50, 130), (160 * 200, 160 * 31, 200, 231)]
    proc = _Processor(frames=401, spans=spans)
    with caplog.at_level(logging.INFO):
        assert stt.process_file(proc, hp, "long.wav") == ["b c b"]           # 40, 80 and 31 frames
    assert proc.calls == [("segment", 64000, 16000, {"pad_ms": 50.0, "min_db": -60.0}), ("process_segments", 2, 2), ("process_segments", 1, 2)]
    assert [m.batch_size for m in models[1:]] == [2] and models[1].log == [(2, (90, 2, 7), [40, 80]), (2, (90, 2, 7), [31, 0])]
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.INFO]
    assert lines == ["0.000 0.400 b", "0.500 1.300 c", "2.000 2.310 b"]
    proc = _Processor(frames=401, spans=[])                                  # nothing was flagged: one empty string, no model built
    assert stt.process_file(proc, hp, "long.wav") == [""] and len(models) == 2
