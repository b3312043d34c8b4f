"""Long recordings on the GPU: the voice-activity kernels and the ragged gather (csrc/vad.hip) against tests/vad_ref.py -- the
energies within the derived bound of a float64 evaluation, the flags, the stats and the gather bit for bit -- what the calls
refuse, and stt.py --file with `long_audio : segment` end to end on a tiny model."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import vad_ref as R
from rnn_speech_amd import lib, ops, segmenter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------- energy
@pytest.mark.parametrize("name", sorted(R.ENERGY_CASES))
def test_energy_against_float64(name):
    pcm, lengths, hop, fields = R.energy_case(name)
    B, n_max = pcm.shape
    plan = ops.vad_plan(B, n_max, hop)
    assert {k: plan[k] for k in fields} == fields, plan                   # the case runs the variant it was written for
    dev = torch.from_numpy(pcm).cuda()
    out = torch.full((B, plan["f_max"] + 3), 7.0, device="cuda")          # wider than needed: -120 up to f_max, whatever was there
    first = ops.vad_energy(dev, lengths, hop, out=out).cpu().numpy()
    again = ops.vad_energy(dev, lengths, hop).cpu().numpy()               # ... and into a tensor of the call's own
    assert again.shape == (B, plan["f_max"]) and np.array_equal(bits(first[:, :plan["f_max"]]), bits(again))      # two runs, the same bits
    worst = R.check_energy(first, pcm, lengths, hop)
    print("%s: worst error / bound %.3f" % (name, worst))


def test_energy_of_an_inf_sample_and_of_silence():
    pcm, lengths, hop, _ = R.energy_case("ragged_b3")
    pcm[0, 5 * hop + 7] = np.inf                                          # block 5: frames 4 and 5 read -120, their neighbours do not
    pcm[2, :3333] = 0.0                                                   # digital silence
    got = ops.vad_energy(torch.from_numpy(pcm).cuda(), lengths, hop).cpu().numpy()
    R.check_energy(got, pcm, lengths, hop)
    assert got[0, 4] == got[0, 5] == -120.0 and got[0, 3] > -119.0 and got[0, 6] > -119.0
    assert np.all(got[2] == -120.0) and np.all(got[1] == -120.0)


# ---------------------------------------------------------------- flags
def _check_flags(energy, n_frames, opts):
    """One call on energy [B, f_max] (device) against the reference, row by row: speech and stats bit for bit, zeros past F."""
    speech, stats = ops.vad_flags(energy, n_frames, **opts)
    speech, stats, host = speech.cpu().numpy(), stats.cpu().numpy(), energy.cpu().numpy()
    for b, F in enumerate(n_frames):
        want, want_stats = R.flags_ref(host[b], F, **opts)
        assert np.array_equal(speech[b, :F], want), (b, F, np.flatnonzero(speech[b, :F] != want)[:8])
        assert not speech[b, F:].any()
        assert np.array_equal(bits(stats[b]), bits(want_stats)), (b, stats[b], want_stats)
    return speech


def test_flags_on_the_kernels_own_energies():
    for name in ("ragged_b3", "edges_h160", "many_tiles_441"):
        pcm, lengths, hop, _ = R.energy_case(name)
        energy = ops.vad_energy(torch.from_numpy(pcm).cuda(), lengths, hop)
        n_frames = [R.ceil_div(n, hop) for n in lengths]
        _check_flags(energy, n_frames, dict(R.DEFAULTS))
        speech = _check_flags(energy, n_frames, dict(R.DEFAULTS, percentile=50, margin_db=3.0, min_run=2, hangover=4))
        assert name != "many_tiles_441" or 0 < speech.sum() < speech.size          # a level that moves: some speech, some not


_FLAGS = R.flags_cases()


@pytest.mark.parametrize("name", sorted(_FLAGS))
def test_flags_on_synthetic_rows(name):
    energy, opts = _FLAGS[name]
    F = len(energy)
    row = np.full((1, F + 5), np.nan, np.float32)                         # words past F are not read
    row[0, :F] = energy
    speech = _check_flags(torch.from_numpy(row).cuda(), [F], dict(R.DEFAULTS, **opts))
    if name == "all_equal_loud":
        assert speech[0, :F].all()
    if name in ("all_equal_quiet", "min_run_long"):
        assert not speech.any()
    if name == "bursts":
        assert not speech[0, 20:40].any() and speech[0, 40:85].all() and not speech[0, 85:100].any()      # the run of 4 is gone, that of 5 widened


def test_flags_of_ragged_rows_in_one_call():
    rng = np.random.RandomState(11)
    n_frames = [0, 700, 1, 1300, 64]
    rows = np.full((5, 1300), np.nan, np.float32)
    for b, F in enumerate(n_frames):
        rows[b, :F] = (-55.0 + 35.0 * (np.sin(np.arange(F) / (5.0 + b)) > 0.2) + rng.randn(F)).astype(np.float32)
    _check_flags(torch.from_numpy(rows).cuda(), n_frames, dict(R.DEFAULTS, min_run=3, hangover=7))


# ---------------------------------------------------------------- gather
def _gather_case(n_max, lengths, spans, w_out):
    rng = np.random.RandomState(n_max + w_out)
    pcm = np.full((len(lengths), n_max), np.nan, np.float32)             # poisoned at and past each length
    for b, n in enumerate(lengths):
        pcm[b, :n] = rng.randn(n).astype(np.float32)
    row, start, count = ([sp[i] for sp in spans] for i in range(3))
    out = torch.full((len(spans), w_out), np.nan, device="cuda")
    got = ops.gather_spans(torch.from_numpy(pcm).cuda(), lengths, row, start, count, w_out, out=out).cpu().numpy()
    want = R.gather_ref(pcm, lengths, row, start, count, w_out)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:8]
    return got


def test_gather_bit_for_bit():
    lengths = [1000, 333]
    spans = [(0, s, 100) for s in (0, 1, 2, 3, 4, 5, 6, 7)]              # every residue of the start mod 4
    spans += [(0, 900, 100), (0, 950, 100), (0, 1000, 10), (0, 5000, 10)]      # ending at n, reaching past it, starting at and past it
    spans += [(0, 10, 0), (1, 0, 120), (1, 301, 32), (1, 330, 120), (0, 17, 3)]      # count 0; the other row; past ITS length
    for n_max, w_out in ((1000, 120), (1000, 121), (1003, 120), (1003, 7)):      # aligned rows or row 0 alone; spans that share a vector
        got = _gather_case(n_max, lengths, spans, w_out)
        assert not got[12].any() and not got[11].any()                    # count 0, a start past the row: zeros
    _gather_case(1000, lengths, [(b % 2, 3 * b, 40 + b % 5) for b in range(300)], 44)      # more spans than travel as arguments
    empty = ops.gather_spans(torch.zeros(1, 8, device="cuda"), [8], [], [], [], 16)      # S = 0: a no-op that succeeds
    assert tuple(empty.shape) == (0, 16)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    handle = lib.load()
    pcm = torch.zeros(2, 1600, device="cuda")
    energy = torch.full((2, 10), 3.0, device="cuda")

    def refused(text, call, *outputs):
        before = [o.clone() for o in outputs]
        with pytest.raises(lib.AmdSpeechError, match=text):
            call()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, outputs)), text

    refused("hop", lambda: ops.vad_energy(pcm, [1600, 5], 0, out=energy), energy)
    refused("n_samples\\[1\\] = -1", lambda: ops.vad_energy(pcm, [1600, -1], 160, out=energy), energy)
    refused("n_samples\\[0\\] = 1601", lambda: ops.vad_energy(pcm, [1601, 0], 160, out=energy), energy)
    refused("f_max 9 is below", lambda: ops.vad_energy(pcm, [1600, 5], 160, out=energy[:, :9].contiguous()), energy)
    odd = torch.zeros(1601, device="cuda")[1:].view(1, 1600)
    refused("16-byte aligned", lambda: ops.vad_energy(odd, [1600], 160, out=energy[:1]), energy)
    assert handle.amdspeech_vad_energy(None, None, (ctypes.c_int * 2)(5, 5), 2, 1600, 160, energy.data_ptr(), 10, None) != 0
    assert b"null pointer" in handle.amdspeech_last_error()

    speech, stats = torch.full((2, 10), 9, device="cuda", dtype=torch.uint8), torch.full((2, 3), 5.0, device="cuda")
    for text, opts in (("percentile -1", dict(percentile=-1)), ("percentile 101", dict(percentile=101)), ("min_run 0", dict(min_run=0)),
                       ("hangover -1", dict(hangover=-1)), ("hangover 1025", dict(hangover=1025)), ("must be finite", dict(margin_db=float("nan"))),
                       ("must be finite", dict(range_db=float("inf"))), ("must be finite", dict(min_db=float("-inf")))):
        refused(text, lambda: ops.vad_flags(energy, [10, 3], speech=speech, stats=stats, **dict(R.DEFAULTS, **opts)), speech, stats)
    refused("n_frames\\[1\\] = -2", lambda: ops.vad_flags(energy, [10, -2], speech=speech, stats=stats), speech, stats)
    refused("n_frames\\[0\\] = 11", lambda: ops.vad_flags(energy, [11, 0], speech=speech, stats=stats), speech, stats)
    assert handle.amdspeech_vad_flags(None, energy.data_ptr(), (ctypes.c_int * 2)(5, 5), 2, 10, 10, 10.0, 50.0, -70.0, 5, 20, speech.data_ptr(),
                                      stats.data_ptr(), None) != 0 and b"null pointer" in handle.amdspeech_last_error()

    out = torch.full((2, 8), 4.0, device="cuda")
    refused("w_out 0", lambda: ops.gather_spans(pcm, [1600, 5], [0, 1], [0, 0], [8, 8], 0), out)
    refused("negative start -1 or count 8", lambda: ops.gather_spans(pcm, [1600, 5], [0, 1], [-1, 0], [8, 8], 8, out=out), out)
    refused("negative start 0 or count -8", lambda: ops.gather_spans(pcm, [1600, 5], [0, 1], [0, 0], [8, -8], 8, out=out), out)
    refused("row\\[1\\] = 2", lambda: ops.gather_spans(pcm, [1600, 5], [0, 2], [0, 0], [8, 8], 8, out=out), out)
    refused("n_samples\\[1\\] = -5", lambda: ops.gather_spans(pcm, [1600, -5], [0, 1], [0, 0], [8, 8], 8, out=out), out)
    shifted = torch.full((17,), 4.0, device="cuda")[1:].view(2, 8)
    refused("out must be 16-byte aligned", lambda: ops.gather_spans(pcm, [1600, 5], [0, 1], [0, 0], [8, 8], 8, out=shifted), shifted)


# ---------------------------------------------------------------- end to end
def _write_wav(path, sig, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(sig, -1, 1) * 32767).astype("<i2").tobytes())


def _config(tmp_path, long_audio):
    """The repository's config.ini with a tiny model of 90 frames at 16 kHz.  Hangover and padding of 30 ms each: a burst of 0.7 s
    is then 70 + 2 (a frame spans two blocks) + 6 frames of speech, below Lmax = 89 - 6, so only the 1.2 s burst is cut by force."""
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, new in (("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 20"),
                     ("num_layers : 3", "num_layers : 1"), ("hidden_size : 512", "hidden_size : 32"), ("batch_size : 32", "batch_size : 2"),
                     ("n_mfcc : 40", "n_mfcc : 20"), ("sample_rate : 22050", "sample_rate : 16000"), ("vad_hangover_ms : 200", "vad_hangover_ms : 30"),
                     ("vad_pad_ms : 100", "vad_pad_ms : 30"), ("long_audio : truncate", long_audio)):
        assert old in src, old
        src = src.replace(old, new, 1)
    cfg = tmp_path / ("config_%d.ini" % len(long_audio))
    cfg.write_text(src)
    return str(cfg)


def test_stt_file_segments_a_long_recording(tmp_path, capsys):
    import stt
    import util.hyperparams as hyperparams
    from models.SpeechRecognizer import SpeechRecognizer
    from util.dataprocessor import DataProcessor
    sr = 16000
    signal, bursts = R.bursts_recording(sr, seed=3, long_burst_s=1.2)
    path = str(tmp_path / "long.wav")
    _write_wav(path, signal, sr)
    sig, got_sr = ops.audio_decode(path)
    assert got_sr == sr and len(sig) == len(signal) > 4 * 90 * 160

    def hyper_params(long_audio):
        hp = hyperparams.HyperParameterHandler(_config(tmp_path, long_audio)).get_hyper_params()
        ap = stt.build_audio_processor(hp)
        reco = SpeechRecognizer(hp["language"])
        hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
        return hp, ap

    hp, ap = hyper_params("long_audio : segment")
    assert hp["long_audio"] == "segment" and ap.max_input_seq_length == 90 and ap.load_sr == sr
    tiny = stt._forward_model(hp, 1)                                      # a tiny acoustic checkpoint, saved as the command line restores it
    tiny.save(None, hp["checkpoint_dir"] + "/acoustic/")
    tiny.close()
    texts_of = lambda predictions: [DataProcessor.get_labels_str(hp["char_map"], p) for p in predictions]

    # the spans: the planner reference on the kernels' own flags and energies; every burst inside exactly one span, but for the
    # 1.2 s one, which is cut by force inside
    vad = dict(floor_percentile=hp["vad_floor_percentile"], margin_db=hp["vad_margin_db"], range_db=hp["vad_range_db"], min_db=hp["vad_min_db"],
               min_speech_ms=hp["vad_min_speech_ms"], hangover_ms=hp["vad_hangover_ms"], pad_ms=hp["vad_pad_ms"])
    seg = ap.segment(sig, sr, **vad)
    hop, n = 160, len(sig)
    F = R.ceil_div(n, hop)
    pcm = torch.from_numpy(sig[None, :]).cuda()
    energy = ops.vad_energy(pcm, [n], hop)
    speech, stats = ops.vad_flags(energy, [F], 10, 10.0, 50.0, -70.0, 5, 3)
    energy, speech = energy[0, :F].cpu().numpy(), speech[0, :F].cpu().numpy()
    assert np.array_equal(speech, R.flags_ref(energy, F, 10, 10.0, 50.0, -70.0, 5, 3)[0])
    budget = segmenter.frame_budget(sr, hop, sr, "mfcc", 90)
    assert budget == 89 and (seg.n, seg.sr, seg.hop) == (n, sr, hop) and seg.stats == tuple(float(v) for v in stats[0].cpu().numpy())
    assert seg.spans == R.spans_ref(speech, energy, n, hop, budget, 3) and len(seg.spans) >= 5
    R.check_plan_invariants(speech, [(s, e) for _, _, s, e in seg.spans], budget)
    for i, (b0, b1) in enumerate(bursts):
        holders = [k for k, (a, c, _, _) in enumerate(seg.spans) if a <= b0 and b1 <= a + c]
        touched = [k for k, (a, c, _, _) in enumerate(seg.spans) if a < b1 and b0 < a + c]
        if i == 1:                                                       # 120 frames: consecutive spans that meet at forced cuts
            assert len(touched) >= 2 and touched == list(range(touched[0], touched[-1] + 1)) and not holders
            assert seg.spans[touched[0]][0] <= b0 and b1 <= sum(seg.spans[touched[-1]][:2])
            assert all(sum(seg.spans[k][:2]) == seg.spans[k + 1][0] for k in touched[:-1])
        else:
            assert len(holders) == 1 and touched == holders, (i, holders, touched)

    # the features of the spans: what process_batch makes of the same spans cut on the host, bit for bit
    feat, lengths = ap.process_segments(seg.pcm, seg.n, seg.sr, seg.spans)
    want, want_lengths = ap.process_batch([sig[a:a + c] for a, c, _, _ in seg.spans], sr)
    assert tuple(feat.shape) == (90, len(seg.spans), 20) and list(lengths) == list(want_lengths) and max(lengths) <= 90
    assert np.array_equal(bits(feat), bits(want))

    # the text: the per-row decodes of the same batches, joined by spaces
    capsys.readouterr()
    got = stt.process_file(ap, hp, path)
    assert capsys.readouterr().out.strip() == str(got)
    model = stt._forward_model(hp, 2)
    rows = []
    for i in range(0, len(seg.spans), 2):
        part = seg.spans[i:i + 2]
        f, ln = ap.process_segments(seg.pcm, seg.n, seg.sr, part, rows=2)
        rows += texts_of(model.process_input(None, f, [min(v, 90) for v in ln]))[:len(part)]
    model.close()
    assert len(rows) == len(seg.spans) and got == [" ".join(rows)]

    # the same file with the key at truncate (or absent): the first 90 frames alone, as before
    hp_t, ap_t = hyper_params("long_audio : truncate")
    assert hp_t["long_audio"] == "truncate"
    truncated = stt.process_file(ap_t, hp_t, path)
    feat_vec, original = ap_t.process_audio_file(path)
    assert original > 4 * 90 and feat_vec.shape == (90, 20)
    model = stt._forward_model(hp_t, 1)
    assert truncated == texts_of(model.process_input(None, feat_vec[:, None, :], [90]))
    model.close()
    del hp_t["long_audio"]
    assert stt.process_file(ap_t, hp_t, path) == truncated
