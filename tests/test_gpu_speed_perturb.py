"""The per-row resampler / speed perturbation on the GPU (csrc/frontend.hip: resample_rows_kernel) against the float64 oracle of
tests/speed_perturb_ref.py: every produced sample within the bound the resampler test of test_gpu_frontend.py holds amdspeech_resample to, poison
past every input row and in the output buffer, bit-exact copy rows; then the layers above it up to a config-built training dataset."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speed_perturb_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(name, out_extra=0):
    """One ops.resample_rows call on a case: (out [B][out_max] numpy, lengths, the case).  out_extra > 0: a wider poisoned `out`."""
    from rnn_speech_amd import ops
    rate_in, rate_out, n, pm, host, refs = ref.built(name)
    pcm = torch.from_numpy(host).cuda()
    out_max = max(max(len(r) for r in refs), 1) + out_extra
    out = torch.full((len(n), out_max), float("nan"), device="cuda")
    got, n_out = ops.resample_rows(pcm, n, pm, rate_in, rate_out, out=out)
    assert got is out
    return out.cpu().numpy(), n_out, (rate_in, rate_out, n, pm, host, refs)


@pytest.mark.parametrize("name", sorted(ref.cases()))
def test_rows_match_the_float64_oracle(name):
    from rnn_speech_amd import ops
    rate_in, rate_out, rows, special = ref.cases()[name]
    out, n_out, (_, _, n, pm, host, refs) = _run(name, out_extra=3 if name != "up" else 0)
    plan = ops.resample_rows_plan(n, pm, host.shape[1], rate_in, rate_out, out_max=out.shape[1])
    assert plan == ref.expected_plan(n, pm, rate_in, rate_out, out_max=out.shape[1]) and plan["tile"] == ref.TILE
    if name == "tile_edges":
        assert sorted(set(t % ref.TILE for t in n_out)) == [0, 1, ref.TILE - 1]
    if name == "wide":
        assert plan["meta_launches"] == 3
    assert not np.isnan(out[[b for b in range(len(n)) if b not in special]]).any()      # nothing at or past a row's n was read
    worst = 0.0
    for b in range(len(n)):
        want = refs[b]
        assert n_out[b] == len(want) == ref.n_total(n[b], rate_in, rate_out, pm[b])
        assert not bits(out[b, n_out[b]:]).any(), (name, b)                             # +0.0f from n_total to out_max
        if ref.is_copy(rate_in, rate_out, pm[b]):
            assert np.array_equal(bits(out[b, :n_out[b]]), bits(host[b, :n[b]])), (name, b)      # bit for bit
            continue
        k = ref.n_interp(n[b], rate_in, rate_out, pm[b])
        assert not bits(out[b, k:n_out[b]]).any(), (name, b)                            # the 0 or 1 padding samples
        if n_out[b]:
            worst = max(worst, float(np.abs(out[b, :n_out[b]] - want).max()))
    print("resample_rows %s: max |error| %.3g" % (name, worst))
    assert worst < ref.BOUND, (name, worst)


def test_two_calls_give_the_same_bits_and_resample_is_resample_rows_at_1000_permille():
    """Determinism; and ops.resample is ops.resample_rows with every row at 1000 permille: the same lengths and the same bits, on input
    that is NaN past every row, within the oracle's bound."""
    from rnn_speech_amd import ops
    first, _, _ = _run("edges16k")
    second, _, _ = _run("edges16k")
    assert np.array_equal(bits(first), bits(second))
    for name, rows in (("edges16k", None), ("down", [3]), ("wide", None)):
        rate_in, rate_out, n, pm, host, refs = ref.built(name)
        rows = list(range(len(n))) if rows is None else rows
        assert name != "down" or [pm[b] for b in rows] == [1000]
        pcm = torch.from_numpy(np.ascontiguousarray(host[rows])).cuda()
        n_rows = [n[b] for b in rows]
        new, n_new = ops.resample_rows(pcm, n_rows, [1000] * len(rows), rate_in, rate_out)
        old, n_old = ops.resample(pcm, n_rows, rate_in, rate_out)
        assert n_new == n_old == [ref.n_total(k, rate_in, rate_out, 1000) for k in n_rows] and new.shape == old.shape
        new, old = new.cpu().numpy(), old.cpu().numpy()
        assert not np.isnan(new).any() and np.array_equal(bits(new), bits(old)), name
        worst = 0.0
        for i, b in enumerate(rows):
            if n[b] == 0 or (name == "wide" and pm[b] != 1000):       # (wide: the rows whose 1000-permille reference the table holds)
                continue
            want = refs[b] if pm[b] == 1000 else ref.reference_row(host[b, :n[b]], rate_in, rate_out, 1000)
            worst = max(worst, float(np.abs(new[i, :n_new[i]] - want).max()))
        print("resample at 1000 permille, %s: max |error| %.3g" % (name, worst))
        assert worst < ref.BOUND, (name, worst)


# ------------------------------------------------------------------------------------------------ AudioProcessor
def _write_wav(path, x, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.astype("<i2").tobytes())


def test_process_files_with_per_row_factors(tmp_path):
    """WAV and FLAC files at 16 and 22.05 kHz, a factor per row: lengths and features are those of process_signal on the
    oracle-resampled waveform (rate conversion and speed change in one pass); without factors nothing changes."""
    from flac_writer import write_flac
    from oracle import frontend as ofe
    from rnn_speech_amd.audioprocessor import AudioProcessor, DEFAULT_LOAD_SR
    rng = np.random.RandomState(5)
    files, sigs = [], []
    for i, (sr, kind) in enumerate([(16000, "wav"), (16000, "flac"), (22050, "wav"), (22050, "flac"), (16000, "wav")]):
        n = int(sr * (0.3 + 0.05 * i))
        t = np.arange(n) / float(sr)
        x = np.round((0.4 * np.sin(2 * np.pi * (300 + 100 * i) * t) + 0.05 * rng.randn(n)) * 20000).astype(np.int64)
        path = str(tmp_path / ("u%d.%s" % (i, kind)))
        if kind == "wav":
            _write_wav(path, x, sr)
        else:
            write_flac(path, x, sr, 16, blocksize=4096, plan=[{"kind": "fixed2", "porder": 3}])
        files.append(path)
        sigs.append((x.astype(np.float32) / np.float32(32768), sr))
    speeds = [900, 1100, 1000, 1100, 1000]           # row 2 is a copy row beside an interpolated one at the same rate
    ap = AudioProcessor(120, "mfcc", n_mfcc=40)
    feat, lengths = ap.process_files(files, rows=6, speed_permille=speeds)
    assert feat.shape == (120, 6, 40) and lengths[5] == 0 and not feat[:, 5].any()
    for i, (s, sr) in enumerate(sigs):
        if ref.is_copy(sr, DEFAULT_LOAD_SR, speeds[i]):
            ref_sig = s
        else:
            ref_sig = ofe.resample_kaiser_best(s, sr * speeds[i], DEFAULT_LOAD_SR * 1000).astype(np.float32)
        assert len(ref_sig) == ref.n_total(len(s), sr, DEFAULT_LOAD_SR, speeds[i])
        ref_feat, ref_len = ap.process_signal(ref_sig, DEFAULT_LOAD_SR)
        assert lengths[i] == ref_len, i
        got = feat[:min(ref_len, 120), i].cpu().numpy()
        assert np.abs(got - ref_feat).max() < 2e-2 * max(1.0, np.abs(ref_feat).max()), i
    plain, plain_len = ap.process_files(files, rows=6)
    same, same_len = ap.process_files(files, rows=6, speed_permille=None)
    assert plain_len == same_len and np.array_equal(bits(plain.cpu().numpy()), bits(same.cpu().numpy()))
    assert lengths[2] == plain_len[2] and np.array_equal(bits(feat[:, 2].cpu().numpy()), bits(plain[:, 2].cpu().numpy()))
    unit, unit_len = ap.process_files(files, speed_permille=[1000] * len(files))       # a factor of 1 is no factor: the same kernel, the same bits
    bare, bare_len = ap.process_files(files)
    assert unit_len == bare_len and np.array_equal(bits(unit.cpu().numpy()), bits(bare.cpu().numpy()))
    # in-memory signals at one rate: the factor alone
    sig16 = [s for s, sr in sigs if sr == 16000]
    fb, lb = ap.process_batch(sig16, 16000, speed_permille=[1100, 1000, 900])
    for i, s in enumerate(sig16):
        pm = [1100, 1000, 900][i]
        want_sig = s if pm == 1000 else ofe.resample_kaiser_best(s, 16000 * pm, 16000 * 1000).astype(np.float32)
        ref_feat, ref_len = ap.process_signal(want_sig, 16000)
        assert lb[i] == ref_len
        assert np.abs(fb[:min(ref_len, 120), i].cpu().numpy() - ref_feat).max() < 2e-2 * max(1.0, np.abs(ref_feat).max()), i
    with pytest.raises(ValueError):
        ap.process_files(files, speed_permille=[1000] * 4)
    with pytest.raises(ValueError):
        ap.process_files(files, speed_permille=[1000] * 4 + [2500])


# ------------------------------------------------------------------------------------------------ a config-built training dataset
TEXTS = ["hello there", "it'll do", "so it is"]
FACTORS = [900, 1000, 1100]


def _config(tmp_path, on, seed):
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / ("ckpt_%d" % on)), 1)
    for old, new in (("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 3"),
                     ("n_mfcc : 40", "n_mfcc : 20"), ("train_decoder : beam", "train_decoder : greedy")):
        assert old in src
        src = src.replace(old, new, 1)
    if on:
        src = src.replace("speed_perturb_factors :\n", "speed_perturb_factors : 0.9, 1.0, 1.1\n", 1)
        src = src.replace("speed_perturb_seed : 0\n", "speed_perturb_seed : %d\n" % seed, 1)
    else:                                         # a config.ini written before the keys existed
        src = "\n".join(l for l in src.splitlines() if not l.startswith("speed_perturb_"))
    cfg = tmp_path / ("config_%d.ini" % on)
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    items, counts = [], []
    for i, (txt, seconds) in enumerate(zip(TEXTS, (0.4, 0.5, 0.6))):
        path = str(tmp_path / ("u%d.wav" % i))
        x = np.round(ref.signal(int(seconds * 16000), 16000, 50 + i) * 20000)
        if not os.path.exists(path):
            _write_wav(path, x, 16000)
        items.append([path, txt, seconds])
        counts.append(len(x))
    return hp, items, counts


def _draws(seed, serial):
    return [ref.draw(seed << 32, (serial << 32) | pos, FACTORS) for pos in range(len(TEXTS))]


def test_training_dataset_from_config_follows_the_draw(tmp_path):
    import stt
    from models.AcousticModel import Session
    from rnn_speech_amd import lib
    seed = next(s for s in range(1, 200) if len(set(_draws(s, 0))) == 3 and _draws(s, 0) != _draws(s, 1))
    frames = lambda n: lib.load().amdspeech_frontend_num_frames(0, n, 22050)      # noqa: E731
    batches = {}
    for on in (1, 0):
        hp, items, counts = _config(tmp_path, on, seed)
        assert (hp["speed_perturb_factors"], hp["speed_perturb_seed"]) == ((FACTORS, seed) if on else ([], 0))
        stt.build_audio_processor(hp)
        sess = Session()
        model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:2])
        try:
            train, test = t_it.dataset, v_it.dataset
            assert train._speed == ((tuple(FACTORS), seed) if on else None) and test._speed is None
            for _ in range(2):                    # two passes: the second draws afresh
                serial = train._epoch[0]
                (feat, lengths, _), = list(train.batches())
                speeds = _draws(seed, serial) if on else [1000] * 3
                assert list(lengths) == [frames(ref.n_total(n, 16000, 22050, pm)) for n, pm in zip(counts, speeds)], (on, serial)
                batches.setdefault(on, []).append((feat.cpu().numpy(), list(lengths)))
            (ftest, ltest, _), = list(test.batches())         # the test dataset is unperturbed
            assert list(ltest)[:2] == [frames(ref.n_total(n, 16000, 22050, 1000)) for n in counts[:2]]
            if on:
                assert batches[1][0][1] != batches[1][1][1]
                loss, err, step, exhausted = model.run_train_step(sess, 1, 1.0)
                assert step == 1 and np.isfinite(loss)
                model.engine.check()
            else:                                 # keys absent: bit-identical to a dataset built without the argument
                plain = stt.AcousticModel.build_dataset(items, 3, 90, 12, "mfcc", hp["char_map"], n_mfcc=20)
                (fp, lp, _), = list(plain.batches())
                for f, l in batches[0]:
                    assert l == list(lp) and np.array_equal(bits(f), bits(fp.cpu().numpy()))
        finally:
            model.close()
