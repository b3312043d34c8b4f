"""Noise and reverberation augmentation on the GPU (csrc/augment.hip) against the float64 oracle of tests/noise_reverb_ref.py: the
reverberation within the rounding bound of an L-term f32 sum, poison past every input row and in the output buffer, bit-exact copy
rows; the sums of squares; the mix; then the layers above up to a config-built training dataset."""
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_reverb_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ reverberation
def _reverb(name):
    from rnn_speech_amd import ops
    n, idx, host, bank, taps, delays, refs = ref.built_reverb(name)
    out = torch.full(host.shape, float("nan"), device="cuda")
    got = ops.reverb_rows(torch.from_numpy(host).cuda(), n, torch.from_numpy(bank).cuda(), taps, delays, idx, out=out)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(ref.reverb_cases()))
def test_reverb_rows_match_the_float64_oracle(name):
    from rnn_speech_amd import ops
    n, idx, host, bank, taps, delays, refs = ref.built_reverb(name)
    plan = ops.reverb_rows_plan(n, host.shape[1], taps, delays, bank.shape[1], idx)
    assert plan == ref.expected_plan(n, host.shape[1], taps, idx) and plan["tile"] == ref.TILE
    if name == "n_edges":
        assert sorted(set(n)) == [0, 1, ref.TILE - 1, ref.TILE, ref.TILE + 1]
    if name == "delay_past_n":
        assert any(delays[r] >= k > 0 for k, r in zip(n, idx))
    out = _reverb(name)
    worst = 0.0
    for b, (k, r) in enumerate(zip(n, idx)):
        assert not bits(out[b, k:]).any(), (name, b)                                  # +0.0f from n to n_max
        if r < 0:
            assert np.array_equal(bits(out[b, :k]), bits(host[b, :k])), (name, b)      # bit for bit: NaN payloads, -0.0
            continue
        assert not np.isnan(out[b]).any(), (name, b)                                   # nothing at or past n was read
        want, mag = refs[b]
        bound = ref.reverb_bound(taps[r], mag)
        err = np.abs(out[b, :k].astype(np.float64) - want)
        if k:
            worst = max(worst, float((err / bound).max()))
    print("reverb_rows %s: worst |error| / bound %.3g" % (name, worst))
    assert worst <= 1.0, (name, worst)


def test_reverb_two_calls_give_the_same_bits():
    first, second = _reverb("short_taps"), _reverb("short_taps")
    assert np.array_equal(bits(first), bits(second))
    first, second = _reverb("taps_8192"), _reverb("taps_8192")
    assert np.array_equal(bits(first), bits(second))


# ------------------------------------------------------------------------------------------------ sums of squares
def test_row_sumsq_against_fsum_and_twice():
    from rnn_speech_amd import ops
    T = 4096                                        # the reduction's tile; 64 workgroups a row: 64 T + 1 reaches a second round
    n = [0, 1, 255, 257, T - 1, T, T + 1, 64 * T + 1]
    host = np.full((len(n), max(n)), ref.POISON, np.float32)
    for b, k in enumerate(n):
        host[b, :k] = ref.signal(k, b) * (10.0 ** (b - 4))      # magnitudes from 1e-5 to 1e3
    pcm = torch.from_numpy(host).cuda()
    got = ops.row_sumsq(pcm, n).cpu().numpy()
    again = ops.row_sumsq(pcm, n).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), again.view(np.uint64))
    assert got[0] == 0.0 and not np.signbit(got[0])
    worst = 0.0
    for b, k in enumerate(n[1:], 1):
        want = ref.sumsq(host[b, :k])
        worst = max(worst, abs(got[b] - want) / want)
    print("row_sumsq: worst relative error %.3g (2^-45 = %.3g)" % (worst, 2.0 ** -45))
    assert worst <= 2.0 ** -45
    # the bits of a row do not depend on the batch around it
    alone = ops.row_sumsq(pcm[4:5, :n[4] + 3].contiguous(), [n[4]]).cpu().numpy()
    assert alone.view(np.uint64)[0] == got.view(np.uint64)[4]


# ------------------------------------------------------------------------------------------------ noise mix
def _mix_case():
    T = ref.TILE
    clips = [(0.05 * np.random.RandomState(40 + m).randn(k) + 0.01).astype(np.float32) for m, k in enumerate((700, 1, 2 * T + 100, 64))]
    clips.append(np.zeros(32, np.float32))                                            # a clip without energy
    #        n          clip offset snr
    rows = [(2 * T + 1, 0, 699, 0),          # a clip shorter than the row: wrap-around, from its last sample
            (T, 1, 0, -200),                 # len 1
            (T + 1, 2, 2 * T + 99, 600),     # offset len - 1, +60 dB
            (T - 1, 3, 5, 50),
            (300, -1, 0, 0),                 # no noise: unchanged bits (specials)
            (500, 0, 10, 100),               # a silent row: unchanged bits
            (0, 2, 0, 0),                    # no samples
            (200, 4, 3, 100)]                # a silent clip: unchanged bits
    n = [r[0] for r in rows]
    host = np.full((len(rows), max(n) + 2), ref.POISON, np.float32)
    for b, k in enumerate(n):
        host[b, :k] = 0.0 if b == 5 else ref.signal(k, 20 + b)
    host[4, :len(ref.SPECIALS)].view(np.uint32)[:] = ref.SPECIALS
    host[4, len(ref.SPECIALS):300] = ref.signal(300 - len(ref.SPECIALS), 3)
    lens = [len(c) for c in clips]
    bank = np.zeros((len(clips), max(lens)), np.float32)
    for m, c in enumerate(clips):
        bank[m, :len(c)] = c
    return rows, n, host, clips, lens, bank


def test_noise_mix_rows_match_the_oracle_in_place_and_out_of_place():
    from rnn_speech_amd import ops
    rows, n, host, clips, lens, bank = _mix_case()
    idx, offs, snr = [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
    plan = ops.noise_mix_rows_plan(n, host.shape[1], lens, bank.shape[1], idx, offs, snr)
    assert plan == ref.expected_mix_plan(n, host.shape[1], idx)
    dbank = torch.from_numpy(bank).cuda()
    nss = ops.row_sumsq(dbank, lens)
    clean = np.where(np.isnan(host), np.float32(0), host)        # rows 0 .. 3 and 5 .. 7 hold no NaN before n; row 4's specials are not summed
    pcm = torch.from_numpy(host).cuda()
    rss = ops.row_sumsq(torch.from_numpy(clean).cuda(), n)
    out = torch.full(host.shape, float("nan"), device="cuda")
    assert ops.noise_mix_rows(pcm, n, rss, dbank, lens, nss, idx, offs, snr, out=out) is out
    assert np.array_equal(bits(pcm.cpu().numpy()), bits(host))                        # out of place: the input is untouched
    inplace = pcm.clone()
    assert ops.noise_mix_rows(inplace, n, rss, dbank, lens, nss, idx, offs, snr, out=inplace) is inplace
    out, inplace = out.cpu().numpy(), inplace.cpu().numpy()
    worst = 0.0
    for b, (k, m, off, s) in enumerate(rows):
        assert np.array_equal(bits(out[b, :k]), bits(inplace[b, :k])), b              # the same bits either way
        assert not bits(out[b, k:]).any(), b                                          # out of place: +0.0f past n
        assert np.array_equal(bits(inplace[b, k:]), bits(host[b, k:])), b             # in place: left alone
        if m < 0 or b in (5, 6, 7):
            assert np.array_equal(bits(out[b, :k]), bits(host[b, :k])), b             # unchanged bits
            continue
        want, added = ref.reference_mix(host[b, :k], clips[m], off, s, with_parts=True)
        bound = 2.0 ** -22 * np.abs(added) + 2.0 ** -24 * np.abs(want)
        err = np.abs(out[b, :k].astype(np.float64) - want)
        assert not np.isnan(out[b, :k]).any(), b
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        measured = 10 * math.log10(ref.sumsq(host[b, :k]) / k / (ref.sumsq(added) / k))
        if len(clips[m]) == 1:
            assert abs(measured - s / 10.0) < 1e-3, (b, measured)
    print("noise_mix_rows: worst |error| / bound %.3g" % worst)
    assert worst <= 1.0


def test_noise_mix_two_runs_of_the_whole_chain_give_the_same_bits():
    """Determinism: reverberation -> sum of squares -> mix, twice, from fresh buffers."""
    from rnn_speech_amd import ops
    n, idx, host, bank, taps, delays, refs = ref.built_reverb("short_taps")
    clip = (0.05 * np.random.RandomState(9).randn(1, 900)).astype(np.float32)
    B = len(n)

    def chain():
        wet = ops.reverb_rows(torch.from_numpy(host).cuda(), n, torch.from_numpy(bank).cuda(), taps, delays, idx)
        dclip = torch.from_numpy(clip).cuda()
        energy = ops.row_sumsq(wet, n)
        # (row 6, the copy row, carries the specials -- NaN energy: it takes the copy path of the mix, which is part of the contract)
        mixed = ops.noise_mix_rows(wet, n, energy, dclip, [900], ops.row_sumsq(dclip, [900]), [0] * B, [b * 100 for b in range(B)],
                                   [50 + 10 * b for b in range(B)], out=wet)
        return mixed.cpu().numpy(), energy.cpu().numpy()

    (a, ea), (b, eb) = chain(), chain()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ea.view(np.uint64), eb.view(np.uint64))
    assert np.array_equal(bits(a[6, :n[6]]), bits(host[6, :n[6]]))


# ------------------------------------------------------------------------------------------------ AudioProcessor
def _write_wav(path, x, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(x.astype("<i2").tobytes())


def _oracle_augment(sig, bank_rirs, bank_noises, d):
    """The oracle-augmented waveform (float32) of one row under draw d: reverberate (unit-energy response as the bank stores it,
    delay at its largest sample), then mix."""
    rir, noise, offset, snr = d
    x = np.asarray(sig, np.float64)
    if rir >= 0:
        h = bank_rirs[rir].astype(np.float64)
        x = ref.reference_reverb(x, h, int(np.argmax(np.abs(h)))).astype(np.float32).astype(np.float64)
    if noise >= 0:
        x = ref.reference_mix(x, bank_noises[noise], offset, snr)
    return x.astype(np.float32)


def _bank_arrays():
    rirs = [ref.rir(300, 40, 1), ref.rir(33, 0, 2)]
    noises = [(0.05 * np.random.RandomState(70).randn(3000)).astype(np.float32), (0.03 * np.random.RandomState(71).randn(20000)).astype(np.float32)]
    return rirs, noises


def test_process_files_with_per_row_draws(tmp_path):
    """WAV and FLAC files at 16 and 22.05 kHz, a draw per row: the features are those of process_signal on the oracle-augmented
    waveform; without draws nothing changes."""
    from flac_writer import write_flac
    from oracle import frontend as ofe
    from rnn_speech_amd.audioprocessor import AudioProcessor, AugmentBank, DEFAULT_LOAD_SR
    rng = np.random.RandomState(5)
    files, sigs = [], []
    for i, (sr, kind) in enumerate([(16000, "wav"), (16000, "flac"), (22050, "wav"), (22050, "flac"), (16000, "wav")]):
        k = int(sr * (0.3 + 0.05 * i))
        t = np.arange(k) / float(sr)
        x = np.round((0.4 * np.sin(2 * np.pi * (300 + 100 * i) * t) + 0.05 * rng.randn(k)) * 20000).astype(np.int64)
        path = str(tmp_path / ("u%d.%s" % (i, kind)))
        if kind == "wav":
            _write_wav(path, x, sr)
        else:
            write_flac(path, x, sr, 16, blocksize=4096, plan=[{"kind": "fixed2", "porder": 3}])
        files.append(path)
        sigs.append((x.astype(np.float32) / np.float32(32768), sr))
    rirs, noises = _bank_arrays()
    bank = AugmentBank(rirs, noises)
    assert bank.rir_taps == [300, 33] and bank.rir_delay == [40, 0] and bank.noise_len == [3000, 20000]
    stored = bank.rir_bank.cpu().numpy()
    stored = [stored[0, :300], stored[1, :33]]
    want_ss = [ref.sumsq(v) for v in noises]
    assert np.allclose(bank.noise_sumsq.cpu().numpy(), want_ss, rtol=2.0 ** -45, atol=0)
    draws = [(0, 1, 19999, 100), (1, -1, 0, 0), (-1, 0, 7, 50), (0, 0, 2999, 200), (-1, -1, 0, 0)]
    plain_ap = AudioProcessor(120, "mfcc", n_mfcc=40)
    ap = AudioProcessor(120, "mfcc", n_mfcc=40, augment_bank=bank)
    feat, lengths = ap.process_files(files, rows=6, augment=draws)
    assert feat.shape == (120, 6, 40) and lengths[5] == 0 and not feat[:, 5].any()
    plain, plain_len = plain_ap.process_files(files, rows=6)
    for i, (s, sr) in enumerate(sigs):
        at_sr = s if sr == DEFAULT_LOAD_SR else ofe.resample_kaiser_best(s, sr, DEFAULT_LOAD_SR).astype(np.float32)
        ref_feat, ref_len = plain_ap.process_signal(_oracle_augment(at_sr, stored, noises, draws[i]), DEFAULT_LOAD_SR)
        assert lengths[i] == ref_len == plain_len[i], i                               # the length does not change
        got = feat[:min(ref_len, 120), i].cpu().numpy()
        assert np.abs(got - ref_feat).max() < 2e-2 * max(1.0, np.abs(ref_feat).max()), i
        if draws[i][:2] != (-1, -1):                                                  # ... and the augmentation is not a no-op
            assert np.abs(got - plain[:min(ref_len, 120), i].cpu().numpy()).max() > 0.1, i
    assert np.array_equal(bits(feat[:, 4].cpu().numpy()), bits(plain[:, 4].cpu().numpy()))      # an all-off row keeps its bits
    # None, and all-off draws, are bit-identical to a processor without a bank
    for kw in (dict(), dict(augment=None), dict(augment=[(-1, -1, 0, 0)] * 5)):
        same, same_len = ap.process_files(files, rows=6, **kw)
        assert same_len == plain_len and np.array_equal(bits(same.cpu().numpy()), bits(plain.cpu().numpy())), kw
    # in-memory signals at one rate, beside a speed factor: speed -> reverberation -> noise
    sig16 = [s for s, sr in sigs if sr == 16000]
    d16 = [(1, 0, 100, 150), (-1, -1, 0, 0), (0, -1, 0, 0)]
    fb, lb = ap.process_batch(sig16, 16000, speed_permille=[1100, 1000, 900], augment=d16)
    base, base_len = plain_ap.process_batch(sig16, 16000, speed_permille=[1100, 1000, 900])
    for i, s in enumerate(sig16):
        pm = [1100, 1000, 900][i]
        fast = s if pm == 1000 else ofe.resample_kaiser_best(s, 16000 * pm, 16000 * 1000).astype(np.float32)
        ref_feat, ref_len = plain_ap.process_signal(_oracle_augment(fast, stored, noises, d16[i]), 16000)
        assert lb[i] == ref_len == base_len[i]
        assert np.abs(fb[:min(ref_len, 120), i].cpu().numpy() - ref_feat).max() < 2e-2 * max(1.0, np.abs(ref_feat).max()), i
    assert np.array_equal(bits(fb[:, 1].cpu().numpy()), bits(base[:, 1].cpu().numpy()))
    with pytest.raises(ValueError):
        ap.process_files(files, augment=draws + [(0, 0, 0, 0)])                       # more draws than rows
    with pytest.raises(ValueError, match="augment_bank"):
        plain_ap.process_files(files, augment=draws)


# ------------------------------------------------------------------------------------------------ a config-built training dataset
TEXTS = ["hello there", "it'll do", "so it is"]
SNR = (50, 200)


def _config(tmp_path, on, seed):
    from models.SpeechRecognizer import SpeechRecognizer
    from util.hyperparams import read_config_file
    import re
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / ("ckpt_%d" % on)), 1)
    for old, new in (("max_input_seq_length : 1001", "max_input_seq_length : 90"), ("max_target_seq_length : 161", "max_target_seq_length : 12"),
                     ("num_layers : 3", "num_layers : 2"), ("hidden_size : 512", "hidden_size : 64"), ("batch_size : 32", "batch_size : 3"),
                     ("n_mfcc : 40", "n_mfcc : 20"), ("train_decoder : beam", "train_decoder : greedy")):
        assert old in src
        src = src.replace(old, new, 1)
    rirs, noises = _bank_arrays()
    for kind, arrays, scale in (("rirs", rirs, 16000.0), ("noise", noises, 20000.0)):
        os.makedirs(str(tmp_path / kind), exist_ok=True)
        for i, a in enumerate(arrays):                                                # 22,050 Hz: no resampling on the way into the bank
            _write_wav(str(tmp_path / kind / ("%s%d.wav" % (kind, i))), np.round(a * scale), 22050)
    keys = dict(noise_dir=tmp_path / "noise", noise_prob=1, noise_snr_db="5, 20", reverb_dir=tmp_path / "rirs", reverb_prob=1,
                reverb_max_taps=256, augment_seed=seed)
    if on:
        for key, value in keys.items():
            src, count = re.subn(r"^%s :.*$" % key, lambda _: "%s : %s" % (key, value), src, count=1, flags=re.M)
            assert count == 1, key
    else:                                         # a config.ini written before the keys existed
        src = "\n".join(l for l in src.splitlines() if not l.startswith(("noise_", "reverb_", "augment_")))
    cfg = tmp_path / ("config_%d.ini" % on)
    cfg.write_text(src)
    hp = read_config_file(str(cfg))
    reco = SpeechRecognizer(hp["language"])
    hp["char_map"], hp["char_map_length"] = reco.get_char_map(), reco.get_char_map_length()
    items, sigs = [], []
    for i, (txt, seconds) in enumerate(zip(TEXTS, (0.4, 0.5, 0.6))):
        path = str(tmp_path / ("u%d.wav" % i))
        x = np.round(ref.signal(int(seconds * 22050), 50 + i) * 20000)
        if not os.path.exists(path):
            _write_wav(path, x, 22050)
        items.append([path, txt, seconds])
        sigs.append(x.astype(np.float32) / np.float32(32768))
    return hp, items, sigs


def _draws(seed, serial, noise_len):
    return [ref.draw(seed << 32, (serial << 32) | pos, 1000, 2, 1000, noise_len, SNR) for pos in range(len(TEXTS))]


def test_training_dataset_from_config_follows_the_draw(tmp_path):
    import stt
    from models.AcousticModel import Session
    from rnn_speech_amd.audioprocessor import AudioProcessor
    noise_len = [3000, 20000]
    seed = next(s for s in range(1, 200) if len({d[0] for d in _draws(s, 0, noise_len)}) == 2 and len({d[1] for d in _draws(s, 0, noise_len)}) == 2
                and _draws(s, 0, noise_len) != _draws(s, 1, noise_len))
    plain_ap = AudioProcessor(90, "mfcc", n_mfcc=20)
    batches = {}
    for on in (1, 0):
        hp, items, sigs = _config(tmp_path, on, seed)
        assert (hp["augment_seed"], hp["reverb_prob"], hp["noise_prob"]) == ((seed, 1.0, 1.0) if on else (0, 0.0, 0.0))      # (absent: seed 0)
        stt.build_audio_processor(hp)
        sess = Session()
        model, t_it, v_it = stt.build_acoustic_training_rnn(sess, hp, dict(tb_name=None, timeline=False, learn_rate=None), items, items[:2])
        try:
            train, test = t_it.dataset, v_it.dataset
            assert test._augment is None and test.audio.augment_bank is None and (train._augment is not None) == bool(on)
            if on:
                bank = train.audio.augment_bank
                assert train._augment[1:] == (1000, 1000, SNR, seed) and bank.noise_len == noise_len
                assert bank.rir_taps == [256, 33] and bank.rir_delay == [40, 0]          # cut to reverb_max_taps
                rb = bank.rir_bank.cpu().numpy()
                stored = [rb[0, :256], rb[1, :33]]
                assert np.allclose((rb.astype(np.float64) ** 2).sum(1), 1.0, rtol=1e-6)  # unit energy
                nb = bank.noise_bank.cpu().numpy()
                clips = [nb[0, :3000], nb[1, :20000]]
            for _ in range(2):                    # two passes: the second draws afresh
                serial = train._epoch[0]
                (feat, lengths, _), = list(train.batches())
                batches.setdefault(on, []).append((feat.cpu().numpy(), list(lengths)))
                if on:
                    for i, d in enumerate(_draws(seed, serial, noise_len)):
                        ref_feat, ref_len = plain_ap.process_signal(_oracle_augment(sigs[i], stored, clips, d), 22050)
                        assert lengths[i] == ref_len
                        got = feat[:min(ref_len, 90), i].cpu().numpy()
                        assert np.abs(got - ref_feat).max() < 2e-2 * max(1.0, np.abs(ref_feat).max()), (serial, i)
            (ftest, ltest, _), = list(test.batches())         # the validation dataset is untouched
            (fbare, lbare, _), = list(stt.AcousticModel.build_dataset(items[:2], 3, 90, 12, "mfcc", hp["char_map"], n_mfcc=20).batches())
            assert list(ltest) == list(lbare) and np.array_equal(bits(ftest.cpu().numpy()), bits(fbare.cpu().numpy()))
            for i in range(2):
                ref_feat, ref_len = plain_ap.process_signal(sigs[i], 22050)
                assert ltest[i] == ref_len and np.abs(ftest[:min(ref_len, 90), i].cpu().numpy() - ref_feat).max() < 1e-3
            if on:
                assert batches[1][0][1] == batches[1][1][1] and not np.array_equal(bits(batches[1][0][0]), bits(batches[1][1][0]))
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
