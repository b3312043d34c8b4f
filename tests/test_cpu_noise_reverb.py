"""Noise and reverberation augmentation (csrc/augment.hip), everything that needs no GPU: the float64 oracle against numpy's own
convolutions, the SNR of the oracle's mix, the draw of the C ABI against the Python restatement, the plans, what the calls refuse,
the config keys and the dataset's draws."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_reverb_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdspeech_reverb_rows_workspace_bytes", "amdspeech_reverb_rows", "amdspeech_reverb_rows_plan",
         "amdspeech_row_sumsq_workspace_bytes", "amdspeech_row_sumsq", "amdspeech_noise_mix_rows_workspace_bytes",
         "amdspeech_noise_mix_rows", "amdspeech_noise_mix_rows_plan", "amdspeech_augment_draw")


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*values)


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("n, taps, delay", [(300, 1, 0), (300, 2, 1), (257, 33, 16), (100, 200, 199), (100, 200, 0), (1, 5, 2), (64, 64, 63)])
def test_oracle_is_a_shifted_truncated_convolution(n, taps, delay):
    x, h = ref.signal(n, 3).astype(np.float64), ref.rir(taps, delay, 1).astype(np.float64)
    got, mag = ref.reference_reverb(x, h, delay, with_abs=True)
    full = np.convolve(x, h)                                     # full[t + delay] = sum_k h[k] x[t + delay - k]
    want = np.concatenate([full, np.zeros(n + delay)])[delay:delay + n]
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    size = 1 << int(np.ceil(np.log2(n + taps)))
    via_fft = np.fft.irfft(np.fft.rfft(x, size) * np.fft.rfft(h, size), size)
    want_fft = np.concatenate([via_fft[:n + taps - 1], np.zeros(n + delay)])[delay:delay + n]
    assert np.abs(got - want_fft).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (mag >= np.abs(got) - 1e-15).all() and np.array_equal(ref.reference_reverb(x, h, delay), got)


@pytest.mark.parametrize("snr", [-200, -37, 0, 50, 200, 600])
@pytest.mark.parametrize("n, length, offset", [(5000, 700, 699), (900, 4000, 123), (64, 1, 0)])
def test_oracle_mix_has_the_requested_snr(snr, n, length, offset):
    """The gain is defined on the WHOLE clip's mean power, so the SNR is measured against that; with the slice the row actually
    received it holds exactly when the clip is periodic in the row (length 1)."""
    x = ref.signal(n, 11).astype(np.float64)
    noise = (0.05 * np.random.RandomState(length).randn(length) + 0.02).astype(np.float32).astype(np.float64)
    mixed, added = ref.reference_mix(x, noise, offset, snr, with_parts=True)
    assert np.allclose(mixed - x, added, rtol=0, atol=1e-15)
    g = ref.gain(ref.sumsq(x), n, ref.sumsq(noise), length, snr)
    assert np.array_equal(added, g * noise[(offset + np.arange(n)) % length])                       # wrap-around from the offset
    measured = 10 * math.log10((ref.sumsq(x) / n) / (g * g * ref.sumsq(noise) / length))
    assert abs(measured - snr / 10.0) < 1e-9
    if length == 1:
        assert abs(10 * math.log10(ref.sumsq(x) / ref.sumsq(added)) - snr / 10.0) < 1e-9
    assert np.array_equal(ref.reference_mix(np.zeros(10), noise, 0, snr), np.zeros(10))             # a silent row
    assert np.array_equal(ref.reference_mix(x, np.zeros(5), 0, snr), x) and len(ref.reference_mix([], noise, 0, snr)) == 0


# ------------------------------------------------------------------------------------------------ header and bindings
def test_header_bindings_and_plan_structs_agree(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    for struct, cls, want in (("amdspeech_reverb_rows_plan_info", lib.ReverbRowsPlanInfo, ref.expected_plan([1], 1, [1], [0])),
                              ("amdspeech_noise_mix_rows_plan_info", lib.NoiseMixRowsPlanInfo, ref.expected_mix_plan([1], 1, [0]))):
        decl = header.split("typedef struct %s {" % struct)[1].split("}")[0]
        fields = [f.strip() for f in decl.replace("int", "").replace(";", "").split(",")]
        assert fields == [n for n, _ in cls._fields_] == sorted(want, key=fields.index), struct
        assert ctypes.sizeof(cls) == 4 * len(fields)
    for name in NAMES:
        proto = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(lib.PROTOTYPES[name][1]), name
        assert getattr(handle, name) is not None
    for query, per_row in ((handle.amdspeech_reverb_rows_workspace_bytes, 16), (handle.amdspeech_noise_mix_rows_workspace_bytes, 24),
                           (handle.amdspeech_row_sumsq_workspace_bytes, 64 * 8 + 4)):
        assert query(0) == 0 and query(-1) == 0
        for B in (1, 32, 257):
            assert query(B) >= per_row * B and query(B) % 256 == 0
    assert "0x5C000000" in header and "amdspeech_augment_draw" in header


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_is_the_documented_hash(handle):
    from rnn_speech_amd import ops
    noise_len = [1, 700, 22050 * 30, 5]
    checked = 0
    for seed in (0, 1, 0xDEADBEEF << 32, (7 << 32) | 99, 2 ** 64 - 1):
        for index in list(range(400)) + [(e << 32) | p for e in (1, 2, 1000, 2 ** 31) for p in range(100)] + [2 ** 64 - 1]:
            for args in ((500, 3, 500, noise_len, (50, 200)), (1000, 1, 1000, [9], (-200, 600)), (0, 4, 1000, noise_len, (0, 0))):
                got = ops.augment_draw(seed, index, *args)
                assert got == ref.draw(seed, index, *args), (seed, index, args)
                rir, noise, offset, snr = got
                assert -1 <= rir < args[1] and -1 <= noise < len(args[3])
                if noise >= 0:
                    assert 0 <= offset < args[3][noise] and args[4][0] <= snr <= args[4][1]            # the offset is inside the clip
                else:
                    assert (offset, snr) == (0, 0)
                checked += 1
    assert checked > 9000
    assert ops.augment_draw(5, 17, 1000, 0, 1000, [], (50, 200)) == (-1, -1, 0, 0)                    # empty banks: nothing to apply
    assert all(ops.augment_draw(5, i, 1000, 3, 0, [10], (50, 200))[1] == -1 for i in range(50))        # probability 0
    assert all(ops.augment_draw(5, i, 1000, 3, 1000, [10], (50, 200))[0] >= 0 for i in range(50))      # probability 1


@pytest.mark.parametrize("seed", [0, 3 << 32, (12345 << 32) | 678])
def test_draw_frequencies_are_within_four_sigma(seed):
    N, R, noise_len, snr = 20000, 3, [100, 4000, 37, 9], (50, 200)
    draws = [ref.draw(seed, i, 300, R, 700, noise_len, snr) for i in range(N)]

    def within(count, total, p):
        assert abs(count - total * p) <= 4 * math.sqrt(total * p * (1 - p)), (count, total, p)

    with_rir = [d for d in draws if d[0] >= 0]
    with_noise = [d for d in draws if d[1] >= 0]
    within(len(with_rir), N, 0.3)
    within(len(with_noise), N, 0.7)
    within(sum(1 for d in draws if d[0] >= 0 and d[1] >= 0), N, 0.21)                                  # the two decisions are independent
    for r in range(R):
        within(sum(1 for d in with_rir if d[0] == r), len(with_rir), 1.0 / R)
    for m in range(len(noise_len)):
        chosen = [d for d in with_noise if d[1] == m]
        within(len(chosen), len(with_noise), 1.0 / len(noise_len))
        assert all(0 <= d[2] < noise_len[m] for d in chosen)
        within(sum(1 for d in chosen if d[2] < noise_len[m] // 2), len(chosen), (noise_len[m] // 2) / float(noise_len[m]))
    for v in (50, 125, 200):
        within(sum(1 for d in with_noise if d[3] == v), len(with_noise), 1.0 / 151)
    assert {d[3] for d in with_noise} == set(range(50, 201))


def test_ranks_and_epochs_are_decorrelated():
    """Another rank (seed64 = (seed + rank) << 32) or another epoch (index = (epoch << 32) | position) agrees with the first pass
    no more often than independent draws would."""
    N, R, noise_len, snr = 20000, 4, [1000, 1000], (0, 99)
    base = [ref.draw(5 << 32, i, 500, R, 500, noise_len, snr) for i in range(N)]
    for other in ([ref.draw(6 << 32, i, 500, R, 500, noise_len, snr) for i in range(N)],
                  [ref.draw(5 << 32, (1 << 32) | i, 500, R, 500, noise_len, snr) for i in range(N)]):
        for part, p in ((0, 0.25 + 0.25 / R), (1, 0.25 + 0.25 / 2)):          # both off, or both on with the same choice
            same = sum(1 for a, b in zip(base, other) if a[part] == b[part])
            assert abs(same - N * p) <= 4 * math.sqrt(N * p * (1 - p)), (part, same)
        both = [(a, b) for a, b in zip(base, other) if a[1] >= 0 and b[1] >= 0]
        p = 1.0 / 100
        assert abs(sum(1 for a, b in both if a[3] == b[3]) - len(both) * p) <= 4 * math.sqrt(len(both) * p * (1 - p))


# ------------------------------------------------------------------------------------------------ the plans
def test_plans_match_the_restated_plans_without_a_device(handle):
    from rnn_speech_amd import ops
    for name, (rirs, rows, n_max) in ref.reverb_cases().items():
        taps, delays = [r[0] for r in rirs], [r[1] for r in rirs]
        n, idx = [r[0] for r in rows], [r[1] for r in rows]
        plan = ops.reverb_rows_plan(n, n_max, taps, delays, max(taps), idx)
        assert plan == ref.expected_plan(n, n_max, taps, idx), name
        assert plan["tile"] == ref.TILE and plan["lds_bytes"] <= 80 * 1024
    # 32 rows of 10 s at 22.05 kHz: the profile's shape
    for L, lds in ((1024, 16384 + 4352), (4096, 21120 + 16640), (8192, 38016 + 33024)):
        plan = ops.reverb_rows_plan([220500] * 32, 220500, [L], [0], L, [0] * 32)
        assert plan == ref.expected_plan([220500] * 32, 220500, [L], [0] * 32)
        assert (plan["workgroups"], plan["k_chunks"], plan["lds_bytes"], plan["copy_rows"]) == (216 * 32, (L + 62) // 32, lds, 0)
    off = ops.reverb_rows_plan([500, 0], 500, [64], [3], 64, [-1, 0])          # a copy row and an empty row: nothing is filtered
    assert (off["taps"], off["lds_bytes"], off["copy_rows"]) == (0, 0, 1)
    assert ops.reverb_rows_plan([5] * 129, 5, [1], [0], 1, [0] * 129)["meta_launches"] == 2
    mix = ops.noise_mix_rows_plan([0, 2049, 7], 2049, [1, 50], 50, [-1, 1, 0], [0, 49, 0], [0, -200, 600])
    assert mix == ref.expected_mix_plan([0, 2049, 7], 2049, [-1, 1, 0]) and (mix["tiles_per_row"], mix["copy_rows"]) == (3, 1)
    assert ops.noise_mix_rows_plan([5] * 86, 5, [5], 5, [0] * 86, [0] * 86, [0] * 86)["meta_launches"] == 2


# ------------------------------------------------------------------------------------------------ what the calls refuse
def _reverb(handle, n, B, n_max, taps, delays, R, taps_max, idx, plan_only=False, pcm=0x10000, out=0x4000000, bank=0x8000000, ws=0x100):
    from rnn_speech_amd import lib
    info = lib.ReverbRowsPlanInfo()
    rc = handle.amdspeech_reverb_rows_plan(n, B, n_max, taps, delays, R, taps_max, idx, ctypes.byref(info))
    if plan_only:
        return rc
    # the call checks its arguments as the plan does, before it touches a device pointer or the device
    rc2 = handle.amdspeech_reverb_rows(None, pcm, n, B, n_max, bank, taps, delays, R, taps_max, idx, out, ws)
    assert rc2 == rc == -1
    return rc


@pytest.mark.parametrize("n, B, n_max, taps, delays, taps_max, idx, word", [
    ([10], 0, 10, [4], [0], 4, [0], b"bad shape"), ([10], 1, 0, [4], [0], 4, [0], b"bad shape"), ([10], 1, 10, [4], [0], 0, [0], b"bad shape"),
    ([10], 65536, 10, [4], [0], 4, [0], b"above 65535"), ([10], 1, 2 ** 30 + 1, [4], [0], 4, [0], b"above 2^30"),
    ([10], 1, 10, [4], [0], 8193, [0], b"above 8192"), ([10], 1, 10, [0], [0], 4, [0], b"rir_taps[0] = 0"),
    ([10], 1, 10, [5], [0], 4, [0], b"rir_taps[0] = 5"), ([10], 1, 10, [4], [4], 4, [0], b"rir_delay[0] = 4"),
    ([10], 1, 10, [4], [-1], 4, [0], b"rir_delay[0] = -1"), ([11], 1, 10, [4], [0], 4, [0], b"n_samples[0] = 11"),
    ([-1], 1, 10, [4], [0], 4, [0], b"n_samples[0] = -1"), ([10], 1, 10, [4], [0], 4, [1], b"rir_index[0] = 1"),
    ([10], 1, 10, [4], [0], 4, [-2], b"rir_index[0] = -2")])
def test_reverb_plan_and_call_refuse_with_a_message(handle, n, B, n_max, taps, delays, taps_max, idx, word):
    _reverb(handle, _ints(n), B, n_max, _ints(taps), _ints(delays), len(taps), taps_max, _ints(idx))
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()


@pytest.mark.parametrize("n, B, n_max, lens, m_max, idx, offs, snr, word", [
    ([10], 0, 10, [4], 4, [0], [0], [0], b"bad shape"), ([10], 1, 10, [4], 0, [0], [0], [0], b"bad shape"),
    ([10], 65536, 10, [4], 4, [0], [0], [0], b"above 65535"), ([10], 1, 2 ** 30 + 1, [4], 4, [0], [0], [0], b"above 2^30"),
    ([10], 1, 10, [0], 4, [0], [0], [0], b"noise_len[0] = 0"), ([10], 1, 10, [5], 4, [0], [0], [0], b"noise_len[0] = 5"),
    ([11], 1, 10, [4], 4, [0], [0], [0], b"n_samples[0] = 11"), ([10], 1, 10, [4], 4, [1], [0], [0], b"noise_index[0] = 1"),
    ([10], 1, 10, [4], 4, [-2], [0], [0], b"noise_index[0] = -2"), ([10], 1, 10, [4], 4, [0], [4], [0], b"noise_offset[0] = 4"),
    ([10], 1, 10, [4], 4, [0], [-1], [0], b"noise_offset[0] = -1"), ([10], 1, 10, [4], 4, [0], [0], [-201], b"snr_decidb[0] = -201"),
    ([10], 1, 10, [4], 4, [0], [0], [601], b"snr_decidb[0] = 601")])
def test_noise_mix_plan_and_call_refuse_with_a_message(handle, n, B, n_max, lens, m_max, idx, offs, snr, word):
    from rnn_speech_amd import lib
    info = lib.NoiseMixRowsPlanInfo()
    args = (_ints(n), B, n_max, _ints(lens), len(lens), m_max, _ints(idx), _ints(offs), _ints(snr))
    assert handle.amdspeech_noise_mix_rows_plan(*(args + (ctypes.byref(info),))) == -1
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()
    rc = handle.amdspeech_noise_mix_rows(None, 0x10000, args[0], B, n_max, 0x8000000, args[3], 0x100, len(lens), m_max, 0x200, args[6],
                                         args[7], args[8], 0x4000000, 0x300)
    assert rc == -1 and word in handle.amdspeech_last_error(), handle.amdspeech_last_error()


def test_null_pointers_overlap_and_bad_draws_are_refused(handle):
    from rnn_speech_amd import lib, ops
    one, zero = _ints([10]), _ints([0])
    taps = _ints([4])

    def refused(rc, word):
        assert rc == -1 and word in handle.amdspeech_last_error(), handle.amdspeech_last_error()

    rinfo, minfo = lib.ReverbRowsPlanInfo(), lib.NoiseMixRowsPlanInfo()
    refused(handle.amdspeech_reverb_rows_plan(None, 1, 10, taps, zero, 1, 4, zero, ctypes.byref(rinfo)), b"null")
    refused(handle.amdspeech_reverb_rows_plan(one, 1, 10, taps, zero, 1, 4, None, ctypes.byref(rinfo)), b"null")
    refused(handle.amdspeech_reverb_rows_plan(one, 1, 10, taps, zero, 1, 4, zero, None), b"null")
    refused(handle.amdspeech_noise_mix_rows_plan(one, 1, 10, None, 1, 4, zero, zero, zero, ctypes.byref(minfo)), b"null")
    refused(handle.amdspeech_noise_mix_rows_plan(one, 1, 10, taps, 1, 4, zero, zero, zero, None), b"null")
    # the calls: null device pointers, then ranges that overlap (nothing is dereferenced, nothing is launched)
    rv = lambda pcm, bank, out, ws: handle.amdspeech_reverb_rows(None, pcm, one, 1, 10, bank, taps, zero, 1, 4, zero, out, ws)   # noqa: E731
    for args in ((None, 0x8000, 0x4000, 0x100), (0x1000, None, 0x4000, 0x100), (0x1000, 0x8000, None, 0x100), (0x1000, 0x8000, 0x4000, None)):
        refused(rv(*args), b"null")
    refused(rv(0x1000, 0x8000, 0x1000, 0x100), b"pcm and out overlap")              # in place is not possible for a filter
    refused(rv(0x1000, 0x8000, 0x1000 + 36, 0x100), b"pcm and out overlap")         # 10 floats = 40 bytes
    refused(rv(0x1000 + 36, 0x8000, 0x1000, 0x100), b"pcm and out overlap")
    refused(rv(0x1000, 0x8000, 0x8000 + 12, 0x100), b"rir_bank and out overlap")
    mx = lambda pcm, out, bank=0x8000, ns=0x100, rs=0x200, ws=0x300: handle.amdspeech_noise_mix_rows(   # noqa: E731
        None, pcm, one, 1, 10, bank, taps, ns, 1, 4, rs, zero, zero, zero, out, ws)
    for kw in (dict(pcm=None, out=0x4000), dict(pcm=0x1000, out=None), dict(pcm=0x1000, out=0x4000, bank=None),
               dict(pcm=0x1000, out=0x4000, ns=None), dict(pcm=0x1000, out=0x4000, rs=None), dict(pcm=0x1000, out=0x4000, ws=None)):
        refused(mx(**kw), b"null")
    refused(mx(0x1000, 0x1000 + 4), b"overlap in part")                              # in place (out == pcm) is allowed, a shifted range is not
    refused(mx(0x1000 + 36, 0x1000), b"overlap in part")
    refused(mx(0x1000, 0x8000 + 8), b"noise_bank and out overlap")
    refused(handle.amdspeech_row_sumsq(None, None, one, 1, 10, 0x100, 0x200), b"null")
    refused(handle.amdspeech_row_sumsq(None, 0x1000, one, 1, 10, None, 0x200), b"null")
    refused(handle.amdspeech_row_sumsq(None, 0x1000, one, 0, 10, 0x100, 0x200), b"bad shape")
    refused(handle.amdspeech_row_sumsq(None, 0x1000, one, 65536, 10, 0x100, 0x200), b"above 65535")
    refused(handle.amdspeech_row_sumsq(None, 0x1000, _ints([11]), 1, 10, 0x100, 0x200), b"n_samples[0] = 11")
    out = _ints([0] * 4)
    refused(handle.amdspeech_augment_draw(0, 0, 500, 1, 500, 1, one, 50, 200, None), b"null")
    refused(handle.amdspeech_augment_draw(0, 0, 500, 1, 500, 1, None, 50, 200, out), b"null noise_len")
    refused(handle.amdspeech_augment_draw(0, 0, 1001, 1, 500, 1, one, 50, 200, out), b"outside 0 .. 1000")
    refused(handle.amdspeech_augment_draw(0, 0, 500, 1, -1, 1, one, 50, 200, out), b"outside 0 .. 1000")
    refused(handle.amdspeech_augment_draw(0, 0, 500, -1, 500, 1, one, 50, 200, out), b"negative bank size")
    refused(handle.amdspeech_augment_draw(0, 0, 500, 1, 500, 1, zero, 50, 200, out), b"noise_len[0] = 0")
    for lo, hi in ((200, 50), (-201, 0), (0, 601)):
        refused(handle.amdspeech_augment_draw(0, 0, 500, 1, 500, 1, one, lo, hi, out), b"snr range")
    with pytest.raises(lib.AmdSpeechError):
        ops.augment_draw(0, 0, 500, 1, 500, [0], (50, 200))
    with pytest.raises(ValueError):
        ops.reverb_rows_plan([10, 10], 10, [4], [0], 4, [0])                          # an index per row


# ------------------------------------------------------------------------------------------------ the config keys
KEYS = ("noise_dir", "noise_prob", "noise_snr_db", "noise_max_seconds", "reverb_dir", "reverb_prob", "reverb_max_taps", "augment_bank_mb",
        "augment_seed")
DEFAULTS = dict(noise_dir="", noise_prob=0.0, noise_snr_db=(50, 200), noise_max_seconds=30.0, reverb_dir="", reverb_prob=0.0,
                reverb_max_taps=8192, augment_bank_mb=256, augment_seed=0)


def _config(tmp_path, **values):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for key, value in values.items():
        src, count = re.subn(r"^%s :.*$" % key, lambda _: "%s : %s" % (key, value), src, count=1, flags=re.M)
        assert count == 1, key
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    return str(cfg), src


def test_config_keys_parse_default_to_off_and_are_not_structural(tmp_path):
    import stt
    from util.hyperparams import read_config_file, HyperParameterHandler
    cfg, src = _config(tmp_path)
    off = read_config_file(cfg)
    assert {k: off[k] for k in KEYS} == dict(DEFAULTS, augment_seed=1) and stt.augment_option(off) is None      # (config.ini ships seed 1)
    bare = tmp_path / "bare.ini"                 # a config.ini written before the keys existed
    bare.write_text("\n".join(l for l in src.splitlines() if not l.startswith(KEYS)))
    assert not re.search(r"^(%s) :" % "|".join(KEYS), bare.read_text(), re.M)
    d = read_config_file(str(bare))
    assert {k: d[k] for k in KEYS} == DEFAULTS and stt.augment_option(d) is None and stt.augment_option({}) is None
    # a directory without a probability, or a probability without a directory: off, and the directory is not even read
    assert stt.augment_option(dict(off, noise_dir="/nowhere", reverb_dir="/nowhere")) is None
    assert stt.augment_option(dict(off, noise_prob=1.0, reverb_prob=1.0)) is None
    on = read_config_file(_config(tmp_path, noise_dir="/data/noise", noise_prob="0.5", noise_snr_db="-5.04, 12.5", noise_max_seconds="7.5",
                                  reverb_dir=" /data/rirs ", reverb_prob="1", reverb_max_taps="4096", augment_bank_mb="64",
                                  augment_seed=str(2 ** 32 - 1))[0])
    assert {k: on[k] for k in KEYS} == dict(noise_dir="/data/noise", noise_prob=0.5, noise_snr_db=(-50, 125), noise_max_seconds=7.5,
                                            reverb_dir="/data/rirs", reverb_prob=1.0, reverb_max_taps=4096, augment_bank_mb=64,
                                            augment_seed=2 ** 32 - 1)
    assert read_config_file(_config(tmp_path, noise_snr_db="10")[0])["noise_snr_db"] == (100, 100)
    for key, text in (("noise_prob", "1.01"), ("noise_prob", "-0.1"), ("noise_prob", "nan"), ("noise_prob", "often"), ("reverb_prob", "2"),
                      ("reverb_prob", "inf"), ("noise_snr_db", "20, 5"), ("noise_snr_db", "-21, 5"), ("noise_snr_db", "5, 61"),
                      ("noise_snr_db", "5, 10, 20"), ("noise_snr_db", "loud"), ("noise_snr_db", ""), ("noise_max_seconds", "0"),
                      ("noise_max_seconds", "nan"), ("reverb_max_taps", "0"), ("reverb_max_taps", "8193"), ("reverb_max_taps", "4096.5"),
                      ("augment_bank_mb", "0"), ("augment_seed", "-1"), ("augment_seed", str(2 ** 32))):
        with pytest.raises(ValueError, match=key):
            read_config_file(_config(tmp_path, **{key: text})[0])

    # not structural: a checkpoint stays usable when only these keys change, either way round
    h = HyperParameterHandler(_config(tmp_path)[0])
    assert not h.check_changed(off) and not h.check_changed(on)
    legacy = {k: v for k, v in off.items() if k not in KEYS}
    assert not h.check_changed(legacy)
    h.save_params(on)
    assert not h.check_changed(off) and not h.check_changed(legacy)
    assert h.check_changed(dict(on, frame_stack=3))      # (the handler still sees a structural key)


# ------------------------------------------------------------------------------------------------ the bank and the dataset
class _Bank(object):
    """What the dataset reads of an AugmentBank, without a device."""

    def __init__(self, taps, noise_len):
        self.rir_bank = object() if taps else None
        self.noise_bank = object() if noise_len else None
        self.rir_taps, self.rir_delay, self.noise_len = list(taps), [0] * len(taps), list(noise_len)


def test_bank_checks_its_input_before_it_touches_a_device():
    from rnn_speech_amd.audioprocessor import AugmentBank
    with pytest.raises(ValueError, match="no energy"):
        AugmentBank(rirs=[np.zeros(16)], device="cpu")
    with pytest.raises(ValueError, match="empty"):
        AugmentBank(noises=[np.zeros(0)], device="cpu")
    with pytest.raises(ValueError, match="reverb_max_taps"):
        AugmentBank(rirs=[np.ones(4)], max_taps=8193, device="cpu")
    with pytest.raises(ValueError, match="augment_bank_mb"):
        AugmentBank(noises=[np.ones(300000, np.float32)], bank_mb=1, device="cpu")
    with pytest.raises(ValueError, match="augment_bank_mb"):
        AugmentBank(rirs=[np.ones(8192)] * 33, bank_mb=1, device="cpu")
    bank = AugmentBank(rirs=[np.array([0.0, 3.0, -4.0, 0.0, 1.0]), np.array([0.5] * 9)], max_taps=4, device="cpu")      # (no noise: no launch)
    assert bank.rir_taps == [4, 4] and bank.rir_delay == [2, 0] and bank.noise_bank is None and bank.nbytes == 32
    host = bank.rir_bank.numpy().astype(np.float64)
    assert np.allclose(host[0], np.array([0.0, 3.0, -4.0, 0.0]) / 5.0, rtol=1e-7) and np.allclose((host * host).sum(1), 1.0, rtol=1e-6)
    assert AugmentBank.list_files(os.path.join(ROOT, "tests", "golden")) == []


def test_dataset_draws_are_reproducible_and_differ_between_passes(handle):
    from models.AcousticModel import AcousticModel
    items = [((np.zeros(4000, np.float32), 16000), "ab")] * 7
    args = (3, 90, 12, "mfcc", ["a", "b", "_"])
    bank = _Bank([64, 200], [700, 9, 22050])
    with pytest.raises(ValueError, match="feature_cache_mb"):
        AcousticModel.build_dataset(items, *args, feature_cache_mb=4, augment=(bank, 500, 500, (50, 200), 5))
    for bad in ((bank, 1001, 0, (50, 200), 0), (bank, 0, -1, (50, 200), 0), (bank, 500, 500, (200, 50), 0), (bank, 500, 500, (-201, 0), 0)):
        with pytest.raises(ValueError):
            AcousticModel.build_dataset(items, *args, augment=bad)
    assert AcousticModel.build_dataset(items, *args).augment_draws(0) is None
    assert AcousticModel.build_dataset(items, *args, augment=(bank, 0, 0, (50, 200), 5)).augment_draws(0) is None       # both off
    assert AcousticModel.build_dataset(items, *args, augment=(_Bank([], []), 500, 500, (50, 200), 5)).augment_draws(0) is None
    assert AcousticModel.build_dataset(items, *args, feature_cache_mb=4, augment=(bank, 0, 0, (50, 200), 5))._cache == {}
    half = AcousticModel.build_dataset(items, *args, augment=(_Bank([64], []), 1000, 1000, (50, 200), 5))              # no clips: reverb only
    assert all(d[0] == 0 and d[1] == -1 for d in half.augment_draws(0))

    seed, snr = 5, (50, 200)
    ds = AcousticModel.build_dataset(items, *args, augment=(bank, 600, 700, snr, seed), prefetch=0)
    assert ds.audio.augment_bank is bank
    want = lambda serial, rank=0: [ref.draw((seed + rank) << 32, (serial << 32) | pos, 600, 2, 700, bank.noise_len, snr)   # noqa: E731
                                   for pos in range(len(items))]
    assert ds.augment_draws(0) == want(0) and ds.augment_draws(1) == want(1) and want(0) != want(1)
    assert ds.augment_draws(3, start=2, count=3) == want(3)[2:5] and ds.augment_draws(3, start=6, count=3) == want(3)[6:]

    def passes(dataset, seen):
        def process_batch(sig, sr, t_max=None, staged=None, speed_permille=None, augment=None):
            staged[0].claimed = False                  # (the staging block goes back to its pool: nothing is uploaded here)
            seen.append((speed_permille, augment))
            return None, [0] * 3
        dataset.audio.process_batch = process_batch
        return dataset

    seen = []
    list(passes(ds, seen).batches())
    assert [a for _, a in seen] == [want(0)[0:3], want(0)[3:6], want(0)[6:]] and all(s is None for s, _ in seen)
    del seen[:]
    sibling = passes(ds.with_items(items[::-1]), seen)
    assert sibling.audio.augment_bank is bank                                              # with_items shares the bank
    list(sibling.batches())
    list(ds.batches())
    flat = [v for _, chunk in seen for v in chunk]
    assert flat[:7] == want(1) and flat[7:] == want(2)                                     # the counter is shared: passes 1 and 2
    both = AcousticModel.build_dataset(items, *args, augment=(bank, 600, 700, snr, seed), speed_perturb=([900, 1100], 5), prefetch=2)
    seen2 = []
    list(passes(both, seen2).batches())
    assert [v for _, chunk in seen2 for v in chunk] == want(0)                             # a second run draws the same; prefetch or not
    assert seen2[0][0] == both.speed_draws(0, 0, 3) and seen2[2][0] == both.speed_draws(0, 6, 1) + [1000, 1000]      # beside the speeds

    from rnn_speech_amd import dataparallel
    before = dataparallel.current()
    try:
        dataparallel.set_current(dataparallel.Group(3, 4))
        ranked = AcousticModel.build_dataset(items, *args, augment=(bank, 600, 700, snr, seed), prefetch=2)
    finally:
        dataparallel.set_current(before)
    assert ranked._rank == 3 and ranked.augment_draws(0) == want(0, rank=3) != want(0) and ranked.with_items(items)._rank == 3


def test_with_items_copies_and_shares_the_parents_objects(handle):
    """A with_items sibling is a copy over a new item list: the processor, the cache, the counters, the rank and the normalised
    options are the parent's own objects, nothing is rebuilt."""
    from models.AcousticModel import AcousticModel
    items = [((np.zeros(4000, np.float32), 16000), "ab")] * 4 + [((np.zeros(3000, np.float32), 16000), "b")]
    bank = _Bank([64, 200], [700, 9])
    ds = AcousticModel.build_dataset(items, 3, 90, 12, "mfcc", ["a", "b", "_"], speed_perturb=([900, 1000, 1100], 5),
                                     augment=(bank, 600, 700, (50, 200), 5), prefetch=0)
    seen = []

    def process_batch(sig, sr, t_max=None, staged=None, speed_permille=None, augment=None):
        staged[0].claimed = False                  # (the staging block goes back to its pool: nothing is uploaded here)
        seen.append((speed_permille, augment))
        return None, [0] * 3
    ds.audio.process_batch = process_batch
    sibling = ds.with_items(items[::-1])
    assert type(sibling) is type(ds) and sibling is not ds and sibling.audio is ds.audio
    for name in ("_cache", "_room", "_epoch", "_rank", "_speed", "_augment"):
        assert getattr(sibling, name) is getattr(ds, name), name
    assert [t for _, t in sibling.items] == ["b"] + ["ab"] * 4 and [t for _, t in ds.items] == ["ab"] * 4 + ["b"]      # the parent keeps its list
    assert (sibling.batch_size, sibling.U, sibling.T, sibling.char_map, sibling.prefetch) == (3, 12, 90, ds.char_map, 0)
    list(sibling.batches())                        # the sibling's pass goes through the parent's processor and counter
    assert ds._epoch[0] == 1 and len(seen) == 2
    assert [s for s, _ in seen] == [ds.speed_draws(0, 0, 3), ds.speed_draws(0, 3, 2) + [1000]]
    assert [a for _, a in seen] == [ds.augment_draws(0, 0, 3), ds.augment_draws(0, 3, 2)]


def test_off_leaves_the_calls_as_they_were(handle):
    """Without the option batches() makes the very call it made before the option existed (no `augment` keyword), and the
    processor's stage returns the tensor it was given."""
    from models.AcousticModel import AcousticModel
    from rnn_speech_amd.audioprocessor import AudioProcessor
    items = [((np.zeros(4000, np.float32), 16000), "ab")] * 2
    ds = AcousticModel.build_dataset(items, 3, 90, 12, "mfcc", ["a", "b", "_"], prefetch=0)
    seen = []

    def process_batch(sig, sr, t_max=None, staged=None, speed_permille=None):
        staged[0].claimed = False
        seen.append(speed_permille)
        return None, [0] * 3
    ds.audio.process_batch = process_batch
    list(ds.batches())
    assert seen == [None] and ds.audio.augment_bank is None
    ap = AudioProcessor(90, "mfcc", device="cpu")
    token = object()
    assert ap._augmented(token, [1], None) is token
    with pytest.raises(ValueError, match="augment_bank"):
        ap._augmented(np.zeros((1, 4)), [1], [(0, -1, 0, 0)])
