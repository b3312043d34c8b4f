"""The per-row resampler / speed perturbation (csrc/frontend.hip: resample_rows_kernel), everything that needs no GPU: header and
bindings, the lengths, the plan and the draw of the C ABI against the Python restatement, what the calls refuse, the config keys and
the dataset's draws."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import speed_perturb_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amdspeech_resample_rows_num_samples", "amdspeech_resample_rows_workspace_bytes", "amdspeech_resample_rows",
         "amdspeech_resample_rows_plan", "amdspeech_speed_perturb_draw")


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


def _ints(values):
    return (ctypes.c_int * max(len(values), 1))(*values)


# ------------------------------------------------------------------------------------------------ header and bindings
def test_header_bindings_and_plan_struct_agree(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_resample_rows_plan_info {")[1].split("}")[0]
    fields = [f.strip() for f in decl.replace("int", "").replace(";", "").split(",")]
    assert fields == [n for n, _ in lib.ResampleRowsPlanInfo._fields_] == sorted(ref.expected_plan([1], [1000], 1, 1), key=fields.index)
    assert ctypes.sizeof(lib.ResampleRowsPlanInfo) == 4 * len(fields)
    for name in NAMES:
        proto = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(lib.PROTOTYPES[name][1]), name
        assert getattr(handle, name) is not None
    assert handle.amdspeech_resample_rows_workspace_bytes(0) == 0
    assert handle.amdspeech_resample_rows_workspace_bytes(32) >= ref.NWIN * 8 + 2 * 32 * 4      # the (win, delta) pairs and 2 B values
    assert "speed perturbation is amdspeech_resample_rows" in header                            # SpecAugment's section points here


# ------------------------------------------------------------------------------------------------ lengths
def test_num_samples_is_the_integer_formula(handle):
    from rnn_speech_amd import ops
    for name, (rate_in, rate_out, rows, _) in ref.cases().items():
        for n, pm in rows:
            assert ops.resample_rows_num_samples(n, rate_in, rate_out, pm) == ref.n_total(n, rate_in, rate_out, pm), (name, n, pm)
    rng = np.random.RandomState(3)
    rates = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)
    for _ in range(20000):
        n = int(rng.randint(0, 2 ** 31 - 1)) if rng.rand() < 0.3 else int(rng.randint(0, 500000))
        rate_in, rate_out = int(rates[rng.randint(len(rates))]), int(rates[rng.randint(len(rates))])
        pm = int(rng.randint(ref.PERMILLE_MIN, ref.PERMILLE_MAX + 1))
        want = ref.n_total(n, rate_in, rate_out, pm)
        got = handle.amdspeech_resample_rows_num_samples(n, rate_in, rate_out, pm)
        if n * rate_out * 1000 >= 2 ** 53 or want > 2 ** 31 - 1:
            assert got < 0, (n, rate_in, rate_out, pm)
        else:
            assert got == want, (n, rate_in, rate_out, pm)
            if pm == 1000 or rng.rand() < 0.05:      # at 1000 permille: the existing resampler's length
                assert handle.amdspeech_resample_rows_num_samples(n, rate_in, rate_out, 1000) == \
                    handle.amdspeech_resample_num_samples(n, rate_in, rate_out)
    # the copy rule's rows keep their length; the padding is 0 or 1 sample
    assert ops.resample_rows_num_samples(3000, 44100, 22050, 500) == 3000 and ref.is_copy(44100, 22050, 500)
    for name, (rate_in, rate_out, rows, _) in ref.cases().items():
        for n, pm in rows:
            assert 0 <= ref.n_total(n, rate_in, rate_out, pm) - ref.n_interp(n, rate_in, rate_out, pm) <= 1, (name, n, pm)


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_matches_the_restated_plan_without_a_device(handle):
    from rnn_speech_amd import ops
    seen = set()
    for name, (rate_in, rate_out, rows, _) in ref.cases().items():
        n, pm = [r[0] for r in rows], [r[1] for r in rows]
        plan = ops.resample_rows_plan(n, pm, max(max(n), 1), rate_in, rate_out)
        assert plan == ref.expected_plan(n, pm, rate_in, rate_out), name
        seen.add((plan["any_copy"], plan["meta_launches"], plan["tiles_per_row"] > 1))
    assert {(1, 1, True), (0, 1, True), (0, 3, False)} <= seen          # copy rows, several tiles, the 512-value chunks
    head = ops.resample_rows_plan([160000] * 32, [900, 1000, 1100, 1000] * 8, 160000, 16000, 22050)      # the headline shape
    assert head == ref.expected_plan([160000] * 32, [900, 1000, 1100, 1000] * 8, 16000, 22050)
    span = int(1023 * 1.1 / 1.378125) + 132                          # the slowest rows reach furthest: 948 samples
    assert head["tile"] == 1024 and head["workgroups"] == -(-245000 // 1024) * 32 and head["span_max"] == span == 948
    assert head["table_chunk"] == 4097 and head["lds_bytes"] == 4 * span + 8 * 4097
    worst = ops.resample_rows_plan([100000], [2000], 100000, 44100 * 4, 22050)                         # the 1/16 bound
    assert worst["span_max"] == 1023 * 16 + 2 * 1024 + 4 and worst["lds_bytes"] == 106456 < 160 * 1024
    off = ops.resample_rows_plan([500, 0], [1000, 1000], 500, 22050, 22050)                             # nothing interpolates
    assert off["span_max"] == off["table_chunk"] == off["lds_bytes"] == 0 and off["any_copy"] == 1
    wide = ops.resample_rows_plan([10] * 257, [1000] * 257, 10, 16000, 22050, out_max=1030)
    assert (wide["tiles_per_row"], wide["workgroups"], wide["meta_launches"]) == (2, 514, 2)


# ------------------------------------------------------------------------------------------------ the draw
def test_draw_is_the_documented_hash(handle):
    from rnn_speech_amd import ops

    def mix(v):
        v = np.uint32(v)
        with np.errstate(over="ignore"):
            v ^= v >> np.uint32(16)
            v *= np.uint32(0x7feb352d)
            v ^= v >> np.uint32(15)
            v *= np.uint32(0x846ca68b)
            v ^= v >> np.uint32(16)
        return v

    for seed, index in ((0, 0), (0x1234567890ABCDEF, (5 << 32) | 77), ((7 << 32) | 99, 2 ** 64 - 1)):      # worked from the formula
        with np.errstate(over="ignore"):
            idx = np.uint32(index & 0xFFFFFFFF) + np.uint32(index >> 32) * np.uint32(0x9E3779B1)
            a = mix(idx ^ np.uint32(seed & 0xFFFFFFFF))
            b = mix(a + np.uint32(0x5B000000) * np.uint32(0x9e3779b9) + np.uint32(seed >> 32))
        factors = [900, 1000, 1100, 1250, 800]
        assert ops.speed_perturb_draw(seed, index, factors) == ref.draw(seed, index, factors) == factors[((int(b) >> 8) * 5) >> 24]
    rng = np.random.RandomState(9)
    for _ in range(2000):
        seed, index = int(rng.randint(0, 2 ** 62)) * 3, int(rng.randint(0, 2 ** 62)) * 3
        factors = [int(v) for v in rng.randint(500, 2001, rng.randint(1, 9))]
        assert ops.speed_perturb_draw(seed, index, factors) == ref.draw(seed, index, factors)


@pytest.mark.parametrize("seed", [0, 0x1234567890ABCDEF, (7 << 32) | 99])
@pytest.mark.parametrize("count", [2, 3, 5, 8])
def test_draw_is_uniform_within_four_sigma(handle, seed, count):
    N = 30000
    factors = [600 + 100 * i for i in range(count)]
    arr = _ints(factors)
    got = np.array([handle.amdspeech_speed_perturb_draw(seed, i, arr, count) for i in range(N)])
    assert all(got[i] == ref.draw(seed, i, factors) for i in range(0, N, 97))
    sigma = np.sqrt(N * (1.0 / count) * (1.0 - 1.0 / count))
    for f in factors:
        assert abs(int((got == f).sum()) - N / count) <= 4 * sigma, (seed, count, f, int((got == f).sum()))
    # epochs and positions do not alias: the same positions of another epoch draw another sequence
    other = [handle.amdspeech_speed_perturb_draw(seed, (1 << 32) | i, arr, count) for i in range(200)]
    assert other != list(got[:200])


# ------------------------------------------------------------------------------------------------ refusals
def _call(handle, n, pm, B, n_max, rate_in, rate_out, out_max, pcm=1 << 20, out=1 << 30, ws=1 << 40):
    return handle.amdspeech_resample_rows(None, ctypes.c_void_p(pcm), n, pm, B, n_max, rate_in, rate_out, ctypes.c_void_p(out), out_max,
                                          ctypes.c_void_p(ws))


REFUSALS = [
    # n, permille, B, n_max, rate_in, rate_out, out_max, word
    ([10], [1000], 0, 10, 16000, 22050, 100, b"bad shape"),
    ([10], [1000], 1, 0, 16000, 22050, 100, b"bad shape"),
    ([10], [1000], 1, 10, 0, 22050, 100, b"bad shape"),
    ([10], [1000], 1, 10, 16000, -1, 100, b"bad shape"),
    ([10], [1000], 1, 10, 16000, 22050, 0, b"bad shape"),
    ([-1], [1000], 1, 10, 16000, 22050, 100, b"n_samples[0] = -1"),
    ([10, 11], [1000, 1000], 2, 10, 16000, 22050, 100, b"n_samples[1] = 11"),
    ([10], [499], 1, 10, 16000, 22050, 100, b"speed_permille[0] = 499"),
    ([10, 10], [1000, 2001], 2, 10, 16000, 22050, 100, b"speed_permille[1] = 2001"),
    ([10], [1000], 1, 10, 16000, 22050, 13, b"needs 14 samples"),              # ceil(10 * 1.378125) = 14
    ([10], [900], 1, 10, 16000, 22050, 15, b"needs 16 samples"),
    ([10], [1000], 1, 10, 1000, 22050, 1000, b"outside 1/16"),                 # ratio 22.05
    ([1000], [2000], 1, 1000, 200000, 22050, 1000, b"outside 1/16"),           # ratio 1 / 18.1
    ([10], [1000], 1, 2 ** 31 - 1, 16000, 48000, 100, b"2^53"),               # n_max * num = 1.03e17
]


@pytest.mark.parametrize("n,pm,B,n_max,rate_in,rate_out,out_max,word", REFUSALS)
def test_plan_and_call_refuse_with_a_message(handle, n, pm, B, n_max, rate_in, rate_out, out_max, word):
    from rnn_speech_amd import lib
    info = lib.ResampleRowsPlanInfo()
    assert handle.amdspeech_resample_rows_plan(_ints(n), _ints(pm), B, n_max, rate_in, rate_out, out_max, ctypes.byref(info)) == -1
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()
    # the call checks its arguments as the plan does, before it touches a device pointer or the device
    assert _call(handle, _ints(n), _ints(pm), B, n_max, rate_in, rate_out, out_max) == -1
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()


def test_null_pointers_overlap_and_bad_queries_are_refused(handle):
    from rnn_speech_amd import lib, ops
    n, pm, info = _ints([10]), _ints([1000]), lib.ResampleRowsPlanInfo()

    def refused(rc, word):
        assert rc == -1 and word in handle.amdspeech_last_error(), handle.amdspeech_last_error()

    refused(handle.amdspeech_resample_rows_plan(None, pm, 1, 10, 16000, 22050, 100, ctypes.byref(info)), b"null")
    refused(handle.amdspeech_resample_rows_plan(n, None, 1, 10, 16000, 22050, 100, ctypes.byref(info)), b"null")
    refused(handle.amdspeech_resample_rows_plan(n, pm, 1, 10, 16000, 22050, 100, None), b"null")
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, pcm=0), b"null")
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, out=0), b"null")
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, ws=0), b"null")
    refused(_call(handle, None, pm, 1, 10, 16000, 22050, 100), b"null")
    refused(_call(handle, n, None, 1, 10, 16000, 22050, 100), b"null")
    base = 1 << 20
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, pcm=base, out=base), b"overlap")
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, pcm=base, out=base + 36), b"overlap")          # the last input word
    refused(_call(handle, n, pm, 1, 10, 16000, 22050, 100, pcm=base + 396, out=base), b"overlap")         # the last output word
    refused(handle.amdspeech_resample_rows_plan(_ints([1] * 4), _ints([1000] * 4), 65536, 10, 16000, 22050, 100, ctypes.byref(info)), b"65535")
    refused(handle.amdspeech_resample_rows_num_samples(-1, 16000, 22050, 1000), b"negative")
    refused(handle.amdspeech_resample_rows_num_samples(10, 0, 22050, 1000), b"rate")
    refused(handle.amdspeech_resample_rows_num_samples(10, 16000, 22050, 2001), b"2001")
    refused(handle.amdspeech_resample_rows_num_samples(2 ** 31 - 1, 8000, 48000, 500), b"2^53")
    refused(handle.amdspeech_resample_rows_num_samples(2 ** 30, 8000, 8000, 500), b"fit an int")
    refused(handle.amdspeech_speed_perturb_draw(0, 0, None, 3), b"null")
    refused(handle.amdspeech_speed_perturb_draw(0, 0, _ints([1000]), 0), b"count 0")
    refused(handle.amdspeech_speed_perturb_draw(0, 0, _ints([1000] * 9), 9), b"count 9")
    refused(handle.amdspeech_speed_perturb_draw(0, 0, _ints([1000, 2500]), 2), b"2500")
    with pytest.raises(lib.AmdSpeechError):
        ops.speed_perturb_draw(0, 0, [])
    with pytest.raises(lib.AmdSpeechError):
        ops.resample_rows_num_samples(10, 16000, 22050, 100)
    with pytest.raises(ValueError):
        ops.resample_rows_plan([10, 10], [1000], 10, 16000, 22050)                                         # a factor per row


def test_uniform_resample_is_the_per_row_call_at_1000_permille(handle):
    """amdspeech_resample plans as amdspeech_resample_rows does (a ratio outside 1/16 .. 16 is refused before anything is launched)
    and shares its workspace size and, at 1000 permille, its lengths."""
    for rate_in, rate_out in ((1000, 17000), (17000, 1000)):
        rc = handle.amdspeech_resample(None, ctypes.c_void_p(1 << 20), _ints([10]), 1, 10, rate_in, rate_out, ctypes.c_void_p(1 << 30),
                                       1000, ctypes.c_void_p(1 << 40))
        assert rc == -1 and b"outside 1/16" in handle.amdspeech_last_error(), handle.amdspeech_last_error()
    for B in (1, 256, 257):
        assert handle.amdspeech_resample_workspace_bytes(B) == handle.amdspeech_resample_rows_workspace_bytes(B) > 0
    for rate_in, rate_out in ((16000, 22050), (44100, 22050), (8000, 22050), (22050, 16000)):
        for n in range(3001):
            assert handle.amdspeech_resample_num_samples(n, rate_in, rate_out) == \
                handle.amdspeech_resample_rows_num_samples(n, rate_in, rate_out, 1000) == ref.n_total(n, rate_in, rate_out, 1000)


# ------------------------------------------------------------------------------------------------ the config keys
def _config(tmp_path, factors=None, seed=None, cache=None):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, value in (("speed_perturb_factors :\n", factors), ("speed_perturb_seed : 0\n", seed), ("feature_cache_mb : 0\n", cache)):
        assert old in src
        if value is not None:
            src = src.replace(old, "%s : %s\n" % (old.split(" :")[0], value), 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    return str(cfg), src


def test_config_keys_parse_default_to_off_and_are_not_structural(tmp_path):
    import stt
    from util.hyperparams import read_config_file, HyperParameterHandler
    cfg, src = _config(tmp_path)
    off = read_config_file(cfg)
    assert off["speed_perturb_factors"] == [] and off["speed_perturb_seed"] == 0 and stt.speed_perturb_option(off) is None
    bare = tmp_path / "bare.ini"                 # a config.ini written before the keys existed
    bare.write_text("\n".join(l for l in src.splitlines() if not l.startswith("speed_perturb_")))
    d = read_config_file(str(bare))
    assert d["speed_perturb_factors"] == [] and d["speed_perturb_seed"] == 0
    assert stt.speed_perturb_option(d) is None and stt.speed_perturb_option({}) is None
    for text in ("1.0", " 1 ", "1.0004"):        # 1.0 alone: off
        assert read_config_file(_config(tmp_path, factors=text)[0])["speed_perturb_factors"] == []
    on = read_config_file(_config(tmp_path, factors="0.9, 1.0,1.1", seed=11)[0])
    assert on["speed_perturb_factors"] == [900, 1000, 1100] and stt.speed_perturb_option(on) == ([900, 1000, 1100], 11)
    assert read_config_file(_config(tmp_path, factors="0.8996, 1.0004, 2, .5")[0])["speed_perturb_factors"] == [900, 1000, 2000, 500]
    assert len(read_config_file(_config(tmp_path, factors=", ".join(["1.1"] * 8))[0])["speed_perturb_factors"]) == 8
    for bad in (dict(factors="0.9, fast"), dict(factors="0.4994"), dict(factors="2.001"), dict(factors="nan"), dict(factors="inf"), dict(factors="1.0, -inf"),
                dict(factors=", ".join(["1.1"] * 9)), dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            read_config_file(_config(tmp_path, **bad)[0])

    # not structural: a checkpoint stays usable when only these keys change, either way round
    h = HyperParameterHandler(_config(tmp_path)[0])
    assert not h.check_changed(off) and not h.check_changed(on)
    legacy = {k: v for k, v in off.items() if not k.startswith("speed_perturb_")}
    assert not h.check_changed(legacy)
    h.save_params(on)
    assert not h.check_changed(off) and not h.check_changed(legacy)
    assert h.check_changed(dict(on, frame_stack=3))      # (the handler still sees a structural key)


# ------------------------------------------------------------------------------------------------ the dataset
def test_dataset_draws_are_reproducible_and_differ_between_passes(handle):
    from models.AcousticModel import AcousticModel
    items = [((np.zeros(4000, np.float32), 16000), "ab")] * 7
    args = (3, 90, 12, "mfcc", ["a", "b", "_"])
    with pytest.raises(ValueError, match="feature_cache_mb"):
        AcousticModel.build_dataset(items, *args, feature_cache_mb=4, speed_perturb=([900, 1000, 1100], 5))
    for bad in (([], 0), ([400], 0), ([1000] * 9, 0)):
        with pytest.raises(ValueError):
            AcousticModel.build_dataset(items, *args, speed_perturb=bad)
    assert AcousticModel.build_dataset(items, *args).speed_draws(0) is None
    assert AcousticModel.build_dataset(items, *args, speed_perturb=([1000], 5)).speed_draws(0) is None      # 1.0 alone: off
    assert AcousticModel.build_dataset(items, *args, feature_cache_mb=4, speed_perturb=([1000], 5))._cache == {}

    factors, seed = [900, 1000, 1100], 5
    ds = AcousticModel.build_dataset(items, *args, speed_perturb=(factors, seed), prefetch=0)
    want = lambda serial: [ref.draw(((seed + 0) << 32), (serial << 32) | pos, factors) for pos in range(len(items))]   # noqa: E731
    assert ds.speed_draws(0) == want(0) and ds.speed_draws(1) == want(1) and want(0) != want(1)
    assert ds.speed_draws(3, start=2, count=3) == want(3)[2:5] and ds.speed_draws(3, start=6, count=3) == want(3)[6:]

    # what batches() hands the device path: one pass after another, shared with the with_items siblings, the same in a second run
    def passes(dataset, seen):
        def process_batch(sig, sr, t_max=None, staged=None, speed_permille=None):
            staged[0].claimed = False                  # (the staging block goes back to its pool: nothing is uploaded here)
            seen.append(speed_permille)
            return None, [0] * 3
        dataset.audio.process_batch = process_batch
        return dataset

    seen = []
    passes(ds, seen)
    assert len(list(ds.batches())) == 3
    assert seen == [want(0)[0:3], want(0)[3:6], want(0)[6:] + [1000, 1000]]              # a short last batch: padding rows at 1000
    del seen[:]
    sibling = passes(ds.with_items(items[::-1]), seen)
    list(sibling.batches())
    list(ds.batches())
    flat = [v for chunk in seen for v in chunk]
    assert flat[:7] == want(1) and flat[9:16] == want(2) and flat[:7] != want(0)      # the counter is shared: passes 1 and 2
    again, seen2 = AcousticModel.build_dataset(items, *args, speed_perturb=(factors, seed), prefetch=2), []
    passes(again, seen2)
    list(again.batches())
    assert [v for chunk in seen2 for v in chunk][:7] == want(0)                            # a second run draws the same; prefetch or not

    # the data-parallel rank enters the seed's high word; it is resolved when the dataset is built, on the caller's thread
    from rnn_speech_amd import dataparallel
    before = dataparallel.current()
    try:
        dataparallel.set_current(dataparallel.Group(3, 4))
        ranked = AcousticModel.build_dataset(items, *args, speed_perturb=(factors, seed), prefetch=2)
    finally:
        dataparallel.set_current(before)
    want3 = [ref.draw((seed + 3) << 32, pos, factors) for pos in range(len(items))]
    assert ranked._rank == 3 and ranked.speed_draws(0) == want3 != want(0)
    seen3 = []
    list(passes(ranked, seen3).batches())                                                 # (the current group is rank 0 again)
    assert [v for chunk in seen3 for v in chunk][:7] == want3
    assert ranked.with_items(items)._rank == 3
