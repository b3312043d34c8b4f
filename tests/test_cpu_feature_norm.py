"""Feature normalisation (csrc/feature_norm.hip), everything that needs no GPU: the reference's own properties, planted faults
against the bound, the plan query and what the C ABI refuses, the corpus statistics, the config keys and the plumbing."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_norm_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


# ------------------------------------------------------------------------------------------------ the reference and the table
def test_reference_is_the_textbook_formula():
    rng = np.random.RandomState(3)
    x = (rng.randn(12, 3, 5) * [1, 10, 0.1, 3, 1] + [0, -1131, 5, 100, -7]).astype(np.float32)
    lengths = [12, 7, 20]
    y = ref.normalise(x, lengths)
    for b, n in enumerate([12, 7, 12]):
        rows = x[:n, b].astype(np.float64)
        assert np.allclose(y[:n, b], (rows - rows.mean(axis=0)) / rows.std(axis=0), rtol=1e-12, atol=1e-12)      # numpy's std: population
        assert np.array_equal(y[n:, b], x[n:, b].astype(np.float64))
        assert np.allclose(y[:n, b].mean(axis=0), 0, atol=1e-9) and np.allclose(y[:n, b].var(axis=0), 1, rtol=1e-9)
    only_mean = ref.normalise(x, lengths, norm_vars=False)
    assert np.allclose(only_mean[:7, 1], x[:7, 1].astype(np.float64) - x[:7, 1].astype(np.float64).mean(axis=0))
    m = ref.moments(x, lengths)
    assert m.shape == (3, 2, 5) and np.allclose(m[1, 1], 7 * x[:7, 1].astype(np.float64).var(axis=0))
    one = ref.normalise(x, [1, 0, 1])               # n = 1: zeros;  n = 0: untouched
    assert np.all(one[0, 0] == 0) and np.array_equal(one[:, 1], x[:, 1].astype(np.float64))


def test_the_table_covers_what_the_kernels_can_get_wrong():
    plans = {name: ref.expected_plan(c[2], c[0], c[1]) for name, c in ref.CASES.items()}
    for name, c in ref.CASES.items():
        assert all(plans[name][f] == v for f, v in c[4].items()), (name, plans[name])
        x, lengths = ref.case_inputs(name)
        assert x.shape == (c[1], c[2], c[0]) and x.dtype == np.float32
        bits = x.view(np.uint32)
        for b, n in enumerate(ref.clipped(lengths, c[1])):      # poison from each row's length on and nowhere else
            assert np.all(bits[n:, b] == ref.POISON) and not np.any(np.isnan(x[:n, b]))
        for d in ref.const_dims(name):
            assert all(len(set(x[:n, b, d])) <= 1 for b, n in enumerate(ref.clipped(lengths, c[1])))
    assert {p["vec"] for p in plans.values()} == {1, 4}
    assert {ref.CASES[n][0] for n in plans if plans[n]["vec"] == 4} >= {40, 120, 4096} and ref.CASES["vec1_d13"][0] == 13
    assert any(p["split"] > 1 for p in plans.values()) and any(p["meta_by_copy"] for p in plans.values())
    assert list(ref.case_lengths("vec4_d40")) == [0, 1, 2, 70, 77]
    assert ref.CASES["wide_batch"][1:3] == (3, 257) and ref.CASES["widest_frame"][:3] == (4096, 2, 1)
    # the offset dim: mean -1131, deviation 3, 1001 frames, more than one slice;  the tiny dim: a variance below the floor
    x, lengths = ref.case_inputs("offset_split")
    mean, var = ref.statistics(x, lengths)
    assert x.shape[0] == 1001 and plans["offset_split"]["split"] > 1
    assert abs(mean[0, 0] + 1131) < 0.5 and abs(np.sqrt(var[0, 0]) - 3) < 0.3 and 0 < var[0, 2] < ref.VAR_FLOOR
    assert np.all(var[:, 1] == 0)
    x, lengths = ref.case_inputs("tiny_variance")
    assert 0 < ref.statistics(x, lengths)[1][0, 2] < ref.VAR_FLOOR
    # rows beyond the grid's cap, columns beyond a workgroup's lanes in both variants
    assert ref.CASES["row_stride"][2] > ref.MAX_WGS
    assert ref.CASES["widest_frame"][0] // 4 > ref.THREADS and ref.CASES["vec1_columns"][0] > ref.THREADS


@pytest.mark.parametrize("name", ref.GPU_CASES)
def test_clean_emulation_meets_the_bound(name):
    """The scheme amdspeech.h documents, emulated in numpy, meets every check of its case."""
    D, t_in, B, _, _ = ref.CASES[name]
    x, lengths = ref.case_inputs(name)
    plan = ref.expected_plan(B, D, t_in)
    verdict = ref.judge(ref.emulate(x, lengths, plan["split"], ref.slots_for(D)), x, lengths, ref.const_dims(name))
    assert ref.passes(verdict), verdict
    only_mean = ref.judge(ref.emulate(x, lengths, plan["split"], ref.slots_for(D), norm_vars=False), x, lengths, ref.const_dims(name),
                          norm_vars=False)
    assert ref.passes(only_mean), only_mean


@pytest.mark.parametrize("fault", sorted(ref.FAULTS))
def test_planted_fault_misses_its_case(fault):
    """Each way to get the kernel wrong, planted in the emulation, fails the checks of the case written for it.  The padding holds
    the planted NaN, and a finite word where the fault would recompute the NaN into itself."""
    name = ref.FAULTS[fault]
    D, t_in, B, _, _ = ref.CASES[name]
    plan = ref.expected_plan(B, D, t_in)
    x, lengths = ref.case_inputs(name, ref.PAD_FINITE if fault == "padding_written" else ref.POISON)
    clean = ref.judge(ref.emulate(x, lengths, plan["split"], ref.slots_for(D)), x, lengths, ref.const_dims(name))
    assert ref.passes(clean), clean
    verdict = ref.judge(ref.emulate(x, lengths, plan["split"], ref.slots_for(D), fault=fault), x, lengths, ref.const_dims(name))
    assert not ref.passes(verdict), verdict
    if fault == "padding_written":
        assert not verdict["pad_intact"]
    else:
        assert verdict["ratio"] > 100, verdict            # none of them is a near miss


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_structs_match_the_header_and_prototypes_are_listed(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_feature_norm_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.FeatureNormPlanInfo._fields_]
    assert [n for n, _ in lib.FeatureNormPlanInfo._fields_] == ["vec", "split", "workgroups", "lds_bytes", "meta_by_copy", "workspace_bytes"]
    assert ctypes.sizeof(lib.FeatureNormPlanInfo) == 4 * len(lib.FeatureNormPlanInfo._fields_)
    decl = header.split("typedef struct amdspeech_feature_norm_desc {")[1].split("}")[0]
    ints, real = [part.strip() for part in decl.strip().rstrip(";").split(";")]
    assert [n.strip() for n in ints.replace("int", "").split(",")] == ["mode", "norm_vars"] and real.split() == ["double", "var_floor"]
    assert [n for n, _ in lib.FeatureNormDesc._fields_] == ["mode", "norm_vars", "var_floor"]
    assert ctypes.sizeof(lib.FeatureNormDesc) == 16 and lib.FeatureNormDesc.var_floor.offset == 8
    for i, mode in enumerate(lib.FEATURE_NORM_MODES):
        assert "#define AMDSPEECH_FEATURE_NORM_%s %d\n" % (mode.upper(), i) in header
    for name in ("amdspeech_feature_norm_plan", "amdspeech_feature_moments", "amdspeech_feature_norm"):
        assert name in lib.PROTOTYPES and getattr(handle, name) is not None


@pytest.mark.parametrize("name", ref.GPU_CASES)
def test_plan_query_equals_the_expected_plan(handle, name):
    from rnn_speech_amd import ops
    D, t_in, B, _, fields = ref.CASES[name]
    for mode in ref.MODES:
        plan = ops.feature_norm_plan(B, D, t_in, mode)
        assert plan == ref.expected_plan(B, D, t_in, mode), (name, mode, plan)
    assert all(ops.feature_norm_plan(B, D, t_in)[f] == v for f, v in fields.items())


def test_plan_at_other_shapes(handle):
    from rnn_speech_amd import ops
    rng = np.random.RandomState(11)
    for _ in range(300):
        B, D, t_in = int(rng.randint(1, 3000)), int(rng.randint(1, 4097)), int(rng.randint(1, 4000))
        want = ref.expected_plan(B, D, t_in)
        if want is not None:
            assert ops.feature_norm_plan(B, D, t_in) == want, (B, D, t_in)
    head = ops.feature_norm_plan(32, 40, 1001)                   # the headline shape: 15 slices of 67 frames, 480 workgroups
    assert (head["split"], head["workgroups"], head["vec"], head["workspace_bytes"]) == (15, 480, 4, 32 * 31 * 40 * 8)
    assert ops.feature_norm_plan(32, 120, 1001)["split"] == 16
    assert ops.feature_norm_plan(32, 40, 1001, "global")["workspace_bytes"] == 0
    assert ops.feature_norm_plan(32, 40, 1001, "none")["workgroups"] == 0
    assert ops.feature_norm_plan(1, 40, 100000)["split"] == 511       # 512 slices of ceil(100000 / 512) = 196 frames: the last would be empty
    assert ops.feature_norm_plan(4096, 40, 3510)["workgroups"] == 2048      # the grid is capped
    with pytest.raises(ValueError):
        ops.feature_norm_plan(32, 40, 1001, "sliding")


REFUSALS = [    # B, D, t_in, mode, a word of the message
    (0, 40, 10, 1, b"bad shape"), (4, 0, 10, 1, b"bad shape"), (4, 40, 0, 1, b"bad shape"), (-1, 40, 10, 1, b"bad shape"),
    (65536, 4, 32768, 1, b"bad shape"), (4, 4097, 10, 1, b"4096"), (4, 40, 10, 3, b"mode"), (4, 40, 10, -1, b"mode"),
]


@pytest.mark.parametrize("B,D,t_in,mode,word", REFUSALS)
def test_plan_and_calls_refuse_a_bad_shape(handle, B, D, t_in, mode, word):
    from rnn_speech_amd import lib
    info = lib.FeatureNormPlanInfo()
    assert handle.amdspeech_feature_norm_plan(B, D, t_in, mode, ctypes.byref(info)) != 0
    assert word in handle.amdspeech_last_error()
    n = (ctypes.c_int * max(min(B, 8), 1))()
    x, ws, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    desc = lib.FeatureNormDesc(mode, 1, 1e-10)
    assert handle.amdspeech_feature_norm(None, x, n, B, D, t_in, ctypes.byref(desc), ws, ws) != 0
    assert word in handle.amdspeech_last_error()
    if word != b"mode":
        assert handle.amdspeech_feature_moments(None, x, n, B, D, t_in, ws, out) != 0
        assert word in handle.amdspeech_last_error()


def test_calls_refuse_bad_arguments(handle):
    """Everything is checked before a pointer is followed or the device is touched."""
    from rnn_speech_amd import lib
    B, D, t_in = 4, 40, 10
    n = (ctypes.c_int * B)(10, 3, 0, 15)
    x, ws, table, out = 1 << 20, 1 << 30, 1 << 29, 1 << 31
    P = ctypes.c_void_p

    def desc(mode=1, norm_vars=1, floor=1e-10):
        return ctypes.byref(lib.FeatureNormDesc(mode, norm_vars, floor))

    def refused(word, rc):
        assert rc != 0 and word in handle.amdspeech_last_error(), handle.amdspeech_last_error()

    norm, mom = handle.amdspeech_feature_norm, handle.amdspeech_feature_moments
    refused(b"null", handle.amdspeech_feature_norm_plan(B, D, t_in, 1, None))
    refused(b"null", norm(None, None, n, B, D, t_in, desc(), None, P(ws)))
    refused(b"null", norm(None, P(x), None, B, D, t_in, desc(), None, P(ws)))
    refused(b"null", norm(None, P(x), n, B, D, t_in, None, None, P(ws)))
    refused(b"null workspace", norm(None, P(x), n, B, D, t_in, desc(1), None, None))
    refused(b"null table", norm(None, P(x), n, B, D, t_in, desc(2), None, P(ws)))
    refused(b"null", mom(None, None, n, B, D, t_in, P(ws), P(out)))
    refused(b"null workspace", mom(None, P(x), n, B, D, t_in, None, P(out)))
    refused(b"null moments", mom(None, P(x), n, B, D, t_in, P(ws), None))
    for floor in (0.0, -1e-10, float("nan"), float("inf")):
        refused(b"var_floor", norm(None, P(x), n, B, D, t_in, desc(1, 1, floor), None, P(ws)))
    # a base off by one word at D % 4 == 0 is refused; at D % 4 != 0 there is nothing to align (the next check speaks)
    refused(b"16-byte aligned", norm(None, P(x + 4), n, B, D, t_in, desc(), None, P(ws)))
    refused(b"16-byte aligned", norm(None, P(x + 4), n, B, D, t_in, desc(2), P(table), None))
    refused(b"16-byte aligned", mom(None, P(x + 8), n, B, D, t_in, P(ws), P(out)))
    refused(b"8-byte aligned", norm(None, P(x + 4), n, B, 13, t_in, desc(), None, P(ws + 4)))
    refused(b"8-byte aligned", norm(None, P(x), n, B, D, t_in, desc(2), P(table + 4), None))
    refused(b"8-byte aligned", mom(None, P(x), n, B, D, t_in, P(ws), P(out + 4)))
    bad = (ctypes.c_int * B)(10, -1, 0, 15)
    refused(b"negative", norm(None, P(x), bad, B, D, t_in, desc(), None, P(ws)))
    refused(b"negative", mom(None, P(x), bad, B, D, t_in, P(ws), P(out)))
    # mode 0 launches nothing and says so with AMDSPEECH_OK: no device is needed
    assert norm(None, P(x), n, B, D, t_in, desc(0), None, None) == 0


def test_ops_check_their_arguments_before_any_device_call(handle):
    import torch
    from rnn_speech_amd import ops
    with pytest.raises(ValueError):
        ops.feature_norm(torch.zeros(4, 2, 40), [4, 4], "utterance")                    # a host tensor
    with pytest.raises(ValueError):
        ops.feature_moments(np.zeros((4, 2, 40), np.float32), [4, 4])
    with pytest.raises(ValueError):
        ops.feature_norm(torch.zeros(4, 2, 40), [4, 4], "sliding")
    x = torch.zeros(4, 2, 40)
    assert ops.feature_norm(x, [4, 4], "none") is x                                     # off: the tensor itself, nothing else happens


# ------------------------------------------------------------------------------------------------ corpus statistics
def _moments_of(batches):
    return [(ref.moments(x, n), n, x.shape[0]) for x, n in batches]


def test_feature_stats_merge_equals_numpy_over_all_frames(tmp_path):
    from rnn_speech_amd.feature_norm import FeatureStats, describe
    rng = np.random.RandomState(2)
    D = 7
    batches = []
    for t_in, lengths in ((30, [30, 12, 0, 41]), (18, [5, 18, 1])):
        x = (rng.randn(t_in, len(lengths), D) * [1, 3, 0.01, 10, 1, 1, 1] + [-1131, 5, 0, 100, 0, 1, -2]).astype(np.float32)
        batches.append((x, lengths))
    frames = np.concatenate([x[:min(n, x.shape[0]), b] for x, lengths in batches for b, n in enumerate(lengths)]).astype(np.float64)
    desc = describe("mfcc", D, 16000, D)
    stats = FeatureStats(desc)
    for m, n, t_in in _moments_of(batches):
        assert stats.merge_moments(m, n, t_in) is stats
    assert stats.count == len(frames) == 30 + 12 + 30 + 5 + 18 + 1
    assert np.allclose(stats.mean, frames.mean(axis=0), rtol=1e-13, atol=1e-13 * np.abs(frames).max())
    assert np.allclose(stats.var, frames.var(axis=0), rtol=1e-10, atol=0)
    again = FeatureStats(desc)                           # deterministic: the same rows in the same order give the same bits
    for m, n, t_in in _moments_of(batches):
        again.merge_moments(m, n, t_in)
    assert np.array_equal(again.mean, stats.mean) and np.array_equal(again.M2, stats.M2)
    with pytest.raises(ValueError):
        stats.merge_moments(np.zeros((2, 2, D + 1)), [1, 1], 4)

    # save / load and the table
    path = str(tmp_path / "stats.npz")
    stats.save(path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    with np.load(path) as z:
        assert set(z.files) == {"count", "mean", "var", "signal_processing", "n_mfcc", "sample_rate", "width"}
        assert np.array_equal(z["mean"], stats.mean) and np.array_equal(z["var"], stats.var) and float(z["count"]) == stats.count
    back = FeatureStats.load(path, desc)
    assert back.description == desc and back.count == stats.count and np.array_equal(back.mean, stats.mean)
    assert np.allclose(back.var, stats.var, rtol=1e-15)
    table = back.table_numpy()
    assert table.dtype == np.float64 and table.shape == (2, D)
    assert np.array_equal(table[0], back.mean) and np.array_equal(table[1], 1.0 / np.sqrt(np.maximum(back.var, 1e-10)))
    assert np.array_equal(back.table_numpy(norm_vars=False)[1], np.ones(D))
    assert back.table_numpy(var_floor=1e6)[1].max() == 1e-3
    with pytest.raises(ValueError):
        back.table_numpy(var_floor=0.0)

    # a file taken from other features is refused, with both descriptions in the message; so is one of no frames
    for other in (describe("mfcc", 40, 16000, D), describe("mfcc", D, 22050, D), describe("fbank", D, 16000, D), describe("mfcc", D, 16000, 8)):
        with pytest.raises(ValueError) as err:
            FeatureStats.load(path, other)
        assert repr(other) in str(err.value) and repr(desc) in str(err.value)
    empty = str(tmp_path / "empty.npz")
    FeatureStats(desc).save(empty)
    with pytest.raises(ValueError, match="no frame"):
        FeatureStats.load(empty, desc)
    with pytest.raises(ValueError, match="no frame"):
        FeatureStats(desc).table_numpy()
    junk = str(tmp_path / "junk.npz")
    np.savez(open(junk, "wb"), mean=np.zeros(3))
    with pytest.raises(ValueError, match="lacks"):
        FeatureStats.load(junk)
    assert describe("fbank", 20, 16000, 120)["n_mfcc"] == 0 == describe("fbank", 40, 16000, 120)["n_mfcc"]      # n_mfcc shapes mfcc only


# ------------------------------------------------------------------------------------------------ config keys and plumbing
def _config(tmp_path, **keys):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for key, (old, new) in keys.items():
        assert "%s : %s\n" % (key, old) in src
        src = src.replace("%s : %s\n" % (key, old), "%s : %s\n" % (key, new), 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    return str(cfg), src


def test_config_ini_keeps_the_strings_other_tests_replace():
    """Existing tests rewrite config.ini by replacing the FIRST occurrence of a string: the new comment block must not hold one."""
    src = open(os.path.join(ROOT, "config.ini")).read()
    assert src.index("checkpoint_dir") > src.index("[general]")
    keys = [l for l in src.splitlines() if " : " in l and not l.startswith("#")]
    comments = "\n".join(l for l in src.splitlines() if l.startswith("#"))
    for line in keys:
        assert src.count(line + "\n") == 1 and line not in comments, line
    assert "feature_norm : none\n" in src and "feature_norm_variance : True\n" in src and "feature_norm_stats : " in src
    section = src.split("[acoustic_network_params]")[1].split("[general]")[0]
    assert "feature_norm : none" in section


def test_config_keys_default_validate_and_compare_structurally(tmp_path):
    from util.hyperparams import read_config_file, HyperParameterHandler
    cfg, src = _config(tmp_path)
    d = read_config_file(cfg)
    assert (d["feature_norm"], d["feature_norm_variance"], d["feature_norm_stats"]) == ("none", True, "data/feature_stats.npz")
    bare = tmp_path / "bare.ini"                 # a config.ini written before the keys existed
    bare.write_text("\n".join(l for l in src.splitlines() if not l.startswith("feature_norm")))
    d = read_config_file(str(bare))
    assert (d["feature_norm"], d["feature_norm_variance"], d["feature_norm_stats"]) == ("none", True, None)
    for mode in ("utterance", "global"):
        cfg, _ = _config(tmp_path, feature_norm=("none", mode), feature_norm_variance=("True", "False"))
        d = read_config_file(cfg)
        assert (d["feature_norm"], d["feature_norm_variance"]) == (mode, False)
    for keys in (dict(feature_norm=("none", "sliding")), dict(feature_norm=("none", "Utterance")), dict(feature_norm_variance=("True", "perhaps"))):
        cfg, _ = _config(tmp_path, **keys)
        with pytest.raises(ValueError):
            read_config_file(cfg)
    no_path = tmp_path / "no_path.ini"           # global without a statistics file
    no_path.write_text("\n".join(l.replace("feature_norm : none", "feature_norm : global") for l in src.splitlines()
                                 if not l.startswith("feature_norm_stats")))
    with pytest.raises(ValueError, match="feature_norm_stats"):
        read_config_file(str(no_path))

    cfg, _ = _config(tmp_path)
    h = HyperParameterHandler(cfg)
    old = h.get_hyper_params()
    assert not h.check_changed(old)
    legacy = {k: v for k, v in old.items() if not k.startswith("feature_norm")}
    assert not h.check_changed(legacy)
    h.save_params(legacy)                        # a pickle written before the keys existed compares as none / True
    assert not h.check_changed(old)
    assert h.check_changed(dict(old, feature_norm="utterance")) and h.check_changed(dict(old, feature_norm_variance=False))
    assert not h.check_changed(dict(old, feature_norm_stats="elsewhere.npz"))          # the path is not structural
    h.save_params(dict(old, feature_norm="global"))
    assert h.check_changed(old) and h.check_changed(legacy)
    assert h.check_changed(dict(old, frame_stack=3))


def test_processor_dataset_and_model_carry_the_keys(tmp_path):
    import stt
    from models.AcousticModel import AcousticModel
    from rnn_speech_amd.feature_norm import FeatureStats, describe
    from util.audioprocessor import AudioProcessor
    base = AudioProcessor(1001, "mfcc", n_mfcc=40, device="cpu")
    assert (base.feature_norm, base.feature_norm_variance, base.feature_stats) == ("none", True, None)
    utt = AudioProcessor(1001, "fbank", device="cpu", feature_norm="utterance", feature_norm_variance=False, frame_stack=3, frame_skip=3)
    assert (utt.feature_norm, utt.feature_norm_variance, utt.source_feature_size, utt.feature_size) == ("utterance", False, 120, 360)
    with pytest.raises(ValueError):
        AudioProcessor(1001, "mfcc", device="cpu", feature_norm="sliding")
    with pytest.raises(ValueError, match="feature_stats"):
        AudioProcessor(1001, "mfcc", device="cpu", feature_norm="global")

    stats = FeatureStats(describe("mfcc", 20, 22050, 20))
    stats.merge_moments(np.stack([np.arange(20.0), np.full(20, 8.0)])[None], [2], 2)
    path = str(tmp_path / "stats.npz")
    stats.save(path)
    glob = AudioProcessor(90, "mfcc", n_mfcc=20, device="cpu", feature_norm="global", feature_stats=path)
    assert glob.feature_stats.count == 2 and np.array_equal(glob.feature_stats.mean, np.arange(20.0))
    assert AudioProcessor(90, "mfcc", n_mfcc=20, device="cpu", feature_norm="global", feature_stats=stats).feature_stats is stats
    for other in (dict(n_mfcc=40), dict(n_mfcc=20, load_sr=16000), dict(feature_type="fbank")):       # a file of other features is refused
        kw = dict(dict(feature_type="mfcc", n_mfcc=20), **other)
        with pytest.raises(ValueError, match="the processor computes"):
            AudioProcessor(90, kw.pop("feature_type"), device="cpu", feature_norm="global", feature_stats=path, **kw)
        kw = dict(dict(feature_type="mfcc", n_mfcc=20), **other)
        with pytest.raises(ValueError, match="the processor computes"):
            AudioProcessor(90, kw.pop("feature_type"), device="cpu", feature_norm="global", feature_stats=stats, **kw)
    # with the mode off the file is not even opened
    assert AudioProcessor(90, "mfcc", n_mfcc=40, device="cpu", feature_stats=str(tmp_path / "missing.npz")).feature_stats is None

    ds = AcousticModel.build_dataset([], 2, 90, 12, "mfcc", {}, feature_norm="global", feature_norm_variance=False, feature_stats=path)
    assert (ds.audio.feature_norm, ds.audio.feature_norm_variance, ds.audio.feature_stats.count) == ("global", False, 2)
    again = ds.with_items([])
    assert (again.audio.feature_norm, again.audio.feature_norm_variance) == ("global", False) and again.audio.feature_stats is ds.audio.feature_stats
    plain = AcousticModel.build_dataset([], 2, 90, 12, "mfcc", {})
    assert (plain.audio.feature_norm, plain.audio.feature_stats) == ("none", None)
    model = AcousticModel(2, 64, 2, 30, 12, 60, False, 30)
    assert (model.feature_norm, model.feature_norm_variance, model.feature_stats) == ("none", True, None)
    stt._set_model_options(model, dict(feature_norm="global", feature_norm_variance=False, feature_norm_stats=path))
    assert (model.feature_norm, model.feature_norm_variance, model.feature_stats) == ("global", False, path)
    stt._set_model_options(model, dict(feature_norm="utterance", feature_norm_stats=path))          # the file belongs to global mode only
    assert (model.feature_norm, model.feature_norm_variance, model.feature_stats) == ("utterance", True, None)
    hp = dict(max_input_seq_length=90, signal_processing="mfcc", n_mfcc=20, max_target_seq_length=12, feature_norm="global",
              feature_norm_stats=path)
    audio = stt.build_audio_processor(hp)
    assert audio.feature_norm == "global" and audio.feature_stats.count == 2 and hp["input_dim"] == 20


def test_command_line_carries_the_new_mode(monkeypatch):
    import stt
    names = [name for name, _, _ in stt._MODES]
    assert names[:7] == ["train_acoustic", "train_language", "file", "record", "evaluate", "generate_text", "align"]
    assert names[7:] == ["feature_stats"] and stt._MODES[7][1] == "store_true"
    monkeypatch.setattr(sys, "argv", ["stt.py", "--feature_stats", "--config", "other.ini"])
    args = stt.parse_args()
    assert args["feature_stats"] is True and args["train_acoustic"] is False and args["config_file"] == "other.ini"
    monkeypatch.setattr(sys, "argv", ["stt.py", "--feature_stats", "--evaluate"])
    with pytest.raises(SystemExit):
        stt.parse_args()
