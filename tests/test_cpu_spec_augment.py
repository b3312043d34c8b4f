"""SpecAugment (csrc/spec_augment.hip), everything that needs no GPU: the numpy reference's own properties, the spans and the plan
query of the C ABI against it, what the calls refuse, and the config keys."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_augment_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


def _desc(pol, seed=ref.SEED):
    from rnn_speech_amd import lib
    return lib.SpecAugmentDesc(pol["period"], pol["freq_masks"], pol["freq_width"], pol["time_masks"], pol["time_width"],
                               pol["time_permille"], seed)


# ------------------------------------------------------------------------------------------------ the reference alone
def test_the_draw_is_the_documented_hash():
    """Two values worked by hand from the formula (32-bit wrap-around), so that a slip in `ref.r` cannot hide behind the library
    making the same slip."""
    def mix(v):
        v = np.uint32(v)
        with np.errstate(over="ignore"):
            v ^= v >> np.uint32(16)
            v *= np.uint32(0x7feb352d)
            v ^= v >> np.uint32(15)
            v *= np.uint32(0x846ca68b)
            v ^= v >> np.uint32(16)
        return v

    for seed, stream, idx in ((ref.SEED, 0x5A000000, 0), (ref.SEED, 0x5A000003, 2 * 64 + 1), (0xFFFFFFFFFFFFFFFF, 0x5A000002, 12345)):
        with np.errstate(over="ignore"):
            a = mix(np.uint32(idx) ^ np.uint32(seed & 0xFFFFFFFF))
            b = mix(a + np.uint32(stream) * np.uint32(0x9e3779b9) + np.uint32(seed >> 32))
        assert ref.r(seed, stream, idx) == int(b) >> 8 < 1 << 24


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_no_case_masks_nothing_or_everything(name):
    """The conditions the table was written under, from the reference alone: every case but cap_zero and full_width has a
    non-empty frequency span and a non-empty time span, cap_zero has frequency spans and NO time span, and at least 10 live words
    stay unmasked everywhere."""
    T, B, W, P, F, Fw, M, Tw, pm, lengths = ref.CASES[name]
    pol = ref.case_policy(name)
    freq = time = 0
    for b in range(B):
        n = min(lengths[b], T)
        if n <= 0:
            continue
        sp = ref.spans(pol, ref.SEED, b, n)
        assert len(sp) == F + M
        freq += sum(w > 0 for _, w in sp[:F])
        time += sum(w > 0 for _, w in sp[F:])
    if name == "cap_zero":
        assert freq > 0 and time == 0
    elif name == "full_width":
        assert freq > 0 and M == 0
    else:
        assert freq > 0 and time > 0
    x, lens = ref.case_inputs(name)
    out = ref.apply(x, lens, pol, ref.SEED)
    live = np.arange(T)[:, None] < np.minimum(lens, T)[None, :]
    assert not np.any(x[live] == 0) and not np.any(x[live] == ref.POISON) and np.all(x[~live] == ref.POISON)
    changed = out != x
    assert np.all(out[changed] == 0) and not np.any(changed[~live])
    assert changed.any() and int((~changed[live]).sum()) >= 10
    if name == "cap_zero":                       # only whole bins change: a changed word's bin is changed in every live frame of its row
        for b in range(B):
            col = changed[:min(lens[b], T), b]
            assert np.array_equal(col.any(axis=0), col.all(axis=0))
    # a brute-force restatement, element by element
    if T * B * W <= 20000:
        brute = x.copy()
        for b in range(B):
            n = min(int(lens[b]), T)
            sp = ref.spans(pol, ref.SEED, b, n) if n > 0 else []
            for t in range(n):
                for c in range(W):
                    if any(s <= c % P < s + w for s, w in sp[:F]) or any(s <= t < s + w for s, w in sp[F:]):
                        brute[t, b, c] = 0
        assert np.array_equal(out, brute)


def test_the_stride_case_strides():
    T, B, W = ref.CASES["stride"][:3]
    plan = ref.expected_plan(T, B, W, ref.case_policy("stride"))
    assert plan["workgroups"] == ref.MAX_WGS and T * B > ref.MAX_WGS * plan["items_per_workgroup"]
    assert min(ref.CASES["stride"][9]) == 270 and max(ref.CASES["stride"][9]) == 309


def test_widths_and_starts_stay_in_range_and_spread():
    for name, case in ref.CASES.items():
        T, B, W, P, F, Fw, M, Tw, pm, lengths = case
        pol = ref.case_policy(name)
        for seed in [ref.SEED] + [s * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF for s in range(1, 6)]:
            for b in range(min(B, 8)):
                for n in {0, 1, min(lengths[b], T), T}:
                    sp = ref.spans(pol, seed, b, n)
                    for start, width in sp[:F]:
                        assert 0 <= width <= min(Fw, P) and 0 <= start <= P - width
                    for start, width in sp[F:]:
                        assert 0 <= width <= min(Tw, n * pm // 1000) and 0 <= start <= n - width
    # uniform: 20,000 draws over 28 widths (expected 714 per bin, standard deviation 26: five of them either way)
    pol = ref.policy(80, 1, 27, 0, 0, 0)
    hits = np.bincount([ref.spans(pol, seed, 3, 10)[0][1] for seed in range(20000)], minlength=28)
    assert len(hits) == 28 and hits.min() > 714 - 130 and hits.max() < 714 + 130


# ------------------------------------------------------------------------------------------------ the C ABI against it
def test_library_spans_equal_the_reference(handle):
    from rnn_speech_amd import ops
    for name, case in ref.CASES.items():
        T, B, W, P, F, Fw, M, Tw, pm, lengths = case
        pol = ref.case_policy(name)
        rows = range(B) if B <= 8 else list(range(0, B, 37)) + [B - 1]
        for b in rows:
            for n in sorted({0, min(lengths[b], T)}):
                want = ref.spans(pol, ref.SEED, b, n)
                assert ops.spec_augment_spans(pol, ref.SEED, b, n) == want, (name, b, n)
                out = (ctypes.c_int * (2 * (F + M) + 1))(*([-7] * (2 * (F + M) + 1)))
                assert handle.amdspeech_spec_augment_spans(ctypes.byref(_desc(pol)), b, n, out) == 0
                assert list(out)[:-1] == [v for pair in want for v in pair] and out[2 * (F + M)] == -7      # (no word past the end)
    # other seeds, a high row index, the largest policy
    pol = ref.policy(80, 8, 27, 16, 100, 1000)
    for seed in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0):
        for b, n in ((0, 1), (255, 1001), (100000, 3510)):
            assert ops.spec_augment_spans(pol, seed, b, n) == ref.spans(pol, seed, b, n)


def test_plan_struct_and_desc_are_the_headers(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_spec_augment_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.SpecAugmentPlanInfo._fields_]
    assert ctypes.sizeof(lib.SpecAugmentPlanInfo) == 4 * len(lib.SpecAugmentPlanInfo._fields_)
    decl = header.split("typedef struct amdspeech_spec_augment_desc {")[1].split("}")[0]
    ints, seed = decl.split(";")[:2]
    assert [n.strip() for n in ints.replace("int", "").split(",")] == [n for n, _ in lib.SpecAugmentDesc._fields_[:-1]]
    assert seed.split() == ["unsigned", "long", "long", "seed"] and lib.SpecAugmentDesc._fields_[-1] == ("seed", ctypes.c_uint64)
    assert ctypes.sizeof(lib.SpecAugmentDesc) == 32 and lib.SpecAugmentDesc.seed.offset == 24
    for name in ("amdspeech_spec_augment", "amdspeech_spec_augment_spans", "amdspeech_spec_augment_plan"):
        assert name in lib.PROTOTYPES and getattr(handle, name) is not None


def test_plan_reports_the_geometry_without_a_device(handle):
    from rnn_speech_amd import ops
    for name, case in ref.CASES.items():
        T, B, W = case[:3]
        pol = ref.case_policy(name)
        plan = ops.spec_augment_plan(T, B, W, pol)
        assert plan == ref.expected_plan(T, B, W, pol), name
        assert plan["vec"] == (4 if W % 4 == 0 else 1) and plan["reps"] == W // pol["period"] and plan["workgroups"] > 0, name
    assert {ref.expected_plan(c[0], c[1], c[2], ref.case_policy(n))["vec"] for n, c in ref.CASES.items()} == {1, 4}
    head = ops.spec_augment_plan(1001, 32, 40, ref.policy(40, 2, 7, 2, 40, 200))      # the headline shape: 16 items per workgroup
    assert head == dict(vec=4, lanes=4, items_per_workgroup=64, workgroups=501, reps=1)
    assert ops.spec_augment_plan(3510, 64, 120, ref.policy(40, 2, 7, 2, 40, 200))["workgroups"] == 2048      # the grid is capped
    assert ops.spec_augment_plan(10, 2, 4096, ref.policy(4096, 1, 1, 0, 0, 0))["lanes"] == 256
    # off: nothing would be launched.  No mask of either kind, or no width of either kind (or a kind with only one of the two)
    for off in (ref.policy(40, 0, 0, 0, 0, 1000), ref.policy(40, 0, 7, 0, 40, 1000), ref.policy(40, 2, 0, 2, 0, 1000),
                ref.policy(40, 0, 7, 2, 0, 1000), ref.policy(40, 2, 0, 0, 40, 1000), ref.policy(40, 0, 7, 2, 40, 0)):
        plan = ops.spec_augment_plan(1001, 32, 40, off)
        assert plan == ref.expected_plan(1001, 32, 40, off) and plan["workgroups"] == 0, off
    for on in (ref.policy(40, 1, 1, 0, 0, 0), ref.policy(40, 0, 0, 1, 1, 1)):
        assert ops.spec_augment_plan(1001, 32, 40, on)["workgroups"] == 501, on


REFUSALS = [
    # T, B, W, (P, F, Fw, M, Tw, permille), a word of the message
    (10, 2, 40, (13, 2, 5, 2, 4, 1000), b"does not divide"),         # W % P != 0
    (10, 2, 40, (80, 2, 5, 2, 4, 1000), b"does not divide"),         # P > W
    (10, 2, 40, (0, 2, 0, 2, 4, 1000), b"period"),
    (10, 2, 40, (40, 9, 5, 2, 4, 1000), b"freq_masks"),
    (10, 2, 40, (40, -1, 5, 2, 4, 1000), b"freq_masks"),
    (10, 2, 40, (40, 2, 5, 17, 4, 1000), b"time_masks"),
    (10, 2, 40, (40, 2, 5, -1, 4, 1000), b"time_masks"),
    (10, 2, 40, (40, 2, 41, 2, 4, 1000), b"freq_width"),             # Fw > P
    (10, 2, 80, (40, 2, 41, 2, 4, 1000), b"freq_width"),             # ... P, not W, bounds it
    (10, 2, 40, (40, 2, -1, 2, 4, 1000), b"freq_width"),
    (10, 2, 40, (40, 2, 5, 2, -1, 1000), b"time_width"),
    (10, 2, 40, (40, 2, 5, 2, 4, 1001), b"time_permille"),
    (10, 2, 40, (40, 2, 5, 2, 4, -1), b"time_permille"),
    (10, 2, 4100, (4100, 2, 5, 2, 4, 1000), b"4096"),                # W > 4096
    (10, 2, 0, (1, 2, 1, 2, 4, 1000), b"W 0"),
    (0, 2, 40, (40, 2, 5, 2, 4, 1000), b"bad shape"),
    (10, 0, 40, (40, 2, 5, 2, 4, 1000), b"bad shape"),
    (1 << 16, 1 << 15, 40, (40, 2, 5, 2, 4, 1000), b"bad shape"),    # T * B = 2^31
]


@pytest.mark.parametrize("T,B,W,pol,word", REFUSALS)
def test_plan_and_call_refuse_with_a_message(handle, T, B, W, pol, word):
    from rnn_speech_amd import lib, ops
    pol = ref.policy(*pol)
    assert ref.expected_plan(T, B, W, pol) is None
    info = lib.SpecAugmentPlanInfo()
    assert handle.amdspeech_spec_augment_plan(T, B, W, ctypes.byref(_desc(pol)), ctypes.byref(info)) != 0
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()
    with pytest.raises(lib.AmdSpeechError):
        ops.spec_augment_plan(T, B, W, pol)
    # the call checks the shape and the policy as the plan does, before it touches a pointer or the device
    x, lengths = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    assert handle.amdspeech_spec_augment(None, x, lengths, T, B, W, ctypes.byref(_desc(pol))) != 0
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()


def test_null_pointers_and_bad_span_queries_are_refused(handle):
    from rnn_speech_amd import lib
    pol = ref.policy(40, 2, 7, 2, 5, 1000)
    d, info = _desc(pol), lib.SpecAugmentPlanInfo()
    x, lengths = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    out = (ctypes.c_int * 8)()

    def refused(rc, word):
        assert rc != 0 and word in handle.amdspeech_last_error(), handle.amdspeech_last_error()

    refused(handle.amdspeech_spec_augment_plan(10, 2, 40, ctypes.byref(d), None), b"null")
    refused(handle.amdspeech_spec_augment_plan(10, 2, 40, None, ctypes.byref(info)), b"null")
    refused(handle.amdspeech_spec_augment(None, None, lengths, 10, 2, 40, ctypes.byref(d)), b"null")
    refused(handle.amdspeech_spec_augment(None, x, None, 10, 2, 40, ctypes.byref(d)), b"null")
    refused(handle.amdspeech_spec_augment(None, x, lengths, 10, 2, 40, None), b"null")
    refused(handle.amdspeech_spec_augment_spans(None, 0, 10, out), b"null")
    refused(handle.amdspeech_spec_augment_spans(ctypes.byref(d), 0, 10, None), b"null")
    refused(handle.amdspeech_spec_augment_spans(ctypes.byref(d), -1, 10, out), b"negative")
    refused(handle.amdspeech_spec_augment_spans(ctypes.byref(d), 0, -1, out), b"negative")
    refused(handle.amdspeech_spec_augment_spans(ctypes.byref(_desc(ref.policy(40, 9, 7, 2, 5, 1000))), 0, 10, out), b"freq_masks")
    refused(handle.amdspeech_spec_augment_spans(ctypes.byref(_desc(ref.policy(40, 2, 7, 17, 5, 1000))), 0, 10, out), b"time_masks")
    assert list(out) == [0] * 8                          # a refused query writes nothing


def test_ops_refuses_what_is_not_a_device_batch(handle):
    """ops.spec_augment's own checks come before any device call, so they can be seen without a GPU."""
    import torch
    from rnn_speech_amd import ops
    pol = ref.policy(40, 2, 7, 2, 5, 1000)
    with pytest.raises(ValueError):
        ops.spec_augment(torch.zeros(4, 2, 40), torch.zeros(2, dtype=torch.int32), pol, 1)       # host tensors
    with pytest.raises(ValueError):
        ops.spec_augment(np.zeros((4, 2, 40), np.float32), [4, 4], pol, 1)
    with pytest.raises(ValueError):
        ops.spec_augment_plan(4, 2, 40, dict(period=40), 1)                                      # a policy with keys missing


# ------------------------------------------------------------------------------------------------ the config keys
KEYS = ("spec_augment_freq_masks", "spec_augment_freq_width", "spec_augment_time_masks", "spec_augment_time_width",
        "spec_augment_time_permille", "spec_augment_seed")


def _config(tmp_path, **values):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for key, value in values.items():
        old = "spec_augment_%s : %s\n" % (key, "1.0" if key == "time_ratio" else "0")
        assert old in src
        src = src.replace(old, "spec_augment_%s : %s\n" % (key, value), 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    return str(cfg), src


def test_config_keys_default_parse_range_and_no_structural_change(tmp_path):
    import stt
    from util.audioprocessor import AudioProcessor
    from util.hyperparams import read_config_file, HyperParameterHandler
    cfg, src = _config(tmp_path)
    off = read_config_file(cfg)
    assert [off[k] for k in KEYS] == [0, 0, 0, 0, 1000, 0]
    bare = tmp_path / "bare.ini"                 # a config.ini written before the keys existed
    bare.write_text("\n".join(l for l in src.splitlines() if not l.startswith("spec_augment_")))
    assert not any(l.startswith("spec_augment_") for l in bare.read_text().splitlines())
    d = read_config_file(str(bare))
    assert [d[k] for k in KEYS] == [0, 0, 0, 0, 1000, 0]
    mfcc = AudioProcessor(1001, "mfcc", n_mfcc=40, device="cpu", frame_stack=3, frame_skip=3)
    assert stt.spec_augment_policy(d, mfcc) is None and stt.spec_augment_policy({}, mfcc) is None       # off: no policy at all

    cfg, _ = _config(tmp_path, freq_masks=2, freq_width=7, time_masks=2, time_width=40, time_ratio=0.2, seed=11)
    on = read_config_file(cfg)
    assert [on[k] for k in KEYS] == [2, 7, 2, 40, 200, 11]
    want = dict(period=40, freq_masks=2, freq_width=7, time_masks=2, time_width=40, time_permille=200, seed=11)
    assert stt.spec_augment_policy(on, mfcc) == want                                                  # the source frame's width under stacking
    fbank = AudioProcessor(1001, "fbank", device="cpu")
    assert fbank.source_feature_size == 120 and stt.spec_augment_policy(on, fbank) == want            # 40 mel bins, three groups
    assert stt.spec_augment_policy(on, AudioProcessor(1001, "mfcc", n_mfcc=20, device="cpu"))["period"] == 20
    with pytest.raises(ValueError):
        stt.spec_augment_policy(dict(on, spec_augment_freq_width=21), AudioProcessor(1001, "mfcc", n_mfcc=20, device="cpu"))
    cfg, _ = _config(tmp_path, time_ratio=0.0335)
    assert read_config_file(cfg)["spec_augment_time_permille"] == 34                                  # round(1000 * ratio)
    cfg, _ = _config(tmp_path, freq_masks=8, time_masks=16, time_ratio=0)
    d = read_config_file(cfg)
    assert (d["spec_augment_freq_masks"], d["spec_augment_time_masks"], d["spec_augment_time_permille"]) == (8, 16, 0)
    for bad in (dict(freq_masks=9), dict(freq_masks=-1), dict(time_masks=17), dict(time_masks=-1), dict(freq_width=-1),
                dict(freq_width=4097), dict(time_width=-1), dict(time_ratio=1.001), dict(time_ratio=-0.1), dict(time_ratio="nan"),
                dict(seed=-1), dict(seed=2 ** 32)):
        cfg, _ = _config(tmp_path, **bad)
        with pytest.raises(ValueError):
            read_config_file(cfg)

    # not structural: a checkpoint stays usable when only these keys change, either way round
    cfg, _ = _config(tmp_path)
    h = HyperParameterHandler(cfg)
    assert not h.check_changed(off) and not h.check_changed(on)
    legacy = {k: v for k, v in off.items() if not k.startswith("spec_augment_")}
    assert not h.check_changed(legacy)
    h.save_params(on)
    assert not h.check_changed(off) and not h.check_changed(legacy)
    h.save_params(legacy)                        # a pickle written before the keys existed
    assert not h.check_changed(on)
    assert h.check_changed(dict(on, frame_stack=3))      # (the handler still sees a structural key)


def test_model_carries_the_policy_and_derives_the_seed():
    from models.AcousticModel import AcousticModel
    model = AcousticModel(2, 64, 2, 30, 12, 60, False, 30)
    assert model.spec_augment is None
    model.spec_augment = dict(ref.policy(20, 2, 5, 2, 4, 1000), seed=7)
    seeds = []
    for counter in (1, 2, 3, 2 ** 31 + 5):
        model._dropout_seed = counter
        seeds.append(model._spec_augment_seed())
        assert seeds[-1] == ((7 + 0) << 32) | ((counter * 0x9E3779B1) & 0xFFFFFFFF)
    assert len(set(seeds)) == 4 and all(s >> 32 == 7 for s in seeds)
