"""Low frame rate input (frame_stack / frame_skip), everything that needs no GPU: the numpy reference against a brute force, the host
arithmetic and the plan query of the C ABI, what the calls refuse, the config keys and the AudioProcessor's length rules."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frame_stack_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_reference_equals_the_brute_force(name):
    k, s, D, t_in, B, _, _ = ref.CASES[name]
    x, lengths = ref.case_inputs(name)
    out, n_out = ref.stack(x, lengths, k, s)
    assert out.dtype == np.uint32 and out.shape == (ref.ceil_div(t_in, s), B, k * D)
    assert np.array_equal(out, ref.stack_brute_force(x, lengths, k, s))
    assert list(n_out) == [-(-int(n) // s) for n in lengths]
    # the inputs are what the docstring says: poison from each row's length on and nowhere else, so no poison in the result
    for b in range(B):
        n = min(int(lengths[b]), t_in)
        assert np.all(x[n:, b] == ref.POISON) and not np.any(x[:n, b] == ref.POISON)
    assert not np.any(out == ref.POISON)


def test_the_table_covers_every_axis_value_and_both_variants():
    cases = ref.CASES.values()
    pairs = {(1, 1), (3, 3), (2, 3), (3, 1), (8, 3), (1, 4), (16, 16)}
    assert {(c[0], c[1]) for c in cases} == pairs
    assert {c[2] for c in cases} == {1, 6, 13, 20, 40, 120}
    assert {c[3] for c in cases} >= {1, 2, 7, 9, 10}
    assert {c[4] for c in cases} == {1, 3, 33, 257}
    for pair in pairs:
        assert {ref.expected_plan(c[4], c[2], c[3], c[0], c[1])["vec"] for c in cases if (c[0], c[1]) == pair} == {1, 4}, pair
    assert sum(ref.expected_plan(c[4], c[2], c[3], c[0], c[1])["meta_by_copy"] for c in cases) == 1
    kinds = set()                                # which of 0, 1, t_in - 1, t_in, t_in + 5 the batches hold
    for name, c in ref.CASES.items():
        kinds |= {(c[5] + b) % 5 for b in range(c[4])}
        if c[4] >= 5:
            assert len(set(ref.case_lengths(c[3], c[4], c[5]))) >= 4, name      # mixed within one batch
        plan = ref.expected_plan(c[4], c[2], c[3], c[0], c[1])
        assert all(plan[f] == v for f, v in c[6].items()), (name, plan)
    assert kinds == {0, 1, 2, 3, 4}
    assert list(ref.case_lengths(10, 5, 0)) == [0, 1, 9, 10, 15]
    # t_in below k, and a last window that runs past the end
    assert any(c[3] < c[0] for c in cases) and any((c[3] - 1) // c[1] * c[1] + c[0] > c[3] for c in cases)


@pytest.mark.parametrize("s", [1, 3, 16])
def test_num_frames_is_the_ceiling(handle, s):
    for n in (0, 1, s - 1, s, s + 1, 3510):
        assert handle.amdspeech_frame_stack_num_frames(n, s) == -(-n // s), (n, s)
    assert handle.amdspeech_frame_stack_num_frames(-1, s) < 0
    assert handle.amdspeech_frame_stack_num_frames(10, 0) < 0 and handle.amdspeech_frame_stack_num_frames(10, 17) < 0


def test_plan_struct_is_the_headers(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_frame_stack_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.FrameStackPlanInfo._fields_]
    assert [n for n, _ in lib.FrameStackPlanInfo._fields_] == ["t_out", "d_out", "vec", "workgroups", "meta_by_copy"]
    assert ctypes.sizeof(lib.FrameStackPlanInfo) == 4 * len(lib.FrameStackPlanInfo._fields_)


def test_plan_reports_the_geometry_without_a_device(handle):
    from rnn_speech_amd import ops
    for name, (k, s, D, t_in, B, _, fields) in ref.CASES.items():
        plan = ops.frame_stack_plan(B, D, t_in, k, s)
        assert plan == ref.expected_plan(B, D, t_in, k, s), name
        assert (plan["t_out"], plan["d_out"], plan["vec"]) == (-(-t_in // s), k * D, 4 if D % 4 == 0 else 1), name
        assert all(plan[f] == v for f, v in fields.items()), name
    for B in (1, 255, 256, 257, 1000):
        assert ops.frame_stack_plan(B, 40, 1001, 3, 3)["meta_by_copy"] == (1 if B > 256 else 0), B
    head = ops.frame_stack_plan(32, 40, 1001, 3, 3)        # the headline shape: 334 model frames of 120, 8 items per workgroup
    assert head == dict(t_out=334, d_out=120, vec=4, workgroups=1336, meta_by_copy=0)
    assert ops.frame_stack_plan(32, 40, 3510, 3, 3)["t_out"] == 1170
    assert ops.frame_stack_plan(32, 256, 3510, 16, 1)["workgroups"] == 2048        # the grid is capped


PLAN_REFUSALS = [
    # B, D, t_in, stack, skip, a word of the message
    (0, 40, 10, 3, 3, b"bad shape"), (-1, 40, 10, 3, 3, b"bad shape"), (4, 0, 10, 3, 3, b"bad shape"), (4, 40, 0, 3, 3, b"bad shape"),
    (4, 40, 10, 0, 3, b"stack"), (4, 40, 10, 17, 3, b"stack"), (4, 40, 10, 3, 0, b"skip"), (4, 40, 10, 3, 17, b"skip"),
    (4, 1028, 10, 4, 1, b"4096"), (4, 4097, 10, 1, 1, b"4096"),
]


@pytest.mark.parametrize("B,D,t_in,k,s,word", PLAN_REFUSALS)
def test_plan_and_call_refuse_a_bad_shape(handle, B, D, t_in, k, s, word):
    from rnn_speech_amd import lib, ops
    info = lib.FrameStackPlanInfo()
    assert ref.expected_plan(B, D, t_in, k, s) is None
    assert handle.amdspeech_frame_stack_plan(B, D, t_in, k, s, ctypes.byref(info)) != 0
    assert word in handle.amdspeech_last_error()
    with pytest.raises(lib.AmdSpeechError):
        ops.frame_stack_plan(B, D, t_in, k, s)
    # the call checks the shape as the plan does, before it touches a pointer or the device
    n = (ctypes.c_int * max(B, 1))()
    x, out = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    assert handle.amdspeech_frame_stack(None, x, n, B, D, t_in, k, s, out, n) != 0
    assert word in handle.amdspeech_last_error()


def test_plan_and_call_refuse_bad_pointers(handle):
    from rnn_speech_amd import lib
    B, D, t_in, k, s = 4, 40, 10, 3, 3
    n_in, n_out = (ctypes.c_int * B)(10, 3, 0, 15), (ctypes.c_int * B)()
    x, out = 1 << 20, 1 << 30
    call = handle.amdspeech_frame_stack

    def refused(word, *args):
        assert call(None, *args) != 0
        assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()

    assert handle.amdspeech_frame_stack_plan(B, D, t_in, k, s, None) != 0 and b"null" in handle.amdspeech_last_error()
    refused(b"null", None, n_in, B, D, t_in, k, s, ctypes.c_void_p(out), n_out)
    refused(b"null", ctypes.c_void_p(x), None, B, D, t_in, k, s, ctypes.c_void_p(out), n_out)
    refused(b"null", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, None, n_out)
    refused(b"null", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, ctypes.c_void_p(out), None)
    src_bytes, out_bytes = t_in * B * D * 4, 4 * B * k * D * 4
    refused(b"overlap", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, ctypes.c_void_p(x), n_out)                       # in place
    refused(b"overlap", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, ctypes.c_void_p(x + src_bytes - 16), n_out)      # out starts in x's last words
    refused(b"overlap", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, ctypes.c_void_p(x - out_bytes + 16), n_out)      # out ends in x's first words
    refused(b"aligned", ctypes.c_void_p(x + 4), n_in, B, D, t_in, k, s, ctypes.c_void_p(out), n_out)
    refused(b"aligned", ctypes.c_void_p(x), n_in, B, D, t_in, k, s, ctypes.c_void_p(out + 8), n_out)
    bad = (ctypes.c_int * B)(10, -1, 0, 15)
    refused(b"negative", ctypes.c_void_p(x), bad, B, D, t_in, k, s, ctypes.c_void_p(out), n_out)
    assert list(n_out) == [0] * B                          # a refused call writes no length
    assert lib.PROTOTYPES["amdspeech_frame_stack"][1][2] == ctypes.c_void_p      # (host arrays pass as pointers)


def _config(tmp_path, extra=""):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    assert "frame_stack : 1\n" in src and "frame_skip : 1\n" in src
    for key, value in (l.split(":") for l in extra.splitlines()):
        src = src.replace("%s : 1\n" % key.strip(), "%s : %s\n" % (key.strip(), value.strip()), 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    return str(cfg), src


def test_config_keys_default_parse_range_and_structural_change(tmp_path):
    from util.hyperparams import read_config_file, HyperParameterHandler
    cfg, src = _config(tmp_path)
    d = read_config_file(cfg)
    assert (d["frame_stack"], d["frame_skip"]) == (1, 1)
    bare = tmp_path / "bare.ini"                 # a config.ini written before the keys existed
    bare.write_text("\n".join(l for l in src.splitlines() if not l.startswith(("frame_stack", "frame_skip"))))
    d = read_config_file(str(bare))
    assert (d["frame_stack"], d["frame_skip"]) == (1, 1)
    cfg, _ = _config(tmp_path, "frame_stack : 3\nframe_skip : 3")
    d = read_config_file(cfg)
    assert (d["frame_stack"], d["frame_skip"]) == (3, 3)
    cfg, _ = _config(tmp_path, "frame_stack : 16\nframe_skip : 16")
    assert read_config_file(cfg)["frame_skip"] == 16
    for extra in ("frame_stack : 0", "frame_stack : 17", "frame_skip : 0", "frame_skip : 17"):
        cfg, _ = _config(tmp_path, extra)
        with pytest.raises(ValueError):
            read_config_file(cfg)
    cfg, _ = _config(tmp_path)
    h = HyperParameterHandler(cfg)
    old = h.get_hyper_params()
    assert not h.check_changed(old)
    legacy = dict(old)
    legacy.pop("frame_stack")
    legacy.pop("frame_skip")
    assert not h.check_changed(legacy)
    h.save_params(legacy)                        # a pickle written before the keys existed compares as (1, 1)
    assert not h.check_changed(old)
    assert h.check_changed(dict(old, frame_stack=3))
    assert h.check_changed(dict(old, frame_skip=3))
    h.save_params(old)
    assert h.check_changed(dict(old, frame_stack=3)) and h.check_changed(dict(old, frame_skip=3))


def test_audio_processor_length_rules():
    from util.audioprocessor import AudioProcessor
    base = AudioProcessor(1001, "mfcc", n_mfcc=40, device="cpu")
    lfr = AudioProcessor(1001, "mfcc", n_mfcc=40, device="cpu", frame_stack=3, frame_skip=3)
    assert (lfr.feature_size, lfr.out_seq_length, lfr.frame_hop_samples) == (120, 334, 3 * lfr.hop_samples)
    assert lfr.max_input_seq_length == 1001 and lfr.hop_samples == base.hop_samples
    # at (1, 1) the three attributes are today's values
    assert (base.feature_size, base.out_seq_length, base.frame_hop_samples) == (40, 1001, base.hop_samples)
    assert (base.frame_stack, base.frame_skip) == (1, 1)
    fb = AudioProcessor(3510, "fbank", device="cpu", load_sr=16000, frame_stack=8, frame_skip=3)
    assert (fb.feature_size, fb.out_seq_length, fb.frame_hop_samples) == (960, 1170, 480)
    for bad in (dict(frame_stack=0), dict(frame_stack=17), dict(frame_skip=0), dict(frame_skip=17)):
        with pytest.raises(ValueError):
            AudioProcessor(1001, "mfcc", device="cpu", **bad)
    # the source frames the front end runs for t_max model frames: every frame their windows reach, at most max_input_seq_length
    assert lfr._source_t_max(None) == 1001 and lfr._source_t_max(334) == 1001 and lfr._source_t_max(10) == 30
    assert AudioProcessor(90, "mfcc", device="cpu", frame_stack=8, frame_skip=3)._source_t_max(10) == 35
    assert base._source_t_max(None) == 1001 and base._source_t_max(60) == 60 and base._source_t_max(2000) == 2000


def test_dataset_and_model_carry_the_keys():
    from models.AcousticModel import AcousticModel
    ds = AcousticModel.build_dataset([], 2, 90, 12, "mfcc", {}, frame_stack=3, frame_skip=3)
    assert (ds.T, ds.audio.feature_size, ds.audio.max_input_seq_length) == (30, 60, 90)
    again = ds.with_items([])
    assert (again.T, again.audio.frame_stack, again.audio.frame_skip, again.audio.max_input_seq_length) == (30, 3, 3, 90)
    plain = AcousticModel.build_dataset([], 2, 90, 12, "mfcc", {})
    assert (plain.T, plain.audio.feature_size) == (90, 20)
    model = AcousticModel(2, 64, 2, 30, 12, 60, False, 30)
    assert (model.frame_stack, model.frame_skip) == (1, 1)
