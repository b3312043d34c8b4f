"""Lookahead convolution, everything that needs no GPU: the numpy reference's backward against central differences, the header
section, the exported symbols and the plan query of the C ABI, what the calls refuse, the parameter layout, the checkpoint names and
a native round trip, and the config key."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookahead_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("amdspeech_lookahead_fwd", "amdspeech_lookahead_bwd_workspace_bytes", "amdspeech_lookahead_bwd", "amdspeech_lookahead_plan")
FIELDS = ["vec", "unroll", "col_blocks", "t_chunk", "chunks", "workgroups", "lds_bytes", "dw_partials", "dw_terms", "reduce_slices",
          "reduce_terms", "reduce_workgroups"]


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


# ---- the reference
@pytest.mark.parametrize("T,B,H,context,lengths", [(9, 3, 4, 3, [9, 4, 0]), (4, 2, 3, 6, [4, 1]), (12, 2, 2, 1, [15, 2])])
def test_reference_backward_is_the_gradient_of_its_forward(T, B, H, context, lengths):
    rng = np.random.RandomState(T + context)
    x, dy, w = rng.randn(T, B, H), rng.randn(T, B, H), rng.randn(context + 1, H)
    live = np.arange(T)[:, None] < ref.clip_lengths(lengths, T)[None, :]
    dy_live = np.where(live[:, :, None], dy, 0.0)

    def f(x_, w_):
        return float((ref.forward(x_, w_, lengths) * dy_live).sum())

    dx, dw = ref.backward(x, w, dy, lengths)
    eps = 1e-6
    for a, grad, which in ((x, dx, 0), (w, dw, 1)):
        num = np.zeros_like(a)
        for idx in np.ndindex(*a.shape):
            hi, lo = a.copy(), a.copy()
            hi[idx] += eps
            lo[idx] -= eps
            num[idx] = ((f(hi, w) - f(lo, w)) if which == 0 else (f(x, hi) - f(x, lo))) / (2 * eps)
        if which == 0:
            num = np.where(live[:, :, None], num, 0.0)          # (x past the length is not an input: the reference never reads it)
        assert np.abs(num - grad).max() < 1e-8, which
    assert not dx[~live].any() and not ref.forward(x, w, lengths)[~live].any()
    # frames at or past the length are never read
    poisoned = np.where(live[:, :, None], x, np.nan)
    assert np.array_equal(ref.forward(poisoned, w, lengths), ref.forward(x, w, lengths))
    # the absolute sums bound the sums
    assert (np.abs(ref.forward(x, w, lengths)) <= ref.forward(x, w, lengths, absolute=True) + 1e-15).all()


def test_reference_identity_weights_copy_the_live_frames():
    rng = np.random.RandomState(0)
    x = rng.randn(7, 3, 5)
    w = np.zeros((4, 5))
    w[0] = 1.0
    y = ref.forward(x, w, [7, 3, 0])
    assert np.array_equal(y[:, 0], x[:, 0]) and np.array_equal(y[:3, 1], x[:3, 1]) and not y[3:, 1].any() and not y[:, 2].any()


def test_length_sets_hold_the_edge_lengths():
    rng = np.random.RandomState(1)
    for T, B, H, context in ref.CASES:
        sets = ref.length_sets(T, B, context, rng)
        seen = set(int(v) for s in sets for v in s)
        assert all(len(s) == B for s in sets)
        assert {v for v in (0, 1, context, context + 1, T) if v <= T} <= seen, (T, B, context)


# ---- header, symbols, plan
def test_header_section_prototypes_and_struct(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    assert header.count("lookahead convolution ---") == 1
    section = header.split("lookahead convolution ---")[1].split("voice activity / long recordings ---")[0]
    for name in SYMBOLS:
        proto = re.search(r"\b%s\(([^)]*)\);" % name, section)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(lib.PROTOTYPES[name][1]), name
        assert getattr(handle, name)
    decl = section.split("typedef struct amdspeech_lookahead_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == FIELDS
    assert [n for n, _ in lib.LookaheadPlanInfo._fields_] == FIELDS
    assert ctypes.sizeof(lib.LookaheadPlanInfo) == 4 * len(FIELDS)
    for word in ("ACCUMULATES", "never read", "EVERY element", "fmaf", "No floating-point atomics", "AMDSPEECH_EINVAL", "1 .. 32"):
        assert word in section, word


def expected_plan(T, B, H, context):
    """The chunk arithmetic the header states, restated."""
    ceil = lambda a, b: -(-a // b)
    vec = 4 if H % 4 == 0 else 1
    col_blocks = ceil(B * H // vec, 64)
    tc = max(ceil(T, ceil(1024, col_blocks)), 4 * context)
    tc = ceil(tc, 8) * 8
    chunks = ceil(T, tc)
    return dict(vec=vec, unroll=8, col_blocks=col_blocks, t_chunk=tc, chunks=chunks, workgroups=col_blocks * chunks,
                lds_bytes=(2 * context + 9) * 64 * vec * 4, dw_partials=chunks * B, dw_terms=tc, reduce_slices=8,
                reduce_terms=ceil(chunks * B, 8), reduce_workgroups=ceil((context + 1) * H, 32))


HEADLINE = [(1001, 32, 512, 5), (1001, 32, 512, 20), (1001, 32, 512, 32), (998, 64, 1024, 5), (998, 64, 1024, 20), (998, 64, 1024, 32)]


@pytest.mark.parametrize("T,B,H,context", ref.CASES + HEADLINE + [(385, 2, 64, 32), (3000, 1, 8, 1), (100000, 2, 64, 3)])
def test_plan_reports_the_geometry_without_a_device(handle, T, B, H, context):
    from rnn_speech_amd import ops
    plan = ops.lookahead_plan(T, B, H, context)
    want = expected_plan(T, B, H, context)
    assert {k: plan[k] for k in FIELDS} == want
    assert plan["vec"] == (4 if H % 4 == 0 else 1)
    # the chunks tile the time axis, none is empty, whole blocks, the halo is at most a quarter of a chunk
    assert (plan["chunks"] - 1) * plan["t_chunk"] < T <= plan["chunks"] * plan["t_chunk"]
    assert plan["t_chunk"] % plan["unroll"] == 0 and 4 * context <= plan["t_chunk"]
    # the workspace covers the plan's partial tiles, and those of every shorter run of the same model
    assert plan["workspace_bytes"] >= plan["dw_partials"] * (context + 1) * H * 4
    assert plan["workspace_bytes"] == handle.amdspeech_lookahead_bwd_workspace_bytes(T, B, H, context)
    for t in sorted({1, 2, context, T // 3 + 1, T // 2 + 1, T - 1, T} - {0}):
        if t <= T:
            short = ops.lookahead_plan(t, B, H, context)
            assert short["dw_partials"] * (context + 1) * H * 4 <= plan["workspace_bytes"], t
    assert ref.dw_tree_depth(plan) == plan["t_chunk"] + plan["reduce_terms"] + 8 + 1


def test_plan_at_the_headline_shape_covers_the_chip(handle):
    from rnn_speech_amd import ops
    for context, chunk, chunks in ((5, 64, 16), (20, 80, 13), (32, 128, 8)):
        plan = ops.lookahead_plan(1001, 32, 512, context)
        assert (plan["t_chunk"], plan["chunks"], plan["col_blocks"]) == (chunk, chunks, 64)
        assert plan["workgroups"] >= 2 * 256                       # at least two waves on every one of the 256 CUs
        assert context * plan["chunks"] <= 0.26 * 1001             # what the halos re-read of the 1001 frames
        assert plan["lds_bytes"] <= 160 * 1024


PLAN_REFUSALS = [
    (0, 2, 16, 3, b"bad shape"), (4, 0, 16, 3, b"bad shape"), (4, 2, 0, 3, b"bad shape"), (-1, 2, 16, 3, b"bad shape"),
    (4, 2, 16, 0, b"context 0 outside 1 .. 32"), (4, 2, 16, 33, b"context 33 outside 1 .. 32"), (4, 2, 16, -1, b"outside 1 .. 32"),
    (4, 1 << 16, 1 << 15, 3, b"too large"), (1 << 20, 1 << 12, 16, 3, b"too large"),
]


@pytest.mark.parametrize("T,B,H,context,word", PLAN_REFUSALS)
def test_plan_and_calls_refuse_a_bad_shape(handle, T, B, H, context, word):
    from rnn_speech_amd import lib, ops
    info = lib.LookaheadPlanInfo()
    assert handle.amdspeech_lookahead_plan(T, B, H, context, ctypes.byref(info)) != 0
    assert word in handle.amdspeech_last_error()
    assert handle.amdspeech_lookahead_bwd_workspace_bytes(T, B, H, context) == 0
    with pytest.raises(lib.AmdSpeechError):
        ops.lookahead_plan(T, B, H, context)
    # the calls check the shape as the plan does, before they touch a pointer or the device
    a, b, c, d, e, f, g = (ctypes.c_void_p(k << 32) for k in range(1, 8))
    assert handle.amdspeech_lookahead_fwd(None, a, b, c, T, B, H, context, d) != 0
    assert word in handle.amdspeech_last_error()
    assert handle.amdspeech_lookahead_bwd(None, a, b, c, d, T, B, H, context, e, f, g) != 0
    assert word in handle.amdspeech_last_error()


def test_calls_refuse_null_and_overlapping_pointers(handle):
    T, B, H, context = 6, 2, 16, 2
    size = T * B * H * 4
    x, w, n, y, dx, dw, ws = (ctypes.c_void_p((k << 32)) for k in range(1, 8))
    null = ctypes.c_void_p(0)
    for args in ((null, w, n, y), (x, null, n, y), (x, w, null, y), (x, w, n, null)):
        assert handle.amdspeech_lookahead_fwd(None, args[0], args[1], args[2], T, B, H, context, args[3]) != 0
        assert b"lookahead_fwd: null pointer" in handle.amdspeech_last_error()
    for k in range(7):
        args = [x, w, y, n, dx, dw, ws]
        args[k] = null
        assert handle.amdspeech_lookahead_bwd(None, args[0], args[1], args[2], args[3], T, B, H, context, args[4], args[5], args[6]) != 0
        assert b"lookahead_bwd: null pointer" in handle.amdspeech_last_error()
    assert handle.amdspeech_lookahead_plan(T, B, H, context, None) != 0 and b"null output" in handle.amdspeech_last_error()
    # ranges that overlap by one word, on either side
    for off in (0, size - 4, -(size - 4)):
        other = ctypes.c_void_p(x.value + off)
        assert handle.amdspeech_lookahead_fwd(None, x, w, n, T, B, H, context, other) != 0
        assert b"x and y overlap" in handle.amdspeech_last_error()
        assert handle.amdspeech_lookahead_bwd(None, x, w, y, n, T, B, H, context, ctypes.c_void_p(y.value + off), dw, ws) != 0
        assert b"dy and dx overlap" in handle.amdspeech_last_error()
        assert handle.amdspeech_lookahead_bwd(None, x, w, y, n, T, B, H, context, other, dw, ws) != 0
        assert b"x and dx overlap" in handle.amdspeech_last_error()


# ---- the parameter layout, the initial values, the checkpoint
def test_layout_takes_the_slot_behind_output_b_and_moves_nothing():
    from rnn_speech_amd.engine import ParamLayout
    base = ParamLayout(3, 16, 5, 80)
    assert ParamLayout(3, 16, 5, 80, lookahead=0).slots == base.slots and "lookahead_w" not in base.slots
    lay = ParamLayout(3, 16, 5, 80, lookahead=7)
    assert lay.names() == base.names() + ["lookahead_w"]
    assert {k: v for k, v in lay.slots.items() if k != "lookahead_w"} == base.slots
    off, shape = lay.slots["lookahead_w"]
    assert off == base.total and shape == (8, 16) and off % 64 == 0 and lay.total == base.total + 128
    assert (lay.kernel_stride, lay.bias_stride) == (base.kernel_stride, base.bias_stride)
    assert lay.num_params() == base.num_params() + 8 * 16


def _store(lookahead, seed=5):
    from rnn_speech_amd.engine import ParamLayout, ParamStore
    store = ParamStore(ParamLayout(2, 8, 5, 80, lookahead=lookahead), "cpu")
    store.init_parameters(seed)
    return store


def test_initial_taps_are_the_identity_and_draw_nothing():
    plain, la = _store(0), _store(4)
    w = la.p("lookahead_w").numpy()
    assert (w[0] == 1.0).all() and not w[1:].any()
    for k, v in plain.to_numpy().items():
        assert np.array_equal(v, la.to_numpy()[k]), k
    assert np.array_equal(plain.params.numpy(), la.params.numpy()[:plain.layout.total])


def test_tf_name_of_the_taps():
    from rnn_speech_amd import checkpoint
    assert checkpoint.tf_name("lookahead_w") == "Lookahead_Layer/lookahead_w"
    assert checkpoint.tf_name("lookahead_w", layerwise=True) == "Lookahead_Layer/lookahead_w"
    assert checkpoint.tf_name("kernel_1") == "rnn/multi_rnn_cell/cell_1/basic_lstm_cell/kernel"


def test_native_checkpoint_round_trip_with_and_without_the_taps(tmp_path):
    from rnn_speech_amd import checkpoint
    rng = np.random.RandomState(3)
    la = _store(4)
    for flat in (la.params, la.adam_m, la.adam_v):
        flat.copy_(__import__("torch").as_tensor(rng.randn(la.layout.total).astype(np.float32)))
    la.adam_step = 9
    arrays = checkpoint.pack(la, 17, 2e-4)
    name = "Lookahead_Layer/lookahead_w"
    assert arrays[name].shape == (5, 8) and arrays["adam/m/" + name].shape == (5, 8) and arrays["adam/v/" + name].shape == (5, 8)
    path = str(tmp_path / "with.npz")
    checkpoint.write(path, arrays)
    back = _store(4, seed=99)
    assert checkpoint.unpack(np.load(path), back) == (17, float(np.float32(2e-4)), True)
    assert back.adam_step == 9
    for flat_a, flat_b in ((la.params, back.params), (la.adam_m, back.adam_m), (la.adam_v, back.adam_v)):
        a, b = la.to_numpy(flat_a), back.to_numpy(flat_b)
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # without the key: the file of today, byte for byte
    plain = _store(0)
    from rnn_speech_amd.engine import ParamLayout, ParamStore
    today = ParamStore(ParamLayout(2, 8, 5, 80), "cpu")
    today.init_parameters(5)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    checkpoint.write(pa, checkpoint.pack(plain, 1, 1e-3))
    checkpoint.write(pb, checkpoint.pack(today, 1, 1e-3))
    assert not any("ookahead" in k for k in np.load(pa).files)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    # a checkpoint without the taps does not load into a model with them
    with pytest.raises(KeyError):
        checkpoint.unpack(np.load(pa), _store(4))


def test_tf_bundle_round_trip_with_the_taps_and_their_adam_slots(handle, tmp_path):
    from rnn_speech_amd import checkpoint, tf_bundle
    import torch
    rng = np.random.RandomState(4)
    la = _store(4)
    for flat in (la.params, la.adam_m, la.adam_v):
        flat.copy_(torch.as_tensor(rng.randn(la.layout.total).astype(np.float32)))
    la.adam_step = 6
    arrays = {k: v for k, v in checkpoint.pack(la, 8, 1e-3).items() if np.asarray(v).dtype in (np.float32, np.int32)}
    prefix = str(tmp_path / "acousticmodel.ckpt-8")
    tf_bundle.write_bundle(prefix, arrays)
    assert tf_bundle.verify_index_checksums(prefix + ".index")
    z = tf_bundle.read_bundle(prefix)
    for slot in ("", "adam/m/", "adam/v/"):
        assert np.array_equal(z[slot + "Lookahead_Layer/lookahead_w"], arrays[slot + "Lookahead_Layer/lookahead_w"])
    back = _store(4, seed=99)
    checkpoint.unpack(z, back)                  # (the bundle holds no int64 adam/step: the parameters arrive, Adam restarts cold)
    assert all(np.array_equal(v, la.to_numpy()[k]) for k, v in back.to_numpy().items())


# ---- the config key
def _config(tmp_path, text_from, text_to):
    src = open(os.path.join(ROOT, "config.ini")).read()
    assert src.count(text_from) >= 1
    path = str(tmp_path / "config.ini")
    with open(path, "w") as fh:
        fh.write(src.replace(text_from, text_to, 1).replace("checkpoint_dir : ", "checkpoint_dir : %s/ckpt_" % tmp_path, 1))
    return path


def test_config_key_default_range_and_bidirectional(tmp_path):
    from rnn_speech_amd import hyperparams as hp
    assert hp.read_config_file(os.path.join(ROOT, "config.ini"))["lookahead_context"] == 0
    assert hp.read_config_file(_config(tmp_path, "lookahead_context : 0\n", ""))["lookahead_context"] == 0        # an older config.ini
    assert hp.read_config_file(_config(tmp_path, "lookahead_context : 0", "lookahead_context : 20"))["lookahead_context"] == 20
    assert hp.read_config_file(_config(tmp_path, "lookahead_context : 0", "lookahead_context : 32"))["lookahead_context"] == 32
    for bad in ("33", "-1"):
        with pytest.raises(ValueError, match="lookahead_context must be in 0 .. 32"):
            hp.read_config_file(_config(tmp_path, "lookahead_context : 0", "lookahead_context : " + bad))
    both = _config(tmp_path, "lookahead_context : 0", "lookahead_context : 4")
    src = open(both).read()
    with open(both, "w") as fh:
        fh.write(src.replace("bidirectional : False", "bidirectional : True", 1))
    with pytest.raises(ValueError, match="lookahead_context : 4 with bidirectional : True"):
        hp.read_config_file(both)


def test_config_key_is_structural_with_a_compatibility_default(tmp_path):
    import pickle
    from rnn_speech_amd import hyperparams as hp
    assert "lookahead_context" in hp._STRUCTURAL and hp._STRUCTURAL_DEFAULTS["lookahead_context"] == 0
    handler = hp.HyperParameterHandler(_config(tmp_path, "lookahead_context : 0", "lookahead_context : 0"))
    params = dict(handler.get_hyper_params())
    assert not handler.check_changed(params)
    assert handler.check_changed(dict(params, lookahead_context=5))
    old = {k: v for k, v in params.items() if k != "lookahead_context"}          # a pickle from before the key existed
    with open(handler.file_path, "wb") as fh:
        pickle.dump(old, fh)
    assert not handler.check_changed(params)
    assert handler.check_changed(dict(params, lookahead_context=5))


def test_model_passes_the_key_to_the_engine():
    import inspect
    from rnn_speech_amd import acoustic_model, engine
    import stt
    assert inspect.signature(engine.Engine.__init__).parameters["lookahead"].default == 0
    assert "lookahead=int(self.lookahead_context)" in inspect.getsource(acoustic_model.AcousticModel._make_engine)

    class Model(object):
        pass

    m = Model()
    stt._set_model_options(m, {"lookahead_context": 7})
    assert m.lookahead_context == 7
    stt._set_model_options(m, {})
    assert m.lookahead_context == 0
