"""The front time-frequency convolution, everything that needs no GPU: the numpy reference against torch's conv2d in float64 and
against central differences, the header section, the exported symbols and the plan query of the C ABI, what the calls refuse, the
parameter layout, the checkpoint names and round trips, the config keys, and the condition the model-level oracle puts on its
inputs (the activation's kinks)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_front_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("amdspeech_conv2d_fwd", "amdspeech_conv2d_bwd_workspace_bytes", "amdspeech_conv2d_bwd", "amdspeech_conv2d_plan")
FIELDS = ["t_out", "f_out", "k", "k_pad", "tile_t", "tile_f", "vec", "fwd_workgroups", "fwd_lds_bytes", "weights_resident", "k_chunk",
          "k_rows", "k_groups", "dw_partials", "bwd_workgroups", "bwd_lds_bytes", "dw_terms", "reduce_slices", "reduce_terms",
          "reduce_workgroups"]


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import lib
    return lib.load()


# ---- the reference
REF_CASES = [(9, 3, 1, 7, 4, 3, 3, 1, 1, [9, 4, 0]), (10, 2, 3, 6, 5, 5, 3, 2, 2, [10, 3]), (7, 2, 2, 9, 3, 11, 7, 3, 4, [9, 5]),
             (6, 1, 1, 5, 2, 1, 1, 4, 1, [6])]


def _torch_forward(x, w, bias, lengths, G, F, kt, kf, st, sf):
    """The same layer from torch.nn.functional.conv2d in float64: mask the input rows, pad, stride, clip, mask the output rows."""
    import torch
    T, B, _ = x.shape
    L = ref.clip_lengths(lengths, T)
    live = np.arange(T)[:, None] < L[None, :]
    xm = np.where(live[:, :, None], x, 0.0).reshape(T, B, G, F).transpose(1, 2, 0, 3)            # [B, G, T, F]
    K, C = w.shape
    wt = w.reshape(G, kt, kf, C).transpose(3, 0, 1, 2)                                             # [C, G, kt, kf]
    out = torch.nn.functional.conv2d(torch.as_tensor(np.ascontiguousarray(xm)), torch.as_tensor(np.ascontiguousarray(wt)),
                                     torch.as_tensor(bias), stride=(st, sf), padding=((kt - 1) // 2, (kf - 1) // 2))
    pre = out.numpy().transpose(2, 0, 3, 1)                                                        # [T', B, F', C]
    To = pre.shape[0]
    live_o = np.arange(To)[:, None] < ref.model_lengths(lengths, T, st)[None, :]
    y = np.where(live_o[:, :, None, None], np.clip(pre, 0.0, 20.0), 0.0)
    return y.reshape(To, B, -1), pre


@pytest.mark.parametrize("T,B,G,F,C,kt,kf,st,sf,lengths", REF_CASES)
def test_reference_forward_is_torch_conv2d(T, B, G, F, C, kt, kf, st, sf, lengths):
    rng = np.random.RandomState(T + kf)
    x, w, bias = rng.randn(T, B, G * F), rng.randn(G * kt * kf, C), rng.randn(C) * 4 + 8
    y, pre = ref.forward(x, w, bias, lengths, G, F, kt, kf, st, sf)
    yt, pret = _torch_forward(x, w, bias, lengths, G, F, kt, kf, st, sf)
    assert y.shape == yt.shape == (-(-T // st), B, -(-F // sf) * C)
    assert np.abs(pre - pret).max() < 1e-12 * (1 + np.abs(pret).max())
    assert np.abs(y - yt).max() < 1e-12 * (1 + np.abs(yt).max())
    assert (y == 20.0).any() or C < 3 or (pre < 20).all()
    # frames past the lengths are never read: NaN there changes nothing
    xn = x.copy()
    xn[np.arange(T)[:, None] >= ref.clip_lengths(lengths, T)[None, :]] = np.nan
    assert np.array_equal(ref.forward(xn, w, bias, lengths, G, F, kt, kf, st, sf)[0], y)
    # the absolute variant bounds the plain one
    _, apre = ref.forward(x, w, bias, lengths, G, F, kt, kf, st, sf, absolute=True)
    assert (np.abs(pre) <= apre * (1 + 1e-12)).all()


@pytest.mark.parametrize("T,B,G,F,C,kt,kf,st,sf,lengths", REF_CASES)
def test_reference_backward_is_the_gradient_of_its_forward(T, B, G, F, C, kt, kf, st, sf, lengths):
    rng = np.random.RandomState(T * 7 + kf)
    x, w, bias = rng.randn(T, B, G * F), rng.randn(G * kt * kf, C) * 0.5, rng.randn(C) * 4 + 8
    y, _ = ref.forward(x, w, bias, lengths, G, F, kt, kf, st, sf)
    dy = rng.randn(*y.shape)

    def f(w_, b_):
        return float((ref.forward(x, w_, b_, lengths, G, F, kt, kf, st, sf)[0] * dy).sum())

    dw, db = ref.backward(x, y, dy, lengths, G, F, kt, kf, st, sf)
    adw, adb = ref.backward(x, y, dy, lengths, G, F, kt, kf, st, sf, absolute=True)
    assert (np.abs(dw) <= adw * (1 + 1e-12)).all() and (np.abs(db) <= adb * (1 + 1e-12)).all()
    eps = 1e-6
    for _ in range(12):
        k, c = rng.randint(w.shape[0]), rng.randint(C)
        wp, wm = w.copy(), w.copy()
        wp[k, c] += eps
        wm[k, c] -= eps
        assert abs((f(wp, bias) - f(wm, bias)) / (2 * eps) - dw[k, c]) < 1e-6 * (1 + abs(dw[k, c])), (k, c)
    for c in range(C):
        bp, bm = bias.copy(), bias.copy()
        bp[c] += eps
        bm[c] -= eps
        assert abs((f(w, bp) - f(w, bm)) / (2 * eps) - db[c]) < 1e-6 * (1 + abs(db[c])), c
    # NaN past the lengths of dy and y never shows
    dead = np.arange(y.shape[0])[:, None] >= ref.model_lengths(lengths, T, st)[None, :]
    yn, dyn = y.copy(), dy.copy()
    yn[dead] = np.nan
    dyn[dead] = np.nan
    dw2, db2 = ref.backward(x, yn, dyn, lengths, G, F, kt, kf, st, sf)
    assert np.array_equal(dw, dw2) and np.array_equal(db, db2)


def test_length_sets_hold_the_edge_lengths():
    rng = np.random.RandomState(1)
    for T, B, G, F, C, kt, kf, st, sf in ref.CASES:
        sets = ref.length_sets(T, B, kt, st, rng)
        seen = set(int(v) for s in sets for v in s)
        assert all(len(s) == B for s in sets)
        pt = (kt - 1) // 2
        assert {v for v in (0, 1, st, st + 1, pt, pt + 1, T) if v <= T} <= seen, (T, B, kt, st)


# ---- header, symbols, plan
def test_header_section_prototypes_and_struct(handle):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    assert header.count("time-frequency convolution (front) ---") == 1
    section = header.split("time-frequency convolution (front) ---")[1].split("voice activity / long recordings ---")[0]
    for name in SYMBOLS:
        proto = re.search(r"\b%s\(([^)]*)\);" % name, section)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(lib.PROTOTYPES[name][1]), name
        assert getattr(handle, name)
    decl = section.split("typedef struct amdspeech_conv2d_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == FIELDS
    assert [n for n, _ in lib.Conv2dPlanInfo._fields_] == FIELDS
    assert ctypes.sizeof(lib.Conv2dPlanInfo) == 4 * len(FIELDS)
    for word in ("ACCUMULATE", "never read", "EVERY element", "v_mfma_f32_16x16x4_f32", "No\n * floating-point atomics", "AMDSPEECH_EINVAL"):
        assert word in section, word


def expected_plan(T, B, G, F, C, kt, kf, st, sf):
    """The tile arithmetic the header states, restated."""
    ceil = lambda a, b: -(-a // b)
    To, Fo = ceil(T, st), ceil(F, sf)
    K = G * kt * kf
    k_pad = ceil(K, 4) * 4
    row = G * (F + kf - 1)
    stride = {16: 16, 32: 48, 48: 48, 64: 80}[C]
    fixed_fwd = k_pad * 4 + 64 * stride * 4
    fixed_bwd = 128 * 4 + 128 * stride * 4
    patch = lambda tt: ((tt - 1) * st + kt) * row * 4
    tile_t = 128 // Fo
    while tile_t > 1 and patch(tile_t) + max(fixed_fwd, fixed_bwd) > 65536:
        tile_t -= 1
    resident_bytes = patch(tile_t) + k_pad * 4 + k_pad * stride * 4
    resident = resident_bytes <= 65536
    tiles = ceil(To, tile_t) * B
    k_rows = ceil(K + 1, 16) * 16
    k_groups = ceil(k_rows, 256)
    partials = min(tiles, ceil(512, k_groups))
    return dict(t_out=To, f_out=Fo, k=K, k_pad=k_pad, tile_t=tile_t, tile_f=Fo, vec=1, fwd_workgroups=tiles,
                fwd_lds_bytes=resident_bytes if resident else patch(tile_t) + fixed_fwd, weights_resident=int(resident),
                k_chunk=k_pad if resident else 64, k_rows=k_rows, k_groups=k_groups, dw_partials=partials,
                bwd_workgroups=partials * k_groups, bwd_lds_bytes=patch(tile_t) + fixed_bwd,
                dw_terms=ceil(tiles, partials) * tile_t * Fo, reduce_slices=8, reduce_terms=ceil(partials, 8),
                reduce_workgroups=ceil((K + 1) * C, 32))


HEADLINE = [(1001, 32, 3, 40, 32, 11, 21, 2, 2), (998, 64, 3, 40, 32, 11, 21, 2, 2), (1001, 32, 3, 40, 32, 5, 5, 2, 1),
            (998, 64, 3, 40, 32, 5, 5, 2, 1)]


@pytest.mark.parametrize("case", ref.CASES + ref.LIMIT_CASES + HEADLINE)
def test_plan_reports_the_geometry_without_a_device(handle, case):
    from rnn_speech_amd import ops
    T, B, G, F, C, kt, kf, st, sf = case
    plan = ops.conv2d_plan(*case)
    assert {k: plan[k] for k in FIELDS} == expected_plan(*case)
    # a tile is at most 128 positions of one row, the tiles cover T', K is padded to the instruction's 4
    assert 1 <= plan["tile_t"] * plan["tile_f"] <= 128 and plan["tile_f"] == plan["f_out"]
    assert plan["k_pad"] % 4 == 0 and 0 <= plan["k_pad"] - plan["k"] < 4
    assert plan["k_chunk"] % 4 == 0 and (plan["k_chunk"] == plan["k_pad"]) == bool(plan["weights_resident"])
    assert plan["fwd_lds_bytes"] <= 160 * 1024 and plan["bwd_lds_bytes"] <= 160 * 1024
    assert plan["k_rows"] >= plan["k"] + 1 and plan["k_groups"] * 256 >= plan["k_rows"]
    # every tile is summed into exactly one partial, and dw_terms is the most positions one partial sums
    assert plan["dw_partials"] <= plan["fwd_workgroups"]
    assert plan["dw_terms"] * plan["dw_partials"] >= plan["fwd_workgroups"] * plan["tile_t"] * plan["tile_f"]
    # the workspace covers the plan's partial tiles, and those of every shorter run at the same other sizes
    assert plan["workspace_bytes"] == plan["dw_partials"] * plan["k_rows"] * C * 4
    assert plan["workspace_bytes"] == handle.amdspeech_conv2d_bwd_workspace_bytes(*case)
    for t in sorted({1, 2, st, st + 1, T // 3 + 1, T // 2 + 1, T - 1, T} - {0}):
        if t <= T:
            short = ops.conv2d_plan(t, *case[1:])
            assert short["tile_t"] == plan["tile_t"] and short["k_rows"] == plan["k_rows"]
            assert short["dw_partials"] * short["k_rows"] * C * 4 <= plan["workspace_bytes"], t
    assert ref.dw_tree_depth(plan) == plan["dw_terms"] + plan["reduce_terms"] + 8 + 1


def test_plan_streams_the_large_filter_bank_and_keeps_the_small_one(handle):
    from rnn_speech_amd import ops
    big, small = ops.conv2d_plan(1001, 32, 3, 40, 32, 11, 21, 2, 2), ops.conv2d_plan(1001, 32, 3, 40, 32, 5, 5, 2, 1)
    assert (big["k"], big["k_pad"], big["weights_resident"], big["k_chunk"], big["tile_t"]) == (693, 696, 0, 64, 6)
    assert (small["k"], small["k_pad"], small["weights_resident"], small["k_chunk"], small["tile_t"]) == (75, 76, 1, 76, 3)
    assert big["fwd_workgroups"] >= 2 * 256 and big["bwd_workgroups"] >= 256          # the grids cover the 256 CUs


BAD_SHAPES = [
    ((0, 2, 1, 16, 16, 3, 3, 1, 1), b"bad shape"), ((4, 0, 1, 16, 16, 3, 3, 1, 1), b"bad shape"), ((-1, 2, 1, 16, 16, 3, 3, 1, 1), b"bad shape"),
    ((4, 2, 0, 16, 16, 3, 3, 1, 1), b"G 0 outside 1 .. 3"), ((4, 2, 4, 16, 16, 3, 3, 1, 1), b"G 4 outside 1 .. 3"),
    ((4, 2, 1, 0, 16, 3, 3, 1, 1), b"F 0 outside 1 .. 128"), ((4, 2, 1, 129, 16, 3, 3, 1, 1), b"F 129 outside 1 .. 128"),
    ((4, 2, 1, 16, 0, 3, 3, 1, 1), b"0 channels"), ((4, 2, 1, 16, 24, 3, 3, 1, 1), b"24 channels"), ((4, 2, 1, 16, 80, 3, 3, 1, 1), b"80 channels"),
    ((4, 2, 1, 16, 16, 2, 3, 1, 1), b"kernel 2 x 3"), ((4, 2, 1, 16, 16, 3, 4, 1, 1), b"kernel 3 x 4"), ((4, 2, 1, 16, 16, 13, 3, 1, 1), b"kernel 13 x 3"),
    ((4, 2, 1, 16, 16, 3, 43, 1, 1), b"kernel 3 x 43"), ((4, 2, 1, 16, 16, 0, 3, 1, 1), b"kernel 0 x 3"),
    ((4, 2, 1, 16, 16, 3, 3, 0, 1), b"stride 0 x 1"), ((4, 2, 1, 16, 16, 3, 3, 1, 5), b"stride 1 x 5"),
    ((4, 2, 1, 128, 64, 3, 3, 1, 1), b"exceeds 4096"),
    ((1 << 20, 1 << 10, 1, 16, 16, 3, 3, 1, 1), b"too large"), ((1 << 16, 1 << 15, 1, 1, 16, 1, 1, 4, 1), b"too large"),
    ((4, 70000, 1, 16, 16, 3, 3, 1, 1), b"B 70000 exceeds 65535"),
]


@pytest.mark.parametrize("case,word", BAD_SHAPES)
def test_plan_and_calls_refuse_a_bad_shape(handle, case, word):
    from rnn_speech_amd import lib, ops
    info = lib.Conv2dPlanInfo()
    assert handle.amdspeech_conv2d_plan(*case, ctypes.byref(info)) != 0
    assert word in handle.amdspeech_last_error(), handle.amdspeech_last_error()
    assert handle.amdspeech_conv2d_bwd_workspace_bytes(*case) == 0
    with pytest.raises(lib.AmdSpeechError):
        ops.conv2d_plan(*case)
    # the calls check the shape as the plan does, before they touch a pointer or the device
    a, b, c, d, e, f, g = (ctypes.c_void_p(k << 40) for k in range(1, 8))
    assert handle.amdspeech_conv2d_fwd(None, a, b, c, d, *case, e, f) != 0
    assert word in handle.amdspeech_last_error()
    assert handle.amdspeech_conv2d_bwd(None, a, b, c, d, *case, e, f, g) != 0
    assert word in handle.amdspeech_last_error()


def test_calls_refuse_null_and_overlapping_pointers(handle):
    case = (6, 2, 1, 16, 16, 3, 3, 2, 1)
    x, w, bias, n, y, lo, ws = (ctypes.c_void_p(k << 40) for k in range(1, 8))
    null = ctypes.c_void_p(0)
    for k in range(6):
        args = [x, w, bias, n, y, lo]
        args[k] = null
        assert handle.amdspeech_conv2d_fwd(None, *args[:4], *case, *args[4:]) != 0
        assert b"conv2d_fwd: null pointer" in handle.amdspeech_last_error()
    for k in range(7):
        args = [x, y, w, n, bias, lo, ws]        # (x, y, dy, lengths, dw, db, ws: any distinct addresses)
        args[k] = null
        assert handle.amdspeech_conv2d_bwd(None, *args[:4], *case, *args[4:]) != 0
        assert b"conv2d_bwd: null pointer" in handle.amdspeech_last_error()
    assert handle.amdspeech_conv2d_plan(*case, None) != 0 and b"null output" in handle.amdspeech_last_error()
    x_bytes, y_bytes = 6 * 2 * 16 * 4, 3 * 2 * 16 * 16 * 4
    for other in (x.value, x.value + x_bytes - 4, x.value - (y_bytes - 4)):
        assert handle.amdspeech_conv2d_fwd(None, x, w, bias, n, *case, ctypes.c_void_p(other), lo) != 0
        assert b"x and y overlap" in handle.amdspeech_last_error()
    dw = ctypes.c_void_p(3 << 40)
    assert handle.amdspeech_conv2d_bwd(None, x, y, y, n, *case, dw, ctypes.c_void_p(dw.value + 4), ws) != 0
    assert b"dw, db and the workspace overlap" in handle.amdspeech_last_error()
    assert handle.amdspeech_conv2d_bwd(None, x, y, y, n, *case, dw, bias, dw) != 0
    assert b"dw, db and the workspace overlap" in handle.amdspeech_last_error()


# ---- the parameter layout, the initial values, the checkpoint
CONV = (32, 5, 3, 2, 2, 3)               # (C, kt, kf, st, sf, G): K = 45


def test_layout_takes_the_last_two_slots_and_moves_nothing():
    from rnn_speech_amd.engine import ParamLayout
    base = ParamLayout(3, 16, 5, 80)
    assert ParamLayout(3, 16, 5, 80, conv=None).slots == base.slots and "conv_w" not in base.slots and "conv_b" not in base.slots
    assert base.names() == ["input_w", "input_b"] + [n % l for l in range(3) for n in ("kernel_%d", "bias_%d")] + ["output_w", "output_b"]
    lay = ParamLayout(3, 16, 5, 80, conv=CONV)
    assert lay.names() == base.names() + ["conv_w", "conv_b"]
    assert {k: v for k, v in lay.slots.items() if k not in ("conv_w", "conv_b")} == base.slots
    assert lay.slots["conv_w"] == (base.total, (45, 32)) and lay.slots["conv_b"] == (base.total + 1472, (32,))
    assert lay.total == base.total + 1472 + 64 and lay.num_params() == base.num_params() + 45 * 32 + 32
    assert (lay.kernel_stride, lay.bias_stride) == (base.kernel_stride, base.bias_stride)
    # behind the lookahead taps when those exist; bidirectional layouts take them too
    both = ParamLayout(3, 16, 5, 80, lookahead=4, conv=CONV)
    assert both.names() == base.names() + ["lookahead_w", "conv_w", "conv_b"]
    bi = ParamLayout(2, 16, 5, 80, bidirectional=True, bidirectional_mode="layer", conv=CONV)
    assert bi.names()[-2:] == ["conv_w", "conv_b"]


def _store(conv, seed=5):
    from rnn_speech_amd.engine import ParamLayout, ParamStore
    store = ParamStore(ParamLayout(2, 8, 5, 80, conv=conv), "cpu")
    store.init_parameters(seed)
    return store


def test_initial_filters_are_glorot_over_the_receptive_field_and_the_bias_is_zero():
    plain, cv = _store(None), _store(CONV)
    w = cv.p("conv_w").numpy()
    lim = np.sqrt(6.0 / (45 + 5 * 3 * 32))
    assert np.abs(w).max() <= lim and np.abs(w).max() > 0.9 * lim and abs(w.mean()) < 0.1 * lim
    assert not cv.p("conv_b").numpy().any()
    for k, v in plain.to_numpy().items():                     # the other tensors draw what they draw without the layer
        assert np.array_equal(v, cv.to_numpy()[k]), k


def test_tf_names_of_the_two_tensors():
    from rnn_speech_amd import checkpoint
    assert checkpoint.tf_name("conv_w") == "Conv_Layer/conv_w" and checkpoint.tf_name("conv_b", layerwise=True) == "Conv_Layer/conv_b"


def test_native_checkpoint_round_trip_with_and_without_the_layer(tmp_path):
    import torch
    from rnn_speech_amd import checkpoint
    from rnn_speech_amd.engine import ParamLayout, ParamStore
    rng = np.random.RandomState(3)
    cv = _store(CONV)
    for flat in (cv.params, cv.adam_m, cv.adam_v):
        flat.copy_(torch.as_tensor(rng.randn(cv.layout.total).astype(np.float32)))
    cv.adam_step = 9
    arrays = checkpoint.pack(cv, 17, 2e-4)
    for slot in ("", "adam/m/", "adam/v/"):
        assert arrays[slot + "Conv_Layer/conv_w"].shape == (45, 32) and arrays[slot + "Conv_Layer/conv_b"].shape == (32,)
    path = str(tmp_path / "with.npz")
    checkpoint.write(path, arrays)
    back = _store(CONV, seed=99)
    assert checkpoint.unpack(np.load(path), back) == (17, float(np.float32(2e-4)), True)
    for flat_a, flat_b in ((cv.params, back.params), (cv.adam_m, back.adam_m), (cv.adam_v, back.adam_v)):
        a, b = cv.to_numpy(flat_a), back.to_numpy(flat_b)
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    # with the layer off: the file of today, byte for byte
    today = ParamStore(ParamLayout(2, 8, 5, 80), "cpu")
    today.init_parameters(5)
    pa, pb = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    checkpoint.write(pa, checkpoint.pack(_store(None), 1, 1e-3))
    checkpoint.write(pb, checkpoint.pack(today, 1, 1e-3))
    assert not any("onv" in k for k in np.load(pa).files)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    with pytest.raises(KeyError):                              # a checkpoint without the layer does not load into a model with it
        checkpoint.unpack(np.load(pa), _store(CONV))


def test_tf_bundle_round_trip_with_the_two_tensors(handle, tmp_path):
    import torch
    from rnn_speech_amd import checkpoint, tf_bundle
    rng = np.random.RandomState(4)
    cv = _store(CONV)
    for flat in (cv.params, cv.adam_m, cv.adam_v):
        flat.copy_(torch.as_tensor(rng.randn(cv.layout.total).astype(np.float32)))
    arrays = {k: v for k, v in checkpoint.pack(cv, 8, 1e-3).items() if np.asarray(v).dtype in (np.float32, np.int32)}
    prefix = str(tmp_path / "acousticmodel.ckpt-8")
    tf_bundle.write_bundle(prefix, arrays)
    assert tf_bundle.verify_index_checksums(prefix + ".index")
    z = tf_bundle.read_bundle(prefix)
    for slot in ("", "adam/m/", "adam/v/"):
        for name in ("Conv_Layer/conv_w", "Conv_Layer/conv_b"):
            assert np.array_equal(z[slot + name], arrays[slot + name])
    back = _store(CONV, seed=99)
    checkpoint.unpack(z, back)
    assert all(np.array_equal(v, cv.to_numpy()[k]) for k, v in back.to_numpy().items())


# ---- the config keys
def _config(tmp_path, *pairs):
    src = open(os.path.join(ROOT, "config.ini")).read()
    for text_from, text_to in pairs:
        assert src.count(text_from) >= 1, text_from
        src = src.replace(text_from, text_to, 1)
    path = str(tmp_path / "config.ini")
    with open(path, "w") as fh:
        fh.write(src.replace("checkpoint_dir : ", "checkpoint_dir : %s/ckpt_" % tmp_path, 1))
    return path


ON = ("conv_channels : 0", "conv_channels : 32")


def test_config_keys_defaults_and_parsing(tmp_path):
    from rnn_speech_amd import hyperparams as hp
    shipped = hp.read_config_file(os.path.join(ROOT, "config.ini"))
    assert (shipped["conv_channels"], shipped["conv_kernel"], shipped["conv_stride"]) == (0, (11, 21), (2, 2))
    # a file written before the keys existed: off
    old = hp.read_config_file(_config(tmp_path, ("conv_channels : 0\n", ""), ("conv_kernel : 11, 21\n", ""), ("conv_stride : 2, 2\n", "")))
    assert (old["conv_channels"], old["conv_kernel"], old["conv_stride"]) == (0, (11, 21), (2, 2))
    on = hp.read_config_file(_config(tmp_path, ON, ("conv_kernel : 11, 21", "conv_kernel : 5,3"), ("conv_stride : 2, 2", "conv_stride :  3 , 1")))
    assert (on["conv_channels"], on["conv_kernel"], on["conv_stride"]) == (32, (5, 3), (3, 1))
    for c in (16, 48, 64):
        assert hp.read_config_file(_config(tmp_path, ("conv_channels : 0", "conv_channels : %d" % c)))["conv_channels"] == c


@pytest.mark.parametrize("pairs,why", [
    ([("conv_channels : 0", "conv_channels : 24")], "conv_channels must be one of 0, 16, 32, 48, 64"),
    ([("conv_channels : 0", "conv_channels : -16")], "conv_channels must be one of"),
    ([("conv_channels : 0", "conv_channels : many")], "conv_channels must be 1 integers"),
    ([("conv_kernel : 11, 21", "conv_kernel : 11")], "conv_kernel must be 2 integers"),
    ([("conv_kernel : 11, 21", "conv_kernel : 4, 21")], "both sizes must be odd"),
    ([("conv_kernel : 11, 21", "conv_kernel : 11, 20")], "both sizes must be odd"),
    ([("conv_kernel : 11, 21", "conv_kernel : 13, 21")], "time taps 1 .. 11"),
    ([("conv_kernel : 11, 21", "conv_kernel : 11, 43")], "frequency taps 1 .. 41"),
    ([("conv_kernel : 11, 21", "conv_kernel : 0, 21")], "time taps 1 .. 11"),
    ([("conv_stride : 2, 2", "conv_stride : 5, 2")], "each stride 1 .. 4"),
    ([("conv_stride : 2, 2", "conv_stride : 2, 0")], "each stride 1 .. 4"),
    ([ON, ("frame_skip : 1", "frame_skip : 3")], "learned form of those two"),
    ([ON, ("frame_stack : 1", "frame_stack : 2")], "learned form of those two"),
    ([("conv_channels : 0", "conv_channels : 64"), ("conv_stride : 2, 2", "conv_stride : 2, 1"), ("n_mfcc : 40", "n_mfcc : 65")],
     "more than 4096"),
])
def test_config_refusals_say_why(tmp_path, pairs, why):
    from rnn_speech_amd import hyperparams as hp
    with pytest.raises(ValueError, match=re.escape(why)):
        hp.read_config_file(_config(tmp_path, *pairs))


def test_config_allows_the_layer_with_every_other_option(tmp_path):
    from rnn_speech_amd import hyperparams as hp
    d = hp.read_config_file(_config(tmp_path, ON, ("bidirectional : False", "bidirectional : True")))
    assert d["conv_channels"] == 32 and d["bidirectional"] is True
    d = hp.read_config_file(_config(tmp_path, ON, ("lookahead_context : 0", "lookahead_context : 3")))
    assert d["conv_channels"] == 32 and d["lookahead_context"] == 3


def test_config_keys_are_structural_with_compatibility_defaults(tmp_path):
    import pickle
    from rnn_speech_amd import hyperparams as hp
    assert hp._STRUCTURAL[-3:] == ("conv_channels", "conv_kernel", "conv_stride")                   # appended
    assert hp._STRUCTURAL_DEFAULTS["conv_channels"] == 0
    handler = hp.HyperParameterHandler(_config(tmp_path))
    params = dict(handler.get_hyper_params())
    assert not handler.check_changed(params)
    assert handler.check_changed(dict(params, conv_channels=32))
    assert handler.check_changed(dict(params, conv_kernel=(5, 5)))
    assert handler.check_changed(dict(params, conv_stride=(3, 2)))
    old = {k: v for k, v in params.items() if not k.startswith("conv_")}          # a pickle from before the keys existed
    with open(handler.file_path, "wb") as fh:
        pickle.dump(old, fh)
    assert not handler.check_changed(params)
    assert handler.check_changed(dict(params, conv_channels=16))


def test_stt_hands_the_keys_to_the_model_and_scales_the_alignment_times():
    import inspect
    from rnn_speech_amd import acoustic_model, engine
    import stt
    assert inspect.signature(engine.Engine.__init__).parameters["conv"].default is None
    assert "conv=self.conv" in inspect.getsource(acoustic_model.AcousticModel._make_engine)

    class Thing(object):
        pass

    m = Thing()
    stt._set_model_options(m, {})
    assert m.conv is None
    stt._set_model_options(m, {"conv_channels": 0, "conv_kernel": (5, 5), "signal_processing": "fbank"})
    assert m.conv is None
    stt._set_model_options(m, {"conv_channels": 32, "conv_kernel": (11, 21), "conv_stride": (2, 2), "signal_processing": "fbank"})
    assert m.conv == (32, 11, 21, 2, 2, 3)
    stt._set_model_options(m, {"conv_channels": 16, "conv_kernel": (3, 5), "conv_stride": (3, 1), "signal_processing": "mfcc"})
    assert m.conv == (16, 3, 5, 3, 1, 1)
    ap = Thing()
    ap.frame_hop_samples, ap.load_sr = 160, 16000
    assert stt.frame_seconds(ap) == 0.01 and stt.frame_seconds(ap, m.conv) == 0.03


def test_ops_checks_say_which_size_is_wrong():
    from rnn_speech_amd import ops
    ops.conv2d_check(32, 11, 21, 2, 2, F=40)
    assert ops.conv2d_out_shape(1001, 40, 32, 2, 2) == (501, 640) and ops.conv2d_out_shape(17, 20, 48, 3, 1) == (6, 960)
    for args, why in (((24, 3, 3, 1, 1), "conv_channels"), ((32, 4, 3, 1, 1), "odd"), ((32, 3, 43, 1, 1), "frequency taps 1 .. 41"),
                      ((32, 3, 3, 5, 1), "each 1 .. 4")):
        with pytest.raises(ValueError, match=re.escape(why)):
            ops.conv2d_check(*args)
    with pytest.raises(ValueError, match="more than 4096"):
        ops.conv2d_check(64, 3, 3, 1, 1, F=128)


# ---- the condition the model-level GPU test puts on its inputs
@pytest.mark.parametrize("cfg", ref.MODEL_CONFIGS, ids=[c[0] for c in ref.MODEL_CONFIGS])
def test_model_inputs_keep_the_undecided_outputs_rare(handle, cfg):
    """For the seeds of tests/test_gpu_conv_front_model.py: a float32-rounded forward (numpy, another summation order than the
    device's) disagrees with the float64 mask only on outputs within the forward bound of a kink, and those are at most 1e-3 of
    the live outputs -- what conv_front_ref.oracle_mask asserts on the device's y."""
    from rnn_speech_amd import ops
    C, kt, kf, st, sf, G = ref.CONV_MODEL
    x, lengths, _ = ref.model_batch(cfg)
    w, b = ref.conv_params(cfg)
    T, B, D = x.shape
    k_pad = ops.conv2d_plan(T, B, G, D // G, C, kt, kf, st, sf)["k_pad"]
    _, pre = ref.forward(x, w, b, lengths, G, D // G, kt, kf, st, sf)
    _, abs_pre = ref.forward(x, w, b, lengths, G, D // G, kt, kf, st, sf, absolute=True)
    P = ref.patches(x, lengths, G, D // G, kt, kf, st, sf).astype(np.float32)
    pre32 = (P @ w + b).astype(np.float32)
    assert (np.abs(pre32 - pre) <= ref.fwd_bound(abs_pre, k_pad)).all()
    y32 = np.clip(pre32, np.float32(0), np.float32(20)).reshape(pre.shape[0], B, -1)
    live_rows = np.arange(pre.shape[0])[:, None] < ref.model_lengths(lengths, T, st)[None, :]
    y32 = np.where(live_rows[:, :, None], y32, 0)
    mask, und, live = ref.oracle_mask(pre, abs_pre, k_pad, y32, lengths, T, st)        # (asserts both conditions)
    assert live.sum() > 1000 and und.sum() <= ref.UNDECIDED_SHARE * live.sum()
    assert mask.shape == y32.shape and 0.2 < mask.sum() / live.sum() < 0.8            # the ReLU is live on both sides
