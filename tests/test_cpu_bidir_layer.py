"""Layer-wise bidirectional stacks (bidirectional_mode = layer): the float64 checker, the parameter layout, checkpoint names and
the config key -- everything that needs no GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bidir_layer_ref as ref  # noqa: E402
from oracle import model as om  # noqa: E402


def random_params(L, H, D, C, seed=0):
    from rnn_speech_amd.engine import ParamLayout
    lay = ParamLayout(L, H, D, C, bidirectional=True, bidirectional_mode="layer")
    rng = np.random.RandomState(seed)
    return {k: rng.randn(*shape) * (0.3 if len(shape) == 2 else 0.1) for k, (_, shape) in lay.slots.items()}


def batch(T, B, D, seed=1):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, size=B)
    lengths[0] = T
    if B > 2:
        lengths[1] = 0
    return rng.randn(T, B, D), lengths


@pytest.mark.parametrize("L,H,B,T", [(1, 8, 3, 7), (2, 16, 4, 9), (3, 8, 5, 6)])
def test_reference_matches_torch_lstm(L, H, B, T):
    """The hand-written cell (the checker of the GPU tests) against torch.nn.LSTM(bidirectional=True, num_layers=L)."""
    D, C = 6, 5
    p = random_params(L, H, D, C)
    x, lengths = batch(T, B, D)
    pt = {k: torch.as_tensor(v) for k, v in p.items()}
    got, _ = ref.forward(pt, torch.as_tensor(x), lengths, L, H)
    want = ref.torch_lstm_forward(p, x, lengths, L, H)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-12)


def test_reference_one_layer_equals_the_top_joined_oracle():
    """At L = 1 the two bidirectional forms are the same function: the checker equals oracle.model.forward_bidirectional."""
    H, D, C, B, T = 8, 6, 5, 4, 9
    p = random_params(1, H, D, C, seed=3)
    x, lengths = batch(T, B, D, seed=4)
    got, _ = ref.forward({k: torch.as_tensor(v) for k, v in p.items()}, torch.as_tensor(x), lengths, 1, H)
    want, _ = om.forward_bidirectional(p, x, np.asarray(lengths, np.int32), 1)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-12)


def test_reference_masks_enter_as_dropout_wrapper():
    """Input masks multiply each cell's (reversed, for bw) input; all-ones masks change nothing, a zero input mask on the bw cell of
    layer 1 removes the bw cell's dependence on the layer below."""
    L, H, D, C, B, T = 2, 8, 6, 5, 3, 5
    p = {k: torch.as_tensor(v) for k, v in random_params(L, H, D, C, seed=5).items()}
    x, lengths = batch(T, B, D, seed=6)
    ones = {(d, w, l): torch.ones(T, B, H if (w == "out" or l == 0) else 2 * H, dtype=torch.float64)
            for d in ("fw", "bw") for w in ("in", "out") for l in range(L)}
    a, _ = ref.forward(p, torch.as_tensor(x), lengths, L, H)
    b, _ = ref.forward(p, torch.as_tensor(x), lengths, L, H, masks=ones)
    assert torch.equal(a, b)


def test_param_layout_shapes_and_strides():
    from rnn_speech_amd.engine import ParamLayout
    L, H, D, C = 3, 32, 20, 80
    lay = ParamLayout(L, H, D, C, bidirectional=True, bidirectional_mode="layer")
    for pre in ("", "bw_"):
        assert lay.slots[pre + "kernel_0"][1] == (2 * H, 4 * H)
        for l in range(1, L):
            assert lay.slots[pre + "kernel_%d" % l][1] == (3 * H, 4 * H)
            assert lay.slots[pre + "bias_%d" % l][1] == (4 * H,)
    assert lay.slots["output_w"][1] == (2 * H, C)
    assert lay.kernel_stride is None and lay.bias_stride is None          # not uniform between layers
    offs = sorted(off for off, _ in lay.slots.values())
    assert all(o % 64 == 0 for o in offs)
    n = 2 * (2 * H * 4 * H + (L - 1) * 3 * H * 4 * H + L * 4 * H) + D * H + H + 2 * H * C + C
    assert lay.num_params() == n
    top = ParamLayout(L, H, D, C, bidirectional=True)
    assert top.slots["kernel_1"][1] == (2 * H, 4 * H) and top.kernel_stride > 0      # the top-joined layout is unchanged
    one = ParamLayout(1, H, D, C, bidirectional=True, bidirectional_mode="layer")
    assert {k: s for k, (_, s) in one.slots.items()} == {k: s for k, (_, s) in ParamLayout(1, H, D, C, bidirectional=True).slots.items()}


def _namer(layerwise):
    from rnn_speech_amd.acoustic_model import AcousticModel
    stub = types.SimpleNamespace(engine=types.SimpleNamespace(layerwise=layerwise), _TF_NAMES=AcousticModel._TF_NAMES)
    return lambda name: AcousticModel._tf_name(stub, name)


def test_checkpoint_names_follow_stack_bidirectional_dynamic_rnn():
    name = _namer(True)
    assert name("kernel_0") == "stack_bidirectional_rnn/cell_0/bidirectional_rnn/fw/basic_lstm_cell/kernel"
    assert name("bias_2") == "stack_bidirectional_rnn/cell_2/bidirectional_rnn/fw/basic_lstm_cell/bias"
    assert name("bw_kernel_1") == "stack_bidirectional_rnn/cell_1/bidirectional_rnn/bw/basic_lstm_cell/kernel"
    assert name("bw_bias_0") == "stack_bidirectional_rnn/cell_0/bidirectional_rnn/bw/basic_lstm_cell/bias"
    assert name("output_w") == "Output_layer/output_w" and name("input_b") == "Input_Layer/input_b"
    top = _namer(False)
    assert top("bw_kernel_1") == "bidirectional_rnn/bw/multi_rnn_cell/cell_1/basic_lstm_cell/kernel"
    assert top("kernel_1") == "rnn/multi_rnn_cell/cell_1/basic_lstm_cell/kernel"


def test_checkpoint_round_trip_npz_and_tf_bundle(tmp_path):
    from rnn_speech_amd import tf_bundle
    name = _namer(True)
    p = {k: v.astype(np.float32) for k, v in random_params(2, 16, 6, 5, seed=8).items()}
    arrays = {name(k): v for k, v in p.items()}
    arrays["global_step"] = np.int32(3)
    arrays["learning_rate"] = np.float32(1e-3)
    np.savez(str(tmp_path / "c.npz"), **arrays)
    tf_bundle.write_bundle(str(tmp_path / "b"), arrays)
    for z in (np.load(str(tmp_path / "c.npz")), tf_bundle.read_bundle(str(tmp_path / "b"))):
        for k, v in p.items():
            np.testing.assert_array_equal(np.asarray(z[name(k)]), v)


def test_config_key_default_parse_and_structural_change(tmp_path):
    from util.hyperparams import read_config_file, HyperParameterHandler
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    cfg = tmp_path / "config.ini"
    cfg.write_text(src)
    d = read_config_file(str(cfg))
    assert d["bidirectional_mode"] == "top"
    cfg.write_text(src.replace("[acoustic_network_params]", "[acoustic_network_params]\nbidirectional_mode : layer", 1))
    assert read_config_file(str(cfg))["bidirectional_mode"] == "layer"
    cfg.write_text(src.replace("[acoustic_network_params]", "[acoustic_network_params]\nbidirectional_mode : sideways", 1))
    with pytest.raises(ValueError):
        read_config_file(str(cfg))
    cfg.write_text(src)
    h = HyperParameterHandler(str(cfg))
    old = h.get_hyper_params()
    assert not h.check_changed(old)
    legacy = dict(old)
    legacy.pop("bidirectional_mode")                   # a pickle written before the key existed compares equal
    assert not h.check_changed(legacy)
    assert h.check_changed(dict(old, bidirectional_mode="layer"))
