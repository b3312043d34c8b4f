"""The lookahead-convolution kernels through ops against the float64 reference (tests/lookahead_ref.py), within the bounds derived
there: ragged lengths (0, 1, context, context + 1, T), NaN wherever the kernels must not read and wherever they must write, a
pre-filled dw, exact zeros past the lengths, bit-identical repeats, identity weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookahead_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _poisoned(a, lengths):
    """a with NaN at and past each row's length."""
    a = a.copy()
    T = a.shape[0]
    dead = np.arange(T)[:, None] >= ref.clip_lengths(lengths, T)[None, :]
    a[dead] = np.nan
    return a


def _aligned_or_not(arr, aligned):
    """A device copy of arr: from a 16-byte aligned base, or from one that is 4 bytes past it."""
    flat = torch.empty(arr.size + 1, device="cuda", dtype=torch.float32)
    view = flat[0:arr.size] if aligned else flat[1:arr.size + 1]
    view = view.view(*arr.shape)
    view.copy_(torch.as_tensor(arr))
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


def _check_case(T, B, H, context, lengths, rng, aligned=True):
    from rnn_speech_amd import ops
    plan = ops.lookahead_plan(T, B, H, context)
    x = rng.randn(T, B, H).astype(np.float32)
    dy = rng.randn(T, B, H).astype(np.float32)
    w = (rng.randn(context + 1, H) * 0.5).astype(np.float32)
    dw0 = rng.randn(context + 1, H).astype(np.float32)
    dev = lambda a: _aligned_or_not(a, aligned)
    xd, dyd, wd = dev(_poisoned(x, lengths)), dev(_poisoned(dy, lengths)), dev(w)
    ld = torch.as_tensor(np.asarray(lengths, np.int32)).cuda()
    nan = np.full((T, B, H), np.nan, np.float32)
    ws = ops.LookaheadWorkspace(T, B, H, context)
    assert ws.buf.numel() >= plan["dw_partials"] * (context + 1) * H * 4

    def run():
        yd, dxd, dwd = dev(nan), dev(nan), dev(dw0)
        ws.buf.view(torch.float32)[:] = float("nan")
        ops.lookahead_fwd(xd, wd, ld, out=yd)
        ops.lookahead_bwd(xd, wd, dyd, ld, dx=dxd, dw=dwd, ws=ws)
        torch.cuda.synchronize()
        return yd.cpu().numpy(), dxd.cpu().numpy(), dwd.cpu().numpy()

    y, dx, dw = run()
    y2, dx2, dw2 = run()
    tag = (T, B, H, context, list(lengths), aligned)
    for a, b in ((y, y2), (dx, dx2), (dw, dw2)):
        assert np.isfinite(a).all(), tag
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag          # two runs: the same bits

    L = ref.clip_lengths(lengths, T)
    dead = np.arange(T)[:, None] >= L[None, :]
    assert not y[dead].any() and not dx[dead].any(), tag                          # exact zeros past the lengths

    y_ref, y_abs = ref.forward(x, w, lengths), ref.forward(x, w, lengths, absolute=True)
    dx_ref, dw_ref = ref.backward(x, w, dy, lengths)
    dx_abs, dw_abs = ref.backward(x, w, dy, lengths, absolute=True)
    err_y, err_dx = np.abs(y - y_ref), np.abs(dx - dx_ref)
    print("case", tag[:4], "y err / bound %.3g" % (err_y / (ref.conv_bound(y_abs, context) + 1e-300)).max(),
          "dx %.3g" % (err_dx / (ref.conv_bound(dx_abs, context) + 1e-300)).max())
    assert (err_y <= ref.conv_bound(y_abs, context)).all(), tag
    assert (err_dx <= ref.conv_bound(dx_abs, context)).all(), tag
    n_terms = np.array([np.maximum(L - j, 0).sum() for j in range(context + 1)])[:, None]
    bound = np.stack([ref.dw_bound(dw_abs[j], dw0[j], plan, n_terms[j, 0]) for j in range(context + 1)])
    err_dw = np.abs(dw - (dw0.astype(np.float64) + dw_ref))
    print("     dw err / bound %.3g (depth %d)" % ((err_dw / (bound + 1e-300)).max(), ref.dw_tree_depth(plan)))
    assert (err_dw <= bound).all(), tag

    # identity weights: y == x as numbers inside the lengths
    ident = np.zeros((context + 1, H), np.float32)
    ident[0] = 1.0
    yi = ops.lookahead_fwd(xd, dev(ident), ld, out=dev(nan)).cpu().numpy()
    live = ~dead
    assert np.array_equal(yi[live], x[live]), tag
    assert not yi[dead].any(), tag


@pytest.mark.parametrize("T,B,H,context", ref.CASES)
def test_kernels_match_the_float64_reference(T, B, H, context):
    rng = np.random.RandomState(T * 1000 + B * 10 + context)
    for lengths in ref.length_sets(T, B, context, rng):
        lengths = lengths.copy()
        if B >= 6:
            lengths[-1] = T + 3                       # a count past T is clipped to it
        _check_case(T, B, H, context, lengths, rng)


def test_unaligned_bases_take_the_single_word_path():
    T, B, H, context = 33, 2, 20, 4
    rng = np.random.RandomState(5)
    for lengths in ref.length_sets(T, B, context, rng):
        _check_case(T, B, H, context, lengths, rng, aligned=False)


def test_chunk_edges():
    """T = 3 * t_chunk + 1 with lengths on both sides of every chunk boundary."""
    from rnn_speech_amd import ops
    B, H, context = 2, 64, 32
    tc = ops.lookahead_plan(1000, B, H, context)["t_chunk"]
    T = 3 * tc + 1
    plan = ops.lookahead_plan(T, B, H, context)
    assert plan["t_chunk"] == tc and plan["chunks"] == 4
    rng = np.random.RandomState(11)
    for lengths in ref.length_sets(T, B, context, rng, extra=(tc - 1, tc, tc + 1, 2 * tc)):
        _check_case(T, B, H, context, lengths, rng)


def test_argument_checks_refuse_without_a_launch():
    from rnn_speech_amd import lib as L, ops
    x = torch.zeros(6, 2, 16, device="cuda")
    w = torch.zeros(3, 16, device="cuda")
    n = torch.full((2,), 6, device="cuda", dtype=torch.int32)
    with pytest.raises(L.AmdSpeechError, match="overlap"):
        ops.lookahead_fwd(x, w, n, out=x)
    with pytest.raises(L.AmdSpeechError, match="overlap"):
        ops.lookahead_bwd(x, w, x, n, dx=x)
    with pytest.raises(L.AmdSpeechError, match="context 33 outside 1 .. 32"):
        ops.lookahead_fwd(x, torch.zeros(34, 16, device="cuda"), n)
    torch.cuda.synchronize()
