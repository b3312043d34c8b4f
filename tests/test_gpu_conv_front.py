"""The front convolution's kernels through ops against the float64 reference (tests/conv_front_ref.py), within the bounds derived
there: ragged lengths (0, 1, st, st + 1, pt, pt + 1, T), NaN wherever the kernels must not read and wherever they must write, exact
model lengths, pre-filled dw / db, exact zeros past the lengths, bit-identical repeats (also beside another stream's kernel), bases
that are not 16-byte aligned, refusals without a launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_front_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _poisoned(a, n_live):
    """a [T,B,...] with NaN at and past each row's count of live frames."""
    a = a.copy()
    a[np.arange(a.shape[0])[:, None] >= np.asarray(n_live)[None, :]] = np.nan
    return a


def _dev(arr, aligned=True):
    """A device copy of arr: from a 16-byte aligned base, or from one that is 4 bytes past it."""
    flat = torch.empty(arr.size + 1, device="cuda", dtype=torch.float32)
    view = (flat[0:arr.size] if aligned else flat[1:arr.size + 1]).view(*arr.shape)
    view.copy_(torch.as_tensor(arr))
    assert (view.data_ptr() % 16 == 0) == aligned
    return view


def _check_case(case, lengths, rng, aligned=True, busy=False):
    from rnn_speech_amd import ops
    T, B, G, F, C, kt, kf, st, sf = case
    plan = ops.conv2d_plan(*case)
    To, Fo, K = plan["t_out"], plan["f_out"], plan["k"]
    x, w, bias, dy, dw0, db0 = ref.case_data(case, rng)
    L, Lo = ref.clip_lengths(lengths, T), ref.model_lengths(lengths, T, st)
    dev = lambda a: _dev(a, aligned)
    xd, wd, bd = dev(_poisoned(x, L)), dev(w), dev(bias)
    ld = torch.as_tensor(np.asarray(lengths, np.int32)).cuda()
    nan = np.full((To, B, Fo * C), np.nan, np.float32)
    ws = ops.Conv2dWorkspace(*case)
    assert ws.buf.numel() >= plan["dw_partials"] * plan["k_rows"] * C * 4
    tag = (case, list(lengths), aligned, busy)

    y_ref, pre = ref.forward(x, w, bias, lengths, G, F, kt, kf, st, sf)
    _, abs_pre = ref.forward(x, w, bias, lengths, G, F, kt, kf, st, sf, absolute=True)

    side = torch.cuda.Stream() if busy else None
    a_busy = torch.randn(1024, 1024, device="cuda") if busy else None

    def run():
        yd, lo = dev(nan), torch.full((B,), -7, device="cuda", dtype=torch.int32)
        ops.conv2d_fwd(xd, wd, bd, ld, G, (kt, kf), (st, sf), out=yd, lengths_out=lo)
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        # the backward pass gets the kernel's own y (as the engine hands it over) with NaN past the model lengths, and NaN in dy there
        ydd, dyd = dev(_poisoned(y, Lo)), dev(_poisoned(dy, Lo))
        dwd, dbd = dev(dw0), dev(db0)
        ws.buf.view(torch.float32)[:] = float("nan")
        if busy:                              # another kernel busy on a second stream while the two launches run
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(4):
                    torch.mm(a_busy, a_busy)
        ops.conv2d_bwd(xd, ydd, dyd, ld, G, (kt, kf), (st, sf), dwd, dbd, ws=ws)
        torch.cuda.synchronize()
        return y, lo.cpu().numpy(), dwd.cpu().numpy(), dbd.cpu().numpy()

    y, lo, dw, db = run()
    y2, lo2, dw2, db2 = run()
    for a, b in ((y, y2), (dw, dw2), (db, db2)):
        assert np.isfinite(a).all(), tag
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag          # two runs: the same bits
    assert np.array_equal(lo, Lo) and np.array_equal(lo2, Lo), tag                # the model lengths are exact
    dead = np.arange(To)[:, None] >= Lo[None, :]
    assert not y[dead].any(), tag                                                 # exact zeros past the model lengths
    assert y.min() >= 0.0 and y.max() <= 20.0, tag

    bound = ref.fwd_bound(abs_pre, plan["k_pad"]).reshape(To, B, Fo * C)
    err_y = np.abs(y - y_ref)
    print("case", case, "y err / bound %.3g" % (err_y / (bound + 1e-300))[~dead].max(initial=0.0))
    assert (err_y <= bound)[~dead].all(), tag

    # the same float32 y for the kernel and the reference: the mask is exact
    dw_ref, db_ref = ref.backward(x, y, dy, lengths, G, F, kt, kf, st, sf)
    dw_abs, db_abs = ref.backward(x, y, dy, lengths, G, F, kt, kf, st, sf, absolute=True)
    n_terms = int(Lo.sum()) * Fo
    err_dw = np.abs(dw - (dw0.astype(np.float64) + dw_ref))
    err_db = np.abs(db - (db0.astype(np.float64) + db_ref))
    bw, bb = ref.dw_bound(dw_abs, dw0, plan, n_terms), ref.dw_bound(db_abs, db0, plan, n_terms)
    print("     dw err / bound %.3g, db %.3g (depth %d, terms %d)" % ((err_dw / (bw + 1e-300)).max(), (err_db / (bb + 1e-300)).max(),
                                                                    ref.dw_tree_depth(plan), n_terms))
    assert (err_dw <= bw).all() and (err_db <= bb).all(), tag
    if n_terms == 0:                          # nothing live: the pre-filled values come back as they were
        assert np.array_equal(dw, dw0) and np.array_equal(db, db0), tag
    return int((y[~dead] == 0.0).sum()), int((y[~dead] == 20.0).sum())


@pytest.mark.parametrize("case", ref.CASES, ids=["x".join(map(str, c)) for c in ref.CASES])
def test_kernels_match_the_float64_reference(case):
    T, B, G, F, C, kt, kf, st, sf = case
    rng = np.random.RandomState(T * 1000 + B * 10 + kt)
    at_zero = at_clip = 0
    for lengths in ref.length_sets(T, B, kt, st, rng):
        lengths = lengths.copy()
        if B >= 8:
            lengths[-1] = T + 3                       # a count past T is clipped to it
            lengths[-2] = -2                          # a negative one counts as 0
        z, c = _check_case(case, lengths, rng)
        at_zero, at_clip = at_zero + z, at_clip + c
    if T >= 16:                                       # both kinks of the activation are live in the data
        assert at_zero > 0 and at_clip > 0, (at_zero, at_clip)


def test_tile_edges():
    """T' one short of, at, and one past a tile edge, with lengths on both sides of every tile boundary."""
    from rnn_speech_amd import ops
    B, G, F, C, kt, kf, st, sf = 3, 3, 40, 32, 11, 21, 2, 2
    tile_t = ops.conv2d_plan(1000, B, G, F, C, kt, kf, st, sf)["tile_t"]
    rng = np.random.RandomState(11)
    for To in (2 * tile_t - 1, 2 * tile_t, 2 * tile_t + 1):
        T = To * st - 1                               # (odd: the last model frame has one source frame)
        case = (T, B, G, F, C, kt, kf, st, sf)
        plan = ops.conv2d_plan(*case)
        assert plan["tile_t"] == tile_t and plan["t_out"] == To and plan["fwd_workgroups"] == -(-To // tile_t) * B
        edge = tile_t * st
        for lengths in ref.length_sets(T, B, kt, st, rng, extra=(edge - 1, edge, edge + 1)):
            _check_case(case, lengths, rng)


def test_unaligned_bases_and_a_busy_second_stream():
    """The plan has no vector path (vec == 1): a base 4 bytes past a 16-byte boundary takes the same kernels.  And the same bits
    come back while another stream keeps the chip busy."""
    from rnn_speech_amd import ops
    case = (17, 2, 1, 20, 48, 3, 5, 3, 1)
    assert ops.conv2d_plan(*case)["vec"] == 1
    rng = np.random.RandomState(5)
    for lengths in ref.length_sets(17, 2, 3, 3, rng)[:2]:
        _check_case(case, lengths, rng, aligned=False)
    _check_case((23, 3, 3, 40, 32, 11, 21, 2, 2), np.asarray([23, 9, 14], np.int32), rng, busy=True)


def test_resident_and_streamed_weights_agree_with_the_reference():
    """(32, 5, 5) keeps the filter bank in LDS, (32, 11, 21) streams it: both paths are in the table above; here the plan says so."""
    from rnn_speech_amd import ops
    assert ops.conv2d_plan(23, 3, 3, 40, 32, 11, 21, 2, 2)["weights_resident"] == 0
    case = (19, 2, 3, 40, 32, 5, 5, 2, 1)
    assert ops.conv2d_plan(*case)["weights_resident"] == 1
    rng = np.random.RandomState(6)
    _check_case(case, np.asarray([19, 8], np.int32), rng)


def test_argument_checks_refuse_without_a_launch():
    from rnn_speech_amd import lib as L, ops
    x = torch.zeros(6, 2, 16, device="cuda")
    w = torch.zeros(9, 16, device="cuda")
    b = torch.zeros(16, device="cuda")
    n = torch.full((2,), 6, device="cuda", dtype=torch.int32)
    y = torch.full((6, 2, 256), 3.0, device="cuda")
    with pytest.raises(L.AmdSpeechError, match="kernel 4 x 4"):                  # even sizes reach the library's own check
        ops.conv2d_fwd(x, torch.zeros(16, 16, device="cuda"), b, n, 1, (4, 4), (1, 1), out=y)
    with pytest.raises(L.AmdSpeechError, match="stride 5 x 1"):
        ops.conv2d_fwd(x, w, b, n, 1, (3, 3), (5, 1))
    with pytest.raises(L.AmdSpeechError, match="24 channels"):
        ops.conv2d_fwd(x, torch.zeros(9, 24, device="cuda"), torch.zeros(24, device="cuda"), n, 1, (3, 3), (1, 1))
    big = torch.zeros(6 * 2 * 16 + 6 * 2 * 256, device="cuda")
    xin, yout = big[:192].view(6, 2, 16), big[188:188 + 3072].view(6, 2, 256)
    with pytest.raises(L.AmdSpeechError, match="x and y overlap"):
        ops.conv2d_fwd(xin, w, b, n, 1, (3, 3), (1, 1), out=yout)
    dw = torch.zeros(9 * 16 + 16, device="cuda")
    with pytest.raises(L.AmdSpeechError, match="overlap"):
        ops.conv2d_bwd(x, y, y, n, 1, (3, 3), (1, 1), dw[:144].view(9, 16), dw[140:156])
    torch.cuda.synchronize()
    assert float(y.min()) == 3.0 and float(y.max()) == 3.0 and not dw.any()       # nothing was launched
