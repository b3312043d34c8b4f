"""The language-model kernels (csrc/lm.hip) against tests/lm_ref.py, within the bounds stated there: the token lookup and its
scatter-add backward, and the softmax cross-entropy on each side of every boundary amdspeech_xent_plan reports."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402
from rnn_speech_amd import lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (1.0, float(np.float32(1.0 / 7.0)))


def _dev(a):
    return torch.as_tensor(a).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ("normal", "pm80", "equal"))
def test_xent_against_float64_on_each_side_of_every_boundary(kind):
    T, B = R.XENT_T, R.XENT_B
    for C in R.xent_class_counts(ops.xent_plan):      # (asked of the library when the test runs, not when it is collected)
        for ld in (T + 1, T + 4):
            c = R.xent_case(C, ld, kind)
            tgt = _dev(c["targets"])                  # [B, ld]: the row stride IS ld
            logits, lengths = _dev(c["logits"]), _dev(c["lengths"])
            M = np.abs(c["logits"].astype(np.float64)).max(axis=2)
            first = None
            for scale in SCALES:
                want_nll, want_g, live = R.xent_ref(c["logits"], c["targets"], c["lengths"], scale)
                loss, nll, g = ops.xent_fwd_bwd(logits, tgt, lengths, scale=scale, want_nll=True)
                torch.cuda.synchronize()
                nll_h, g_h, loss_h = nll.cpu().numpy(), g.cpu().numpy(), loss.cpu().numpy()
                tag = (C, ld, kind, scale)
                err_nll, err_g = np.abs(nll_h - want_nll), np.abs(g_h - want_g).max(axis=2)
                print("xent", tag, "nll err / bound %.3g" % (err_nll / R.nll_bound(C, M)).max(),
                      "dlogits err / bound %.3g" % (err_g / R.dlogits_bound(C, M, scale)).max())
                assert np.all(err_nll <= R.nll_bound(C, M)), tag
                assert np.all(err_g <= R.dlogits_bound(C, M, scale)), tag
                # dead positions: zero, bitwise (no -0.0, nothing left over)
                assert np.all(nll_h.view(np.uint32)[~live] == 0) and np.all(g_h.view(np.uint32)[~live] == 0), tag
                assert np.array_equal(loss_h, R.loss_rule(nll_h)), tag                    # EXACTLY the float64-sum rule
                assert np.all(np.abs(g_h.astype(np.float64).sum(axis=2)) <= R.dlogits_rowsum_bound(C, M, scale)), tag
                # the scoring call (no gradient, no nll buffer) and the aliased call give the same bits
                loss2, none_nll, none_g = ops.xent_fwd_bwd(logits, tgt, lengths, scale=scale, want_grad=False)
                assert none_nll is None and none_g is None and np.array_equal(_bits(loss2), _bits(loss)), tag
                alias = logits.clone()
                loss3, nll3, g3 = ops.xent_fwd_bwd(alias, tgt, lengths, scale=scale, dlogits=alias, want_nll=True)
                assert g3.data_ptr() == alias.data_ptr()
                assert np.array_equal(_bits(g3), _bits(g)) and np.array_equal(_bits(nll3), _bits(nll)), tag
                assert np.array_equal(_bits(loss3), _bits(loss)), tag
                if first is None:
                    first = nll_h
                else:
                    assert np.array_equal(first, nll_h), tag                              # nll does not depend on scale


@pytest.mark.parametrize("case", range(len(R.EMBED_SHAPES) + 1))
def test_embed_forward_is_exact_and_backward_is_within_the_sum_bound(case):
    c = R.embed_cases()[case]
    T, B, V, H = c["T"], c["B"], c["V"], c["H"]
    tok, lengths = _dev(c["tok"]), _dev(c["lengths"])
    w, bias, dz = _dev(c["w"]), _dev(c["bias"]), _dev(c["dz"])
    for b_dev, b_host in ((bias, c["bias"]), (None, None)):
        out = ops.embed_fwd(tok, lengths, w, b_dev, torch.full((T, B, H), 7.0, device="cuda"))
        want = R.embed_fwd_ref(c["tok"], c["lengths"], T, c["w"], b_host).astype(np.float32)
        assert np.array_equal(out.cpu().numpy(), want), (V, H, b_host is None)

    dw_sum, db_sum, aw, ab, n_dw, n_db = R.embed_bwd_ref(c["tok"], c["lengths"], T, c["dz"], V)
    rng = np.random.RandomState(5)
    dw0, db0 = rng.randn(V, H).astype(np.float32), rng.randn(H).astype(np.float32)

    def run(times, with_bias=True):
        dw, db = _dev(dw0), _dev(db0) if with_bias else None
        for _ in range(times):
            ops.embed_bwd(tok, lengths, dz, dw, db)
        torch.cuda.synchronize()
        return dw.cpu().numpy(), db.cpu().numpy() if with_bias else None

    dw1, db1 = run(1)
    absent = n_dw == 0
    assert absent.any() or V == 1 or c["skew"]
    assert np.array_equal(dw1.view(np.uint32)[absent], dw0.view(np.uint32)[absent])       # rows of absent tokens keep their bits
    # one call: dw0 + the n terms, n + 1 terms in all
    bound_w = R.sum_bound((n_dw + 1)[:, None], np.abs(dw0) + aw)
    bound_b = R.sum_bound(n_db + 1, np.abs(db0) + ab)
    err_w, err_b = np.abs(dw1 - (dw0 + dw_sum)), np.abs(db1 - (db0 + db_sum))
    print("embed_bwd", (V, H, T, B), "dw err / bound %.3g" % (err_w[~absent] / bound_w[~absent]).max(),
          "dbias err / bound %.3g" % (err_b / bound_b).max())
    assert np.all(err_w <= bound_w) and np.all(err_b <= bound_b)
    # two calls accumulate: dw0 + twice the sum, 2 n + 1 terms
    dw2, db2 = run(2)
    assert np.all(np.abs(dw2 - (dw0 + 2 * dw_sum)) <= R.sum_bound((2 * n_dw + 1)[:, None], np.abs(dw0) + 2 * aw))
    assert np.all(np.abs(db2 - (db0 + 2 * db_sum)) <= R.sum_bound(2 * n_db + 1, np.abs(db0) + 2 * ab))
    # two fresh runs: the same bits; without a bias gradient: the same dw
    dw1b, db1b = run(1)
    assert np.array_equal(dw1.view(np.uint32), dw1b.view(np.uint32)) and np.array_equal(db1.view(np.uint32), db1b.view(np.uint32))
    dw1c, _ = run(1, with_bias=False)
    assert np.array_equal(dw1.view(np.uint32), dw1c.view(np.uint32))


def test_bad_arguments_are_refused_with_a_message():
    h = lib.load()
    T, B, V, H, C = 4, 2, 5, 8, 6
    tok = torch.zeros(B, T + 1, dtype=torch.int32, device="cuda")
    lengths = torch.full((B,), T, dtype=torch.int32, device="cuda")
    buf = torch.zeros(T * B * 16, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    null = ctypes.c_void_p(0)

    def refused(rc, text):
        assert rc == -1, rc                           # AMDSPEECH_EINVAL
        assert text in h.amdspeech_last_error().decode(), h.amdspeech_last_error()

    refused(h.amdspeech_embed_fwd(None, p(tok), T + 1, p(lengths), T, B, V, 6, p(buf), null, p(buf)), "multiple of 4")
    refused(h.amdspeech_embed_fwd(None, null, T + 1, p(lengths), T, B, V, H, p(buf), null, p(buf)), "null")
    refused(h.amdspeech_embed_fwd(None, p(tok), T + 1, p(lengths), T, B, V, H, null, null, p(buf)), "null")
    refused(h.amdspeech_embed_fwd(None, p(tok), T - 1, p(lengths), T, B, V, H, p(buf), null, p(buf)), "below T")
    refused(h.amdspeech_embed_bwd(None, p(tok), T + 1, p(lengths), T, B, V, 6, p(buf), p(buf), null, p(ws)), "multiple of 4")
    refused(h.amdspeech_embed_bwd(None, p(tok), T + 1, p(lengths), T, B, V, H, p(buf), null, null, p(ws)), "null")
    refused(h.amdspeech_embed_bwd(None, p(tok), T + 1, p(lengths), T, B, V, H, p(buf), p(buf), null, null), "null")
    assert h.amdspeech_embed_bwd_workspace_bytes(T, B, V, 6) == 0 and h.amdspeech_embed_bwd_workspace_bytes(T, B, V, H) > 0
    for bad_c in (1, 4097):
        refused(h.amdspeech_xent_fwd_bwd(None, p(buf), p(tok), T + 1, p(lengths), T, B, bad_c, 1.0, null, p(buf), null, p(ws)), "outside 2")
        assert h.amdspeech_xent_workspace_bytes(T, B, bad_c) == 0
    refused(h.amdspeech_xent_fwd_bwd(None, null, p(tok), T + 1, p(lengths), T, B, C, 1.0, null, p(buf), null, p(ws)), "null")
    refused(h.amdspeech_xent_fwd_bwd(None, p(buf), p(tok), T + 1, p(lengths), T, B, C, 1.0, null, null, null, p(ws)), "null")
    refused(h.amdspeech_xent_fwd_bwd(None, p(buf), null, T + 1, p(lengths), T, B, C, 1.0, null, p(buf), null, p(ws)), "null")
    refused(h.amdspeech_xent_fwd_bwd(None, p(buf), p(tok), T + 1, p(lengths), T, B, C, 1.0, null, p(buf), null, null), "null")
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.embed_fwd(tok[:, :T - 1], lengths, buf[:V * H].view(V, H), None, buf[:T * B * H].view(T, B, H))
