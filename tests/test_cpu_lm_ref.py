"""CPU checks of tests/lm_ref.py: its float64 references against torch's float64 CPU embedding / cross-entropy / autograd, the
stated rounding bounds against a float32 numpy evaluation of the same formulas on every case of the tables (the bounds are
attainable) and against two deliberately wrong variants (they have teeth), and the language-model oracle -- oracle.model on
one-hot input plus lm_ref's cross-entropy -- against central finite differences of its own loss."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_ref as R  # noqa: E402
from oracle import model as om  # noqa: E402
from rnn_speech_amd import ops  # noqa: E402


@pytest.fixture(scope="module")
def xent_cases():
    return R.xent_cases(ops.xent_plan)


def _row_max(logits):
    return np.abs(logits.astype(np.float64)).max(axis=2)


def test_the_plan_reports_boundaries_and_the_table_straddles_them():
    cs = R.xent_class_counts(ops.xent_plan)
    assert set(R.XENT_C_FIXED) <= set(cs) and cs[0] == 2 and cs[-1] == 4096
    kinds = set()
    for c in cs:
        p = ops.xent_plan(R.XENT_T, R.XENT_B, c)
        assert p["c_min"] <= c <= p["c_max"]
        assert p["values_per_lane"] * (p["threads"] // p["rows_per_workgroup"]) >= c      # a row fits its lanes' registers
        assert p["grid"] * p["rows_per_workgroup"] >= R.XENT_T * R.XENT_B
        kinds.add((p["kernel"], p["values_per_lane"]))
        if p["c_max"] < 4096:
            assert p["c_max"] in cs and p["c_max"] + 1 in cs
            q = ops.xent_plan(R.XENT_T, R.XENT_B, p["c_max"] + 1)
            assert (q["kernel"], q["values_per_lane"]) != (p["kernel"], p["values_per_lane"]) and q["c_min"] == p["c_max"] + 1
    assert {k for k, _ in kinds} == {"wave", "block"}
    for bad in (1, 4097):
        with pytest.raises(Exception, match="outside 2"):
            ops.xent_plan(R.XENT_T, R.XENT_B, bad)


def test_xent_reference_agrees_with_torch_float64(xent_cases):
    for c in xent_cases:
        if c["C"] > 300 and c["kind"] != "normal":
            continue
        T, scale = R.XENT_T, 1.0 / 7.0
        nll, g, live = R.xent_ref(c["logits"], c["targets"], c["lengths"], scale)
        x = torch.tensor(c["logits"].astype(np.float64), requires_grad=True)
        tg = torch.tensor(np.where(live, c["targets"][:, :T].T, 0).astype(np.int64))
        per = F.cross_entropy(x.reshape(-1, c["C"]), tg.reshape(-1), reduction="none").reshape(T, -1)
        per = per * torch.tensor(live.astype(np.float64))
        (scale * per.sum()).backward()
        assert np.allclose(nll, per.detach().numpy(), rtol=1e-12, atol=1e-12), (c["C"], c["kind"])
        assert np.allclose(g, x.grad.numpy(), rtol=1e-12, atol=1e-15), (c["C"], c["kind"])
        assert np.all(nll[~live] == 0) and np.all(g[~live] == 0)
        assert not live[2, 0] and not live[3, 0] and live[4, 0] and live[0, 1] and not live[1, 1] and not live[:, 2].any()


def test_embed_reference_agrees_with_torch_float64():
    for c in R.embed_cases():
        T, V, H = c["T"], c["V"], c["H"]
        ids = c["tok"][:, :T].T
        live = R.live_positions(c["lengths"], T)
        hit = live & (ids >= 0) & (ids < V)
        w = torch.tensor(c["w"].astype(np.float64), requires_grad=True)
        bias = torch.tensor(c["bias"].astype(np.float64), requires_grad=True)
        emb = F.embedding(torch.tensor(np.where(hit, ids, 0).astype(np.int64)), w) * torch.tensor(hit.astype(np.float64))[..., None]
        out = emb + bias
        assert np.array_equal(R.embed_fwd_ref(c["tok"], c["lengths"], T, c["w"], c["bias"]), out.detach().numpy())
        assert np.array_equal(R.embed_fwd_ref(c["tok"], c["lengths"], T, c["w"], None), emb.detach().numpy())
        # the backward sums: dbias over every position inside its row, dw over those with an id inside the alphabet
        dz = torch.tensor(c["dz"].astype(np.float64))
        ((emb + bias * torch.tensor(live.astype(np.float64))[..., None]) * dz).sum().backward()
        dw, db, aw, ab, n_dw, n_db = R.embed_bwd_ref(c["tok"], c["lengths"], T, c["dz"], V)
        assert np.allclose(dw, w.grad.numpy(), rtol=1e-13, atol=1e-13) and np.allclose(db, bias.grad.numpy(), rtol=1e-13, atol=1e-13)
        assert n_db == int(live.sum()) and n_dw.sum() == int(hit.sum())
        if c["skew"]:
            assert (n_dw > 0).sum() == 1 and n_dw.max() == T * c["B"]
        elif V > 1:
            assert np.all(n_dw[V // 2:] == 0) and n_dw.sum() < n_db      # ids that never occur; ids out of range


def test_float32_evaluation_stays_inside_the_bounds_on_every_case(xent_cases):
    for c in xent_cases:
        for scale in (1.0, float(np.float32(1.0 / 7.0))):
            nll, g, live = R.xent_ref(c["logits"], c["targets"], c["lengths"], scale)
            nll32, g32 = R.xent_f32(c["logits"], c["targets"], c["lengths"], scale)
            M = _row_max(c["logits"])
            assert np.all(np.abs(nll32 - nll) <= R.nll_bound(c["C"], M)), (c["C"], c["kind"])
            assert np.all(np.abs(g32 - g) <= R.dlogits_bound(c["C"], M, scale)[..., None]), (c["C"], c["kind"])
            assert np.all(np.abs(g32.astype(np.float64).sum(axis=2)) <= R.dlogits_rowsum_bound(c["C"], M, scale))
            assert np.all(nll32[~live] == 0) and np.all(g32[~live] == 0)
    for c in R.embed_cases():      # the n-term bound with a sequential float32 sum in position order
        T, V = c["T"], c["V"]
        dw, db, aw, ab, n_dw, n_db = R.embed_bwd_ref(c["tok"], c["lengths"], T, c["dz"], V)
        ids, live = c["tok"][:, :T].T, R.live_positions(c["lengths"], T)
        got = np.zeros((V, c["H"]), np.float32)
        for t in range(T):
            for b in range(c["B"]):
                if live[t, b] and 0 <= ids[t, b] < V:
                    got[ids[t, b]] += c["dz"][t, b]
        assert np.all(np.abs(got - dw) <= R.sum_bound(n_dw + 1, aw.T).T)


def test_wrong_variants_fall_outside_the_bounds(xent_cases):
    seen = {"no_max": 0, "c_minus_1": 0}
    for c in xent_cases:
        nll, g, live = R.xent_ref(c["logits"], c["targets"], c["lengths"], 1.0)
        M = _row_max(c["logits"])
        if c["kind"] == "pm80":          # no maximum subtracted: the target at -80 beside a +80 has probability 0 in float32
            nll32, _ = R.xent_f32(c["logits"], c["targets"], c["lengths"], 1.0, "no_max")
            assert not np.abs(nll32[0, 0] - nll[0, 0]) <= R.nll_bound(c["C"], M[0, 0]), c["C"]
            seen["no_max"] += 1
        # one class left out of the softmax: every live row is off by about that class's probability, ~1 / C.  The bound grows as
        # C u (a C-term sum in any order), so the two meet near C = u**-0.5 = 4096: the variant is told apart where 1 / C >> C u.
        if c["kind"] == "normal" and c["C"] <= 300:
            nll32, g32 = R.xent_f32(c["logits"], c["targets"], c["lengths"], 1.0, "c_minus_1")
            bad_g = np.abs(g32 - g).max(axis=2) > R.dlogits_bound(c["C"], M, 1.0)
            bad_nll = np.abs(nll32 - nll) > R.nll_bound(c["C"], M)
            assert np.all(bad_g[live]) and np.all(bad_nll[live]), c["C"]
            seen["c_minus_1"] += 1
    assert min(seen.values()) >= len(R.XENT_C_FIXED)


def test_loss_rule_is_the_float64_sum_rounded_once():
    rng = np.random.RandomState(3)
    nll = (rng.rand(161, 4) * 9).astype(np.float32)
    want = np.array([np.float32(sum(float(v) for v in nll[:, b])) for b in range(4)])      # python floats are float64
    assert np.array_equal(R.loss_rule(nll), want)


# ------------------------------------------------------------------------------------------------------- the LM oracle
def test_lm_oracle_gradients_match_central_differences():
    L, H, V, T = 1, 16, 5, 4
    p = {k: v.astype(np.float64) for k, v in om.init_params(L, H, V, V, seed=5).items()}
    rng = np.random.RandomState(1)
    for k in p:
        if k.endswith("_b") or k.startswith("bias"):
            p[k] = 0.1 * rng.randn(*p[k].shape)
    tok = np.array([[4, 0, 1, 2, 4], [4, 3, 3, 4, 0]], np.int32)      # [C-1, y.., C-1]; row 1 has 2 tokens + EOS
    lengths = np.array([4, 3], np.int32)
    loss, _, grads = R.lm_oracle_loss_and_grads(p, tok, lengths, L)
    assert loss.shape == (2,) and np.all(loss > 0)
    eps = 1e-6
    for name in om.param_names(L):
        flat = p[name].reshape(-1)
        for i in rng.choice(flat.size, size=min(flat.size, 6), replace=False):
            keep = flat[i]
            flat[i] = keep + eps
            up = R.lm_oracle_loss_and_grads(p, tok, lengths, L)[0].sum()
            flat[i] = keep - eps
            dn = R.lm_oracle_loss_and_grads(p, tok, lengths, L)[0].sum()
            flat[i] = keep
            fd = (up - dn) / (2 * eps)
            assert abs(fd - grads[name].reshape(-1)[i]) <= 1e-6 * max(1.0, abs(fd)), (name, i, fd, grads[name].reshape(-1)[i])
