"""csrc/lm_step.hip on the GPU: one language-model step for N gathered hypotheses against the float64 step of lm_fusion_ref within
the derived bounds, on every instantiation and boundary the plan query reports; untouched slots, bit-for-bit row independence,
refused shapes, and a sentence stepped token by token against LmEngine.score."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERN = np.int32(0x7FC0BEEF)          # a quiet NaN with a recognisable payload: slots that must not be read or written


def _device_params(p, L, H, V):
    from rnn_speech_amd.engine import ParamLayout
    lay = ParamLayout(L, H, V, V)
    flat = torch.zeros(lay.total, device="cuda")
    for k, a in p.items():
        lay.view(flat, k).copy_(torch.as_tensor(a))
    return lay, flat


def _run(case, parent=None, token=None, dest=None, pool_h=None, pool_c=None):
    """One ops.lm_step on the case's pool and parameters -> (pool_h, pool_c, logq) as numpy."""
    from rnn_speech_amd import ops
    L, H, V = case["L"], case["H"], case["V"]
    lay, flat = _device_params(case["params"], L, H, V)
    parent = case["parent"] if parent is None else parent
    token = case["token"] if token is None else token
    dest = case["dest"] if dest is None else dest
    dh = torch.as_tensor(case["pool_h"] if pool_h is None else pool_h).cuda()
    dc = torch.as_tensor(case["pool_c"] if pool_c is None else pool_c).cuda()
    v = lambda n: lay.view(flat, n)      # noqa: E731
    logq = ops.lm_step(torch.as_tensor(parent).cuda(), torch.as_tensor(token).cuda(), torch.as_tensor(dest).cuda(), dh, dc,
                       v("input_w"), v("input_b"), v("kernel_0"), lay.kernel_stride, v("bias_0"), lay.bias_stride, v("output_w"),
                       v("output_b"))
    torch.cuda.synchronize()
    return dh.cpu().numpy(), dc.cpu().numpy(), logq.cpu().numpy()


@pytest.fixture(scope="module")
def cases():
    from rnn_speech_amd import ops
    out = F.step_cases(ops.lm_step_plan)
    for c in out:      # the reference and its bounds once, shared and left unchanged
        c["ref"] = F.lm_step_ref(c["params"], c["L"], c["h_par"], c["c_par"], c["token"])
        c["bounds"] = F.lm_step_bounds(c["params"], c["L"], c["h_par"], c["c_par"], c["token"])
    return out


def test_the_table_covers_every_instantiation_of_the_plan(cases):
    from rnn_speech_amd import ops
    seen = {(c["L"], c["H"], c["V"]) for c in cases}
    assert {h for _, h, _ in seen} == {16, 48, 256} and {l for l, _, _ in seen} == {1, 3} and {v for _, _, v in seen} == {2, 80, 129}
    ns = {c["N"] for c in cases}
    assert {1, 15, 16, 17, 65} <= ns
    tiles = {ops.lm_step_plan(n, 1, 16, 2)["row_tile"] for n in ns}
    assert tiles == {ops.lm_step_plan(n, 1, 16, 2)["row_tile"] for n in (1, 100, 1000, 100000)} and all(t + 1 in ns for t in tiles)


def test_every_case_meets_the_derived_bounds_and_leaves_other_slots_alone(cases):
    for c in cases:
        used = np.zeros(c["n_slots"], bool)
        used[c["parent"][c["parent"] >= 0]] = True
        pool_h, pool_c = c["pool_h"].copy(), c["pool_c"].copy()
        pool_h.view(np.int32)[~used] = PATTERN            # every slot that is not a parent: the dest slots and the bystanders
        pool_c.view(np.int32)[~used] = PATTERN
        h, cc, logq = _run(c, pool_h=pool_h, pool_c=pool_c)
        tag = (c["L"], c["H"], c["V"], c["N"])
        for got, ref, bound, name in ((h[c["dest"]], c["ref"][0], c["bounds"][0], "h"), (cc[c["dest"]], c["ref"][1], c["bounds"][1], "c"),
                                      (logq, c["ref"][2], c["bounds"][2], "logq")):
            ratio = np.abs(got.astype(np.float64) - ref) / bound
            assert np.isfinite(got).all() and float(ratio.max()) <= 1.0, (tag, name, float(ratio.max()))
        other = np.ones(c["n_slots"], bool)
        other[c["dest"]] = False
        assert h.view(np.int32)[other].tobytes() == pool_h.view(np.int32)[other].tobytes(), tag
        assert cc.view(np.int32)[other].tobytes() == pool_c.view(np.int32)[other].tobytes(), tag


@pytest.mark.parametrize("shape", [(3, 48, 80), (1, 256, 129)])
def test_a_row_gets_the_same_bits_at_any_position_and_any_row_count(cases, shape):
    from rnn_speech_amd import ops
    by_n = {c["N"]: c for c in cases if (c["L"], c["H"], c["V"]) == shape}
    big = by_n[max(by_n)]
    all_tiles = {ops.lm_step_plan(n, *shape)["row_tile"] for n in by_n}
    big_tile = ops.lm_step_plan(big["N"], *shape)["row_tile"]
    assert big_tile == max(all_tiles) and len(all_tiles) >= 2
    h, cc, logq = _run(big)
    h2, cc2, logq2 = _run(big)
    assert h.tobytes() == h2.tobytes() and cc.tobytes() == cc2.tobytes() and logq.tobytes() == logq2.tobytes()      # two runs
    free = np.setdiff1d(np.arange(big["n_slots"]), np.concatenate([big["dest"], big["parent"]]))
    tiles = set()
    for rows in ([big["N"] - 1, 30, 7], list(range(3, 3 + 50))[::-1], [0], list(range(big["N"] - 17, big["N"]))):
        rows = np.array(rows)
        dest = np.concatenate([free, big["dest"]])[:len(rows)].astype(np.int32)      # other slots than in the big call
        keep = ~np.isin(dest, big["parent"][rows])
        assert keep.all()
        tiles.add(ops.lm_step_plan(len(rows), *shape)["row_tile"])
        hs, cs, qs = _run(big, parent=big["parent"][rows], token=big["token"][rows], dest=dest)
        assert hs[dest].tobytes() == h[big["dest"][rows]].tobytes()
        assert cs[dest].tobytes() == cc[big["dest"][rows]].tobytes()
        assert qs.tobytes() == logq[rows].tobytes()
    assert tiles | {big_tile} == all_tiles and big_tile not in tiles      # every instantiation gave the rows the same bits


def test_refused_shapes_return_their_status_without_a_launch():
    from rnn_speech_amd import lib, ops
    for L, H, V, word in ((1, 24, 6, "multiple of 16"), (1, 16, 257, "limit of 256"), (9, 16, 6, "1 .. 8")):
        n_slots = 4
        dh = torch.full((n_slots, L, H), 3.0, device="cuda")
        dc = torch.full((n_slots, L, H), 5.0, device="cuda")
        z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
        idx = torch.tensor([0], dtype=torch.int32, device="cuda")
        logq = torch.full((1, V), 7.0, device="cuda")
        with pytest.raises(lib.AmdSpeechError, match=word):
            ops.lm_step(idx - 1, idx, idx + 1, dh, dc, z(V, H), z(H), z(2 * H, 4 * H), 2 * H * 4 * H, z(4 * H), 4 * H, z(H, V), z(V), logq=logq)
        torch.cuda.synchronize()
        assert bool((dh == 3.0).all()) and bool((dc == 5.0).all()) and bool((logq == 7.0).all())


def test_a_sentence_stepped_token_by_token_reproduces_the_engine_score():
    from rnn_speech_amd.language_model import LmEngine, LmStepper, sentence_rows
    L, H, V, B, T = 2, 128, 80, 3, 12
    eng = LmEngine(L, H, V, B, T, seed=7)
    rng = np.random.RandomState(1)
    p = eng.to_numpy()
    for k in p:
        if p[k].ndim == 1:
            p[k] = (rng.randn(*p[k].shape) * 0.1).astype(np.float32)
    eng.load_numpy(p)
    tok, lens = sentence_rows([list(rng.randint(0, V - 1, size=n - 1)) for n in (12, 7, 1)], V, width=T)
    logp, per_token = eng.score(torch.as_tensor(tok).cuda(), torch.as_tensor(lens).cuda(), max_len=int(lens.max()), per_token=True)
    stepper = LmStepper(eng, 2 * B)
    got = np.zeros((T, B))
    for t in range(T):                                        # the three rows together, each row's state in its own pair of slots
        parent = np.array([-1 if t == 0 else 2 * b + (t - 1) % 2 for b in range(B)], np.int32)
        dest = np.array([2 * b + t % 2 for b in range(B)], np.int32)
        logq = stepper(parent, tok[:, t], dest)
        for b in range(B):
            if t < lens[b]:
                got[t, b] = logq[b, tok[b, t + 1]]
    np.testing.assert_allclose(got, per_token[:T], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(got.sum(axis=0), logp, rtol=1e-3, atol=1e-5)
    assert stepper.calls == T and stepper.rows == T * B
    with pytest.raises(ValueError, match="also a parent"):
        stepper(np.array([0, 1], np.int32), tok[:2, 0], np.array([1, 2], np.int32))
