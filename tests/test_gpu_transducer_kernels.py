"""csrc/transducer.hip on the GPU, stage by stage through the C ABI into poisoned outputs, on every case of transducer_ref's table:
the joint's logits, the lattice loss and dlogits, and the joint's backward against the float64 references within the bounds of
transducer_ref (none of which comes from a GPU); exact zeros where no live node is, rows of dlogits that sum to zero, the same bits
from two calls, from any place in the batch and from dlogits aliasing logits; the label kernel; amdspeech_lm_step_state against
amdspeech_lm_step; and greedy decoding against the reference decoder."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402
import transducer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)


def _plan(*a):
    from rnn_speech_amd import ops
    return ops.rnnt_plan(*a)


CASE_NAMES = [c["name"] for c in R.cases(_plan)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _pipeline(f, g, w, bias, lengths, targets, n, logits_in, dl_in, dw0, db0, alias=False):
    """The three stages on the given inputs -> numpy results.  logits_in / dl_in are what the loss and the backward are fed (the
    reference's roundings, dead nodes NaN); every output starts as NaN."""
    from rnn_speech_amd import ops
    T, B, J = f.shape
    U, C = g.shape[0] - 1, w.shape[1]
    df_, dg_, dw_, db_ = _dev(f), _dev(g), _dev(w), _dev(bias)
    dlen, dn, dt = _dev(lengths), _dev(n), _dev(targets)
    out = {}
    logits = torch.full((B, T, U + 1, C), float("nan"), device="cuda")
    ops.rnnt_joint_fwd(df_, dg_, dw_, db_, dlen, dn, logits=logits)
    out["logits"] = logits.cpu().numpy()
    x = _dev(logits_in)
    loss = torch.full((B,), float("nan"), device="cuda")
    d = x if alias else torch.full_like(x, float("nan"))
    ops.rnnt_loss_fwd_bwd(x, dt, dn, dlen, loss=loss, dlogits=d)
    out["loss"], out["d"] = loss.cpu().numpy(), d.cpu().numpy()
    gdw, gdb = _dev(dw0), _dev(db0)
    gdf = torch.full_like(df_, float("nan"))
    gdg = torch.full_like(dg_, float("nan"))
    ops.rnnt_joint_bwd(_dev(dl_in), df_, dg_, dw_, dlen, dn, gdw, gdb, df=gdf, dg=gdg)
    torch.cuda.synchronize()
    out.update(df=gdf.cpu().numpy(), dg=gdg.cpu().numpy(), dw=gdw.cpu().numpy(), db=gdb.cpu().numpy())
    return out


def _inputs(ev, rows=None):
    """The pipeline's arguments for a case, or for the given rows of it (in that order)."""
    rows = list(range(ev["case"]["B"])) if rows is None else rows
    live = ev["live"][rows][..., None]
    rng = np.random.RandomState(5)
    dw0 = rng.randn(*ev["w"].shape).astype(np.float32)
    db0 = rng.randn(ev["w"].shape[1]).astype(np.float32)
    return (ev["f"][:, rows], ev["g"][:, rows], ev["w"], ev["bias"], ev["lengths"][rows], ev["targets"][rows], ev["n"][rows],
            np.where(live, ev["logits32"][rows], NAN), np.where(live, ev["d32"][rows], NAN), dw0, db0)


@functools.lru_cache(maxsize=None)
def _run(name):
    ev = R.evaluated(name, _plan)
    args = _inputs(ev)
    return ev, args, _pipeline(*args)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_stage_is_within_its_bound_and_exact_zeros_stand_where_no_live_node_is(name):
    ev, args, got = _run(name)
    live = ev["live"]
    # the joint
    err = np.abs(got["logits"].astype(np.float64) - ev["logits_ref"])
    print(name, "logits: worst error / bound %.2f" % float((err / ev["logits_bound"])[live].max() if live.any() else 0))
    assert (err <= ev["logits_bound"])[live].all()
    # the loss and dlogits
    errs = R.slice_errors(got["loss"], got["d"], ev["loss_ref"], ev["d_ref"], ev["lengths"])
    print(name, "loss / dlogits: worst error / bound %.2f" % max(e / ev["bounds"][k] for k, e in errs.items()))
    assert not R.judge(ev, got["loss"], got["d"])
    assert not got["d"][~live].any() and not np.isnan(got["d"]).any()
    Tb = np.clip(ev["lengths"], 0, ev["case"]["T"])
    assert (got["loss"][Tb == 0] == 0).all()
    rs = R.rowsum_worst(got["d"], live)
    print(name, "row sum %.2e, bound %.2e" % (rs, ev["rowsum_bound"]))
    assert rs <= ev["rowsum_bound"]
    # the joint's backward: df / dg overwritten, dw / db accumulated onto what was there
    dw0, db0 = args[-2], args[-1]
    df, dg, dw, db = ev["bwd_ref"]
    b_df, b_dg, b_dw, b_db = ev["bwd_bounds"]
    u = 2.0 ** -24
    for what, g, r, bound in (("df", got["df"], df, b_df), ("dg", got["dg"], dg, b_dg),
                              ("dw", got["dw"], dw + dw0, b_dw + u * np.abs(dw + dw0)), ("db", got["db"], db + db0, b_db + u * np.abs(db + db0))):
        e = np.abs(g.astype(np.float64) - r)
        print(name, what, "worst error / bound %.3f" % float((e / np.maximum(bound, 1e-300)).max()))
        assert (e <= bound).all(), what
    assert not got["df"][~live.any(axis=2).T].any() and not got["dg"][~live.any(axis=1).T].any()


@pytest.mark.parametrize("name", ("t-tile", "t-chunk", "large", "rec-256"))
def test_two_calls_give_the_same_bits_and_dlogits_may_be_logits(name):
    ev, args, got = _run(name)
    again = _pipeline(*args, alias=True)
    live = ev["live"]
    for k in got:
        a, b = got[k], again[k]
        if k == "logits":
            a, b = np.where(live[..., None], a, 0), np.where(live[..., None], b, 0)
        assert a.tobytes() == b.tobytes(), k


def test_a_row_s_results_do_not_depend_on_its_place_in_the_batch_or_on_b():
    ev, args, got = _run("t-tile")
    B = ev["case"]["B"]
    for rows in ([2, 0, 1], [1], [2]):
        sub = _pipeline(*_inputs(ev, rows))
        for i, b in enumerate(rows):
            live = ev["live"][b][..., None]
            assert np.where(live, sub["logits"][i], 0).tobytes() == np.where(live, got["logits"][b], 0).tobytes()
            assert sub["loss"][i].tobytes() == got["loss"][b].tobytes() and sub["d"][i].tobytes() == got["d"][b].tobytes()
            assert sub["df"][:, i].tobytes() == got["df"][:, b].tobytes() and sub["dg"][:, i].tobytes() == got["dg"][:, b].tobytes()
    assert B == 3


def test_the_table_reaches_every_instantiation_the_plan_names():
    from rnn_speech_amd import lib
    recs, tiles = set(), {}
    for c in R.cases(_plan):
        p = _plan(c["T"], c["B"], c["U"], c["J"], c["C"])
        recs.add(p["rec_kernel"])
        # per instantiation of the joint kernels: (second forward prefix tile, second backward prefix step, live node in either)
        n_max = max(r["n"] for r in c["rows"] if r["length"] > 0) if any(r["length"] > 0 for r in c["rows"]) else -1
        tiles.setdefault(p["col_tiles"], set()).update({("fwd_u2", n_max >= p["fwd_u_tile"]), ("bwd_u2", n_max >= p["bwd_u_tile"]),
                                                         ("fwd_u1_only", 0 <= n_max < p["fwd_u_tile"] < c["U"] + 1)})
    assert sorted(tiles) == [2, 5, 8, 16] and recs == set(lib.RNNT_REC_KERNELS)
    for nt, seen in tiles.items():
        assert {("fwd_u2", True), ("bwd_u2", True), ("fwd_u1_only", True)} <= seen, (nt, seen)
    spans = set()
    for c in R.cases(_plan):
        p = _plan(c["T"], c["B"], c["U"], c["J"], c["C"])
        spans.add((p["fwd_t_tiles"] > 1, p["bwd_t_chunks"] > 1, p["bwd_k_slices"] > 1))
    assert {t[0] for t in spans} == {t[1] for t in spans} == {t[2] for t in spans} == {False, True}


def test_the_label_kernel_equals_the_reference_on_short_and_on_multi_chunk_rows():
    from rnn_speech_amd import ops
    rng = np.random.RandomState(2)
    C, U = 80, 150
    dense = np.zeros((6, U), np.int32)
    dense[0, :5] = [5, 0, 5, 79, 7]
    dense[1, :2] = [0, 79]
    dense[2, :5] = [7, -2, 8, -1, 79]                             # negative ids are dropped with the zeros
    dense[3] = rng.randint(0, C - 1, size=U)                      # no EOS at all: every non-zero label is a target
    dense[4] = rng.randint(0, 3, size=U); dense[4, 100] = 79      # many zeros, the EOS in the second chunk of 64
    dense[5] = rng.randint(1, C - 1, size=U); dense[5, 63] = 80; dense[5, 70] = 79
    got = [t.cpu().numpy() for t in ops.rnnt_targets(_dev(dense), C)]
    for g, w in zip(got, R.targets_ref(dense, C)):
        assert g.dtype == np.int32 and g.tobytes() == w.tobytes()


@pytest.mark.parametrize("L,H,V", F.STEP_SHAPES)
def test_lm_step_state_leaves_the_same_pool_bits_as_lm_step(L, H, V):
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import ParamLayout
    for N in (1, 17, 65):
        case = F.step_case(L, H, V, N)
        lay = ParamLayout(L, H, V, V)
        flat = torch.zeros(lay.total, device="cuda")
        for k, a in case["params"].items():
            lay.view(flat, k).copy_(torch.as_tensor(a))
        v = lambda n: lay.view(flat, n)      # noqa: E731
        idx = [_dev(case[k]) for k in ("parent", "token", "dest")]
        h1, c1, h2, c2 = (_dev(case[k]) for k in ("pool_h", "pool_c", "pool_h", "pool_c"))
        ops.lm_step(*idx, h1, c1, v("input_w"), v("input_b"), v("kernel_0"), lay.kernel_stride, v("bias_0"), lay.bias_stride,
                    v("output_w"), v("output_b"))
        ops.lm_step_state(*idx, h2, c2, v("input_w"), v("input_b"), v("kernel_0"), lay.kernel_stride, v("bias_0"), lay.bias_stride, V)
        torch.cuda.synchronize()
        assert h1.cpu().numpy().tobytes() == h2.cpu().numpy().tobytes() and c1.cpu().numpy().tobytes() == c2.cpu().numpy().tobytes()
        assert h2.cpu().numpy().tobytes() != case["pool_h"].tobytes()


@pytest.mark.parametrize("name", [c[0] for c in R.GREEDY_CASES])
def test_greedy_decoding_on_the_device_equals_the_reference_decoder(name):
    from rnn_speech_amd import ops
    from rnn_speech_amd.engine import ParamLayout
    c = R.greedy_case(name)
    L, H, C, B, U, T = c["L"], c["H"], c["C"], c["B"], c["U"], c["T"]
    want_ids, want_len, _, _ = R.greedy_walk(c["p"], L, c["f"], c["lengths"], U, c["w"], c["bias"], F.lm_step_ref)
    lay = ParamLayout(L, H, C, C)
    flat = torch.zeros(lay.total, device="cuda")
    for k, a in c["p"].items():
        if not k.startswith("pred_"):
            lay.view(flat, k).copy_(torch.as_tensor(a))
    v = lambda n: lay.view(flat, n)      # noqa: E731
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32)).cuda()      # noqa: E731
    pool_h = torch.zeros(2 * B, L, H, device="cuda")
    pool_c = torch.zeros(2 * B, L, H, device="cuda")
    parent, token, dest = i32([-1] * B), i32([C - 1] * B), i32([2 * b for b in range(B)])
    t_idx, m, slot = i32([0] * B), i32([0] * B), i32([2 * b for b in range(B)])
    ids = i32(np.zeros((B, U)))
    f, w, bias = (_dev(c[k]) for k in ("f", "w", "bias"))
    pw, pb, lengths = _dev(c["p"]["pred_w"]), _dev(c["p"]["pred_b"]), _dev(c["lengths"])
    step = lambda: ops.lm_step_state(parent, token, dest, pool_h, pool_c, v("input_w"), v("input_b"), v("kernel_0"), lay.kernel_stride,      # noqa: E731
                                     v("bias_0"), lay.bias_stride, C)
    step()                                                        # the start symbol from the zero state into every row's first slot
    for _ in range(T + U):                                        # nothing is read in between
        ops.rnnt_greedy_step(f, lengths, U, pool_h, pw, pb, w, bias, t_idx, m, slot, ids, parent, token, dest)
        step()
    torch.cuda.synchronize()
    got_len, got_ids = m.cpu().numpy(), ids.cpu().numpy()
    assert list(got_len) == list(want_len)
    for b in range(B):
        assert list(got_ids[b, :got_len[b]]) == list(want_ids[b, :want_len[b]])
    Tb = np.clip(c["lengths"], 0, T)
    assert all(t_idx.cpu().numpy()[b] == Tb[b] or got_len[b] == U for b in range(B))      # every row finished
