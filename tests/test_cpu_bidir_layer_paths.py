"""tests/bidir_layer_ref.py's per-call reference tied down without a GPU: against torch.nn.LSTM(bidirectional=True) with an initial
state, its hand-written backward pass against autograd of bidir_layer_ref.forward, the slice metric against the whole-tensor metric
it replaces, and the conditions the GPU matrix (tests/test_gpu_bidir_layer_paths.py) puts on its cases and its recorded table.  At
the end: the library's exported plan (amdspeech_lstm_bidir_plan, host only) against bidir_layer_ref.expected_plan."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bidir_layer_ref as R  # noqa: E402


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _small(T, B, H, L, seed, state=True, lengths=None):
    g = torch.Generator().manual_seed(seed)
    ks, bs = [], []
    for k in range(2):
        for l in range(L):
            ks.append(torch.randn((2 if l == 0 else 3) * H, 4 * H, generator=g, dtype=torch.float64) * (0.8 / np.sqrt(H)))
            bs.append(torch.randn(4 * H, generator=g, dtype=torch.float64) * 0.3)
    z0 = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    dy = [torch.randn(T, B, H, generator=g, dtype=torch.float64) for _ in range(2)]
    h0 = torch.randn(L, B, H, generator=g, dtype=torch.float64) * 0.5 if state else None
    c0 = torch.randn(L, B, H, generator=g, dtype=torch.float64) * 0.5 if state else None
    if lengths is None:
        lengths = np.array(([T, T - 1, 1, 0] + list(np.random.RandomState(seed).randint(1, T + 1, size=B)))[:B], np.int32)
    return ks, bs, z0, dy, h0, c0, lengths


def _masks(T, B, H, L, seed):
    g = torch.Generator().manual_seed(seed)
    return {(d, w, l): (torch.rand(T, B, H if (w == "out" or l == 0) else 2 * H, generator=g) < 0.7).double() / 0.7
            for d in R.DIRS for w in ("in", "out") for l in range(L)}


# ------------------------------------------------------------------------------------------------ against torch.nn.LSTM
@pytest.mark.parametrize("T,B,H,L,state", [(7, 6, 16, 3, True), (9, 5, 8, 2, False), (1, 4, 16, 2, True)])
def test_reference_is_nn_lstm_bidirectional_with_an_initial_state(T, B, H, L, state):
    ks, bs, z0, _, h0, c0, lengths = _small(T, B, H, L, seed=T + B, state=state)
    f = R.call_forward(z0, ks, bs, lengths, h0, c0)
    y, hT, cT = R.torch_lstm_states(ks, bs, z0, lengths, h0, c0)
    assert _rel(torch.cat([f["y"][L - 1, 0], f["y"][L - 1, 1]], dim=2), y) < 1e-12
    assert _rel(f["hT"], hT) < 1e-12 and _rel(f["cT"], cT) < 1e-12          # every layer's forward cell
    assert R.padding_is_zero(f["y"], lengths)
    dead = np.nonzero(lengths == 0)[0]
    if state and len(dead):      # rows without a frame: the state passes through untouched
        assert torch.equal(f["hT"][:, dead], h0[:, dead]) and torch.equal(f["cT"][:, dead], c0[:, dead])


def test_generalised_nn_lstm_helper_agrees_with_the_old_one_without_a_state():
    T, B, H, L = 6, 4, 8, 2
    ks, bs, z0, _, _, _, lengths = _small(T, B, H, L, seed=2, state=False)
    p = {"input_w": np.eye(H), "input_b": np.zeros(H), "output_w": np.eye(2 * H), "output_b": np.zeros(2 * H)}
    for k, pre in enumerate(("", "bw_")):
        for l in range(L):
            p[pre + "kernel_%d" % l], p[pre + "bias_%d" % l] = ks[k * L + l].numpy(), bs[k * L + l].numpy()
    y, _, _ = R.torch_lstm_states(ks, bs, z0, lengths)
    np.testing.assert_allclose(y.numpy(), R.torch_lstm_forward(p, z0.numpy(), lengths, L, H), rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------ against autograd of forward()
@pytest.mark.parametrize("T,B,H,L,masks,state", [(7, 6, 16, 3, True, True), (5, 4, 8, 2, False, True), (6, 5, 8, 2, True, False),
                                                 (1, 3, 8, 2, False, True)])
def test_hand_written_backward_is_autograd_of_the_model_reference(T, B, H, L, masks, state):
    """bidir_layer_ref.forward with identity Linear layers around the stack IS the call; its autograd gradients are the hand-written
    ones to <= 1e-10 of each tensor's maximum, with masks and with h0 / c0."""
    ks, bs, z0, dy, h0, c0, lengths = _small(T, B, H, L, seed=10 * T + L, state=state)
    m = _masks(T, B, H, L, seed=T) if masks else None
    f = R.call_forward(z0, ks, bs, lengths, h0, c0, m)
    r = R.call_backward(f["cache"], dy[0], dy[1])
    p = {"input_w": torch.eye(H, dtype=torch.float64), "input_b": torch.zeros(H, dtype=torch.float64),
         "output_w": torch.eye(2 * H, dtype=torch.float64), "output_b": torch.zeros(2 * H, dtype=torch.float64)}
    for k, pre in enumerate(("", "bw_")):
        for l in range(L):
            p[pre + "kernel_%d" % l] = ks[k * L + l].clone().requires_grad_(True)
            p[pre + "bias_%d" % l] = bs[k * L + l].clone().requires_grad_(True)
    x = z0.clone().requires_grad_(True)
    logits, finals = R.forward(p, x, lengths, L, H, masks=m, h0=h0, c0=c0)
    assert _rel(torch.cat([f["y"][L - 1, 0], f["y"][L - 1, 1]], dim=2), logits) < 1e-12
    for l in range(L):
        assert _rel(f["hT"][l], finals[l][0]) < 1e-12 and _rel(f["cT"][l], finals[l][1]) < 1e-12
    (logits * torch.cat(dy, dim=2)).sum().backward()
    for k, pre in enumerate(("", "bw_")):
        for l in range(L):
            assert _rel(r["dK"][k * L + l], p[pre + "kernel_%d" % l].grad) <= 1e-10, (pre, l)
            assert _rel(r["db"][k * L + l], p[pre + "bias_%d" % l].grad) <= 1e-10, (pre, l)
    assert _rel(r["dz0"], x.grad) <= 1e-10
    assert R.padding_is_zero(r["dz0"], lengths)


def test_gradients_do_not_see_what_lies_past_the_lengths():
    T, B, H, L = 6, 5, 8, 2
    ks, bs, z0, dy, h0, c0, lengths = _small(T, B, H, L, seed=4)
    dead = torch.as_tensor(np.arange(T)[:, None] >= lengths[None, :])
    a = R.call_backward(R.call_forward(z0, ks, bs, lengths, h0, c0)["cache"], dy[0], dy[1])
    z1, d0, d1 = z0.clone(), dy[0].clone(), dy[1].clone()
    z1[dead], d0[dead], d1[dead] = 1e3, -1e3, 7e2
    fb = R.call_forward(z1, ks, bs, lengths, h0, c0)
    b = R.call_backward(fb["cache"], d0, d1)
    assert torch.equal(a["dz0"], b["dz0"]) and all(torch.equal(x, y) for x, y in zip(a["dK"] + a["db"], b["dK"] + b["db"]))


# ------------------------------------------------------------------------------------------------ the matrix
_REF = {}


def _case_ref(case):
    if case["name"] not in _REF:
        inp = R.make_inputs(case)
        masks = R.cpu_masks(case)
        _REF[case["name"]] = (inp, R.reference(case, inp, masks), masks)
    return _REF[case["name"]]


def test_every_variant_has_a_case_and_no_case_an_unknown_variant():
    covered = {v for c in R.CASES for v in c["covers"]}
    assert covered == set(R.VARIANTS), covered ^ set(R.VARIANTS)
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        assert 1 <= c["T"] <= 12 and c["L"] <= 3 and c["precision"] in (0, 1)
        if c["H"] >= 512 or c["B"] >= 64:
            assert c["T"] <= 6 and c["L"] <= 2, c["name"]
        assert c["path"] == R.expected_path(c), c["name"]
        for kind in R.KINDS:      # every (precision, regime) has its measured row, every kind a bound under its cap
            assert 0 < R.bound(c, kind) <= R.CAPS[c["precision"]][0 if kind in R.OUTPUT_KINDS else 1]


def test_matrix_holds_what_the_issue_lists():
    by = {c["name"]: c for c in R.CASES}
    p0, p1 = [c for c in R.CASES if c["precision"] == 0], [c for c in R.CASES if c["precision"] == 1]
    has = lambda cs, **kw: any(all(c[k] == v for k, v in kw.items()) for c in cs)
    assert has(p0, H=16, B=1) and has(p0, H=48, L=3, B=5) and has(p0, H=1008, B=3) and has(p0, H=1024, B=2, T=4) and has(p0, T=1)
    assert all(has(p0, H=128, B=b) for b in (64, 65, 130))
    assert has(p0, lens="short") and has(p0, lens="ones")
    lens = R.make_lengths(by["f32-h48-l3-b5"])
    assert {0, 1, by["f32-h48-l3-b5"]["T"]} <= set(lens.tolist())
    assert R.make_lengths(by["f32-short"]).max() < by["f32-short"]["T"] and (R.make_lengths(by["f32-ones"]) == 1).all()
    for cs in (p0, p1):
        assert any(c["state"] for c in cs) and any(c["regime"] == "saturating" for c in cs)
        for extra in ("dropout", "accumulate", "padding", "per_frame"):
            assert any(extra in c["extras"] for c in cs), extra
        assert any("dropout" in c["extras"] and c["L"] >= 2 for c in cs)
        assert any("per_frame" in c["extras"] and c["B"] % 16 for c in cs)
    assert all(has(p1, H=h) for h in (32, 96, 224, 768)) and (has(p1, H=160) or has(p1, H=320)) and has(p1, H=1024, T=4)
    mid = [c for c in p1 if c["H"] == 128]
    assert {1, 16, 17, 33, 65} <= {c["B"] for c in mid}
    assert has(p1, H=1024, B=65, L=1, path=1) and has(p1, H=1024, B=129, L=1, path=0)
    assert not any("per_frame" in c["extras"] for c in p1 if c["name"].endswith("path0"))      # (path 0 by the plan, not the flag)
    # every instantiated KPW of both bf16x3 kernels, and the wave counts 1, 3, 5, 6, 7 and 8
    shapes = [R.bf3_shape(c["H"]) for c in p1]
    assert {s[0][0] for s in shapes} == {1, 2, 4} and {s[1][0] for s in shapes} == {1, 2, 4, 8, 16}
    assert {1, 3, 5, 6, 7, 8} <= {s[0][1] for s in shapes} | {s[1][1] for s in shapes}
    claims = {"bf3:fwd-kpw1": (0, 0, 1), "bf3:fwd-kpw2": (0, 0, 2), "bf3:fwd-kpw4": (0, 0, 4), "bf3:bwd-kpw1": (1, 0, 1),
              "bf3:bwd-kpw2": (1, 0, 2), "bf3:bwd-kpw4": (1, 0, 4), "bf3:bwd-kpw8": (1, 0, 8), "bf3:bwd-kpw16": (1, 0, 16)}
    for c in p1:
        s = R.bf3_shape(c["H"])
        for v in c["covers"]:
            if v in claims:
                a, b, want = claims[v]
                assert s[a][b] == want, (c["name"], v, s)
            if v.startswith("bf3:waves"):
                assert int(v[len("bf3:waves"):]) in (s[0][1], s[1][1]), (c["name"], v, s)
    nmt = lambda c: (c["B"] + 15) // 16
    assert (nmt(by["bf3-h128-b33"]) + 1) // 2 == 2 and nmt(by["bf3-h128-b33"]) % 2 == 1          # backward: a second group of one tile
    assert (nmt(by["bf3-h128-b65"]) + 3) // 4 == 2 and (nmt(by["bf3-h128-b65"]) + 1) // 2 == 3


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_no_case_leaves_out_a_slice_that_is_not_structurally_zero(case):
    inp, ref, masks = _case_ref(case)
    info = R.info_of(case, inp["lengths"])
    for kind in R.KINDS:
        errs = R.slice_errors(ref[kind], ref[kind], kind, info)
        assert errs, kind
        assert max(e[1] for e in errs) == 0.0
        label, _, frac = min(errs, key=lambda e: e[2])
        assert frac >= R.FLOOR, "%s: slice %s has %.1e of its tensor's maximum" % (kind, label, frac)
        assert R.outside_slices(ref[kind], kind, info) == 0.0, "%s: something that is not exactly zero lies outside every slice" % kind
    # ... and what IS left out is what the module says: dead frames, and the cold cells of a batch without a second step
    cold = [k for k in range(2) if R.starts_from_zero_for_one_step(info, k)]
    assert cold == ([] if inp["lengths"].max() > 1 else ([1] if case["state"] else [0, 1]))
    n_cells, nu = 2 * case["L"], case["H"] // 16
    parts = 2 * (2 + 3 * (case["L"] - 1))
    assert len(R.slices("db", info)) == (4 * n_cells - len(cold) * case["L"]) * nu
    assert len(R.slices("dK", info)) == (4 * parts - len(cold) * (parts // 2 + 3 * case["L"])) * nu
    assert R.padding_is_zero(ref["y"], inp["lengths"]) and R.padding_is_zero(ref["dz0"], inp["lengths"])
    # what the case promises about its inputs
    valid = ~inp["dead"]
    assert all(bool((inp[n][valid].abs() >= 0.01).all()) and bool((inp[n][inp["dead"]] == 0).all()) for n in ("dytop_fw", "dytop_bw"))
    assert bool((inp["garbage"].abs() >= 1.0).all()) and bool(torch.isfinite(inp["garbage"]).all()) and float(inp["garbage"].abs().max()) <= 1e3
    if case["state"]:
        assert 0.4 < float(inp["h0"].std()) < 0.6 and 0.4 < float(inp["c0"].std()) < 0.6


@pytest.mark.parametrize("case", [c for c in R.CASES if c["regime"] == "saturating"],
                         ids=[c["name"] for c in R.CASES if c["regime"] == "saturating"])
def test_saturating_cases_run_the_gates_in_their_tails(case):
    inp = R.make_inputs(case)
    f = R.call_forward(inp["z0"], inp["ks"], inp["bs"], inp["lengths"], inp["h0"], inp["c0"])
    gates = R.gate_values(f["cache"])
    frac = float(((gates < 1e-2) | (gates > 1 - 1e-2)).double().mean())
    assert 0.1 <= frac <= 0.5, frac


def test_measured_table_is_the_emulated_arithmetic_of_this_matrix():
    """The table in bidir_layer_ref.py is a recorded run.  Its cheap cases are measured again here: within a factor 1.5 (float32 on
    another CPU sums in another order); the full table can only be larger than its cheap part."""
    now = R.measure([c for c in R.CASES if R.is_cheap(c)])
    assert set(now) == set(R.MEASURED_CHEAP) == set(R.MEASURED) == {R.family(c) for c in R.CASES}
    for key, row in now.items():
        for kind, e in row.items():
            assert R.MEASURED_CHEAP[key][kind] / 1.5 <= e <= 1.5 * R.MEASURED_CHEAP[key][kind], (key, kind, e, R.MEASURED_CHEAP[key][kind])
            assert R.MEASURED[key][kind] >= R.MEASURED_CHEAP[key][kind]
    # the docstring's table is the dict's
    doc = R.__doc__
    for (pr, regime), row in R.MEASURED.items():
        line = [ln for ln in doc.splitlines() if ln.startswith("%d  %-10s |" % (pr, regime))]
        assert len(line) == 1
        cells = [c.strip() for c in line[0].split("|")[1:]]
        for kind, cell in zip(R.KINDS, cells):
            cap = R.CAPS[pr][0 if kind in R.OUTPUT_KINDS else 1]
            capped = R.FACTOR * row[kind] > cap
            assert cell == "%.1e>%.1e%s" % (row[kind], min(cap, R.FACTOR * row[kind]), "c" if capped else ""), (pr, regime, kind, cell)


# ------------------------------------------------------------------------------------------------ the slice metric
def test_slicer_finds_a_planted_block_the_whole_tensor_metric_misses():
    """One forward workgroup's worth of damage -- 8 hidden units of ONE gate over ONE 16-row tile at one layer -- ten bounds large:
    in the outputs (the units of the tile over a third of its frames) and in a kernel gradient (16 rows of the h part).  The
    damaged block is the reported worst slice, while the whole tensor stays under today's whole-tensor tolerance."""
    case = next(c for c in R.CASES if c["name"] == "f32-padding")
    inp, ref, _ = _case_ref(case)
    info = R.info_of(case, inp["lengths"])
    H, L = case["H"], case["L"]
    # y: the smallest slice of layer 1 beside the tensor's largest entry ("anything small beside something large"), its upper 8 units
    lim = R.bound(case, "y")
    fracs = {lab: frac for lab, _, frac in R.slice_errors(ref["y"], ref["y"], "y", info)}
    label = min((s for s in R.slices("y", info) if s[0].startswith("layer 1 ")), key=lambda s: fracs[s[0]])
    assert 10 * lim * fracs[label[0]] < R.CAPS[0][0]
    l, k, frames, rows, units = label[3]
    valid = torch.as_tensor(label[4])[:, :, None]
    top = float((ref["y"][label[3]] * valid).abs().max())
    bad = ref["y"].clone()
    bad[l, k, frames, rows, units.start + 8:units.stop] += 10 * lim * top * valid
    err, worst_label = R.worst(R.slice_errors(bad, ref["y"], "y", info))
    assert worst_label == label[0] and err == pytest.approx(10 * lim, rel=1e-6), (err, worst_label)
    assert R.whole_errors(bad, ref["y"], "y") < R.CAPS[0][0]
    assert sum(e > lim for _, e, _ in R.slice_errors(bad, ref["y"], "y", info)) == 1
    # dK: the forward cell of layer 1, 16 of its h rows, gate j, units 8:16
    lim = R.bound(case, "dK")
    cell = 0 * L + 1
    blk = (slice(2 * H, 3 * H), slice(H, H + 16))
    bad = [t.clone() for t in ref["dK"]]
    bad[cell][2 * H + 16:2 * H + 32, H + 8:H + 16] += 10 * lim * float(ref["dK"][cell][blk].abs().max())
    errs = R.slice_errors(bad, ref["dK"], "dK", info)
    err, worst_label = R.worst(errs)
    assert worst_label == "layer 1 fw h rows gate j units 0:16" and err == pytest.approx(10 * lim, rel=1e-6), (err, worst_label)
    assert R.whole_errors(bad, ref["dK"], "dK") < R.CAPS[0][1]
    assert sum(e > lim for _, e, _ in errs) == 1
    # a sign error in the top H rows of a (3H, 4H) kernel gradient, scaled down as a small slice beside a large one would be
    bad = [t.clone() for t in ref["dK"]]
    ref2 = [t.clone() for t in ref["dK"]]
    for t in (bad[cell], ref2[cell]):
        t[:H] *= 1e-3
    bad[cell][:H] *= -1
    assert R.whole_errors(bad, ref2, "dK") < R.CAPS[0][1]
    err, worst_label = R.worst(R.slice_errors(bad, ref2, "dK", info))
    assert err == pytest.approx(2.0) and worst_label.startswith("layer 1 fw x-fw rows"), (err, worst_label)


def test_slices_tile_every_tensor_exactly_once():
    T, B, H, L = 7, 20, 48, 3
    lengths = np.array([7, 6, 1, 0] + [5] * 16, np.int32)
    info = dict(T=T, B=B, H=H, L=L, lengths=lengths, state=False)
    live = torch.as_tensor(np.arange(T)[:, None] < lengths[None, :], dtype=torch.float32)[:, :, None].expand(T, B, H)
    shapes = {"y": (L, 2, T, B, H), "dz0": (T, B, H), "hT": (L, B, H),
              "dK": [((2 if l == 0 else 3) * H, 4 * H) for _ in range(2) for l in range(L)], "db": [(4 * H,)] * (2 * L)}
    for kind, shape in shapes.items():
        lists = isinstance(shape, list)
        count = [torch.zeros(s) for s in shape] if lists else torch.zeros(shape)
        for _, key, _, idx, valid in R.slices(kind, info):
            c = count[key] if lists else count
            c[idx] += 1 if valid is None else torch.as_tensor(valid, dtype=torch.float32)[:, :, None]
        if kind in ("y", "dz0"):
            assert torch.equal(count, live.expand(shape)), kind
        else:
            assert all(bool((c == 1).all()) for c in (count if lists else [count])), kind
    # a block of rows without a frame: no frame slices; without a state no hT slices either, with one they are back
    info0 = dict(info, B=36, lengths=np.array([3] * 16 + [0] * 16 + [2] * 4, np.int32))
    assert not [s for s in R.slices("y", info0) if "rows 16:32" in s[0]] and not [s for s in R.slices("hT", info0) if "rows 16:32" in s[0]]
    assert [s for s in R.slices("hT", dict(info0, state=True)) if "rows 16:32" in s[0]]


# ------------------------------------------------------------------------------------------------ the exported plan
# amdspeech_lstm_bidir_plan runs on the host: everything but `path` and `cus` is the device's business on no device.  The cases of the
# matrix, and the two shapes of tools/bidir_layer_bench.py at both precisions.
_WORKLOAD = [dict(name="workload-T%d-B%d-H%d-L%d-p%d" % (s + (p,)), T=s[0], B=s[1], H=s[2], L=s[3], precision=p, extras=())
             for s in R.WORKLOAD_SHAPES for p in (0, 1)]
_PLAN_CASES = R.CASES + _WORKLOAD
EINVAL, EUNSUPPORTED = -1, -3      # include/amdspeech.h


def _lib():
    from rnn_speech_amd import lib as _l
    return _l, _l.load()


def _desc(case, flags=0, **over):
    c = dict(case, **over)
    return _lib()[0].LstmDesc(c["T"], c["B"], c["H"], c["L"], 1.0, 1.0, 0, c["precision"], flags)


def _plan(case, per_frame=False):
    from rnn_speech_amd import ops
    return ops.lstm_bidir_plan(types.SimpleNamespace(lib=_lib()[1], desc=_desc(case)), per_frame=per_frame)


def test_expected_plan_takes_over_expected_path():
    for c in R.CASES:
        assert R.expected_plan(c)["path"] == R.expected_path(c) == c["path"], c["name"]
        assert R.expected_plan(c, cus=0)["path"] == 0


def test_bidir_plan_struct_layout_and_wrapper():
    _l, handle = _lib()
    names = [n for n, _ in _l.LstmBidirPlanInfo._fields_]
    assert tuple(names) == R.PLAN_FIELDS
    assert ctypes.sizeof(_l.LstmBidirPlanInfo) == 4 * 12
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_lstm_bidir_plan_info {")[1].split("}")[0]
    assert [w.strip() for w in decl.replace("int ", "").replace(";", "").split(",")] == names
    # the call writes its twelve ints and nothing past them
    buf = (ctypes.c_int * 16)(*([-7] * 16))
    d = _desc(R.CASES[0])
    assert handle.amdspeech_lstm_bidir_plan(ctypes.byref(d), ctypes.cast(buf, ctypes.POINTER(_l.LstmBidirPlanInfo))) == 0
    assert list(buf[12:]) == [-7] * 4 and -7 not in list(buf[:12])
    # the wrapper is read-only: the workspace's own flags stay as they were
    from rnn_speech_amd import ops
    ws = types.SimpleNamespace(lib=handle, desc=_desc(R.CASES[0], flags=_l.LSTM_INJECT_TIMEOUT))
    assert ops.lstm_bidir_plan(ws, per_frame=True)["path"] == 0 and ws.desc.flags == _l.LSTM_INJECT_TIMEOUT


@pytest.mark.parametrize("case", _PLAN_CASES, ids=[c["name"] for c in _PLAN_CASES])
def test_bidir_plan_is_what_the_mirror_expects(case):
    _l, handle = _lib()
    got, want = _plan(case), R.expected_plan(case, cus=0)
    assert tuple(got) == R.PLAN_FIELDS
    for name in R.PLAN_FIELDS[2:]:
        assert got[name] == want[name], (case["name"], name, got, want)
    if not torch.cuda.is_available():      # (with a device the path and the CUs are its own: tests/test_gpu_bidir_layer_paths.py)
        assert (got["path"], got["cus"]) == (0, 0)
    flagged = _plan(case, per_frame=True)
    assert flagged["path"] == 0 and {k: v for k, v in flagged.items() if k != "path"} == {k: v for k, v in got.items() if k != "path"}
    for flags, plan in ((0, got), (_l.LSTM_PER_DIAGONAL, flagged)):
        assert handle.amdspeech_lstm_bidir_path(ctypes.byref(_desc(case, flags))) == plan["path"]


def test_bidir_plan_refuses_what_the_calls_refuse_in_their_words():
    _l, handle = _lib()
    info = _l.LstmBidirPlanInfo()
    base = R.CASES[0]

    def refused(d, out=info):
        rc = handle.amdspeech_lstm_bidir_plan(ctypes.byref(d), ctypes.byref(out) if out is not None else None)
        return rc, handle.amdspeech_last_error().decode()

    assert refused(_desc(base, precision=2, H=64)) == (EUNSUPPORTED, "lstm_bidir: the layer-wise bidirectional mode runs in exact f32 "
                                                       "(precision 0) or bf16x3 (1), not plain bf16 (2)")
    assert refused(_desc(base, H=1040)) == (EUNSUPPORTED, "lstm_bidir: hidden size 1040 above 1024 (the recurrence keeps H x 32 floats of "
                                            "W_hh per workgroup in LDS)")
    assert refused(_desc(base, precision=1, H=288)) == (
        EUNSUPPORTED, "lstm_bidir: bf16x3 does not take hidden size 288: its kernels split the H (forward) and 4H (backward) rows of W_hh "
                      "over at most 8 waves, 32 x 1, 2, 4, 8 or 16 rows each (H = 64, 128, 256, 512, 768, 1024 qualify)")
    assert handle.amdspeech_lstm_bidir_plan(ctypes.byref(_desc(base, H=288)), ctypes.byref(info)) == 0      # (exact f32 takes it)
    assert refused(_desc(base), out=None) == (EINVAL, "lstm_bidir_plan: null output")
    # ... and amdspeech_lstm_bidir_path answers the same status
    assert handle.amdspeech_lstm_bidir_path(ctypes.byref(_desc(base, precision=2, H=64))) == EUNSUPPORTED
