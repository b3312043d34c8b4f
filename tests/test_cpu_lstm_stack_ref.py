"""tests/lstm_stack_ref.py tied down without a GPU: the float64 reference of the LSTM stack against torch.nn.LSTM (autograd) and
against oracle.model, the slice metric against the whole-tensor metric it replaces, the conditions the GPU matrix
(tests/test_gpu_lstm_stack.py) puts on its inputs, and the plan query's wrapper."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_stack_ref as R  # noqa: E402

from oracle import model as om  # noqa: E402


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def _small(T, B, H, L, seed, state=True, lengths=None):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(L, 2 * H, 4 * H, generator=g, dtype=torch.float64) * (0.8 / np.sqrt(H))
    b = torch.randn(L, 4 * H, generator=g, dtype=torch.float64) * 0.3
    z0 = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    dz = torch.randn(T, B, H, generator=g, dtype=torch.float64)
    h0 = torch.randn(L, B, H, generator=g, dtype=torch.float64) * 0.3 if state else None
    c0 = torch.randn(L, B, H, generator=g, dtype=torch.float64) * 0.3 if state else None
    if lengths is None:
        lengths = np.array(([T, T - 1, 1, 0] + list(np.random.RandomState(seed).randint(1, T + 1, size=B)))[:B], np.int32)
    return k, b, z0, dz, h0, c0, lengths


# ------------------------------------------------------------------------------------------------ against torch.nn.LSTM
def _nn_lstm_chain(k, b, z0, lengths, h0, c0):
    """L single-layer torch.nn.LSTM modules (float64) with this stack's weights: gate order i, f, g, o there, i, j, f, o here; the
    forget bias goes into b_ih; packed sequences apply the lengths (rows of length 0 are left out: nn.LSTM does not take them)."""
    L, H = k.shape[0], k.shape[1] // 2
    perm = torch.cat([torch.arange(0, H), torch.arange(2 * H, 3 * H), torch.arange(H, 2 * H), torch.arange(3 * H, 4 * H)])
    rows = np.nonzero(lengths > 0)[0]
    x = z0[:, rows].clone().requires_grad_(True)
    cur, mods, outs, hT, cT = x, [], [], [], []
    for l in range(L):
        m = torch.nn.LSTM(H, H, 1).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(k[l, :H, perm].t())
            m.weight_hh_l0.copy_(k[l, H:, perm].t())
            bias = b[l].clone()
            bias[2 * H:3 * H] += R.FORGET_BIAS
            m.bias_ih_l0.copy_(bias[perm])
            m.bias_hh_l0.zero_()
        packed = torch.nn.utils.rnn.pack_padded_sequence(cur, torch.as_tensor(lengths[rows]).long(), enforce_sorted=False)
        s0 = None if h0 is None else (h0[l:l + 1, rows].contiguous(), c0[l:l + 1, rows].contiguous())
        y, (hn, cn) = m(packed, s0)
        cur, _ = torch.nn.utils.rnn.pad_packed_sequence(y, total_length=z0.shape[0])
        mods.append(m)
        outs.append(cur)
        hT.append(hn[0])
        cT.append(cn[0])
    return x, mods, outs, torch.stack(hT), torch.stack(cT), rows, perm


@pytest.mark.parametrize("T,B,H,L,state", [(7, 6, 16, 3, True), (12, 5, 32, 2, False), (1, 3, 16, 1, True)])
def test_reference_is_nn_lstm_in_float64(T, B, H, L, state):
    k, b, z0, dz, h0, c0, lengths = _small(T, B, H, L, seed=T + B, state=state)
    f = R.forward(z0, k, b, lengths, h0, c0)
    r = R.backward(f["cache"], dz)
    x, mods, outs, hT, cT, rows, perm = _nn_lstm_chain(k, b, z0, lengths, h0, c0)
    (outs[-1] * dz[:, rows]).sum().backward()
    inv = torch.argsort(perm)
    assert _rel(f["ztop"][:, rows], outs[-1]) < 1e-12
    live = torch.as_tensor(np.arange(T)[:, None] < lengths[rows][None, :])[:, :, None]
    for l in range(L):      # nn.LSTM pads with 0 where the reference carries the state: valid frames
        assert _rel(f["h"][l][:, rows] * live, outs[l]) < 1e-12, l
        dk_ref = torch.cat([mods[l].weight_ih_l0.grad.t(), mods[l].weight_hh_l0.grad.t()])[:, inv]
        assert _rel(r["dK"][l], dk_ref) < 1e-12, l
        assert _rel(r["db"][l], mods[l].bias_ih_l0.grad[inv]) < 1e-12, l
    assert _rel(f["hT"][:, rows], hT) < 1e-12 and _rel(f["cT"][:, rows], cT) < 1e-12
    assert _rel(r["dz0"][:, rows], x.grad) < 1e-12
    dead = np.nonzero(lengths == 0)[0]
    assert R.padding_is_zero(f["ztop"], lengths) and R.padding_is_zero(r["dz0"], lengths)
    if state and len(dead):      # rows without a frame: the state passes through untouched
        assert torch.equal(f["hT"][:, dead], h0[:, dead]) and torch.equal(f["cT"][:, dead], c0[:, dead])


# ------------------------------------------------------------------------------------------------ against oracle.model
@pytest.mark.parametrize("dropout", [False, True])
def test_reference_is_the_oracle_with_identity_linear_layers(dropout):
    T, B, H, L = 6, 5, 16, 3
    k, b, z0, dz, h0, c0, lengths = _small(T, B, H, L, seed=3)
    im = om_ = None
    if dropout:
        g = torch.Generator().manual_seed(5)
        im = [(torch.rand(T, B, H, generator=g) < 0.8).double() / 0.8 for _ in range(L)]
        om_ = [(torch.rand(T, B, H, generator=g) < 0.6).double() / 0.6 for _ in range(L)]
    f = R.forward(z0, k, b, lengths, h0, c0, im, om_)
    r = R.backward(f["cache"], dz)
    # the oracle's input Linear as a table look-up (x = one-hot rows, W = z0: its weight gradient IS dz0), its output Linear = identity
    p = {"input_w": z0.reshape(T * B, H).numpy().copy(), "input_b": np.zeros(H), "output_w": np.eye(H), "output_b": np.zeros(H)}
    for l in range(L):
        p["kernel_%d" % l], p["bias_%d" % l] = k[l].numpy(), b[l].numpy()
    x = np.eye(T * B).reshape(T, B, T * B)
    state = [(c0[l].numpy(), h0[l].numpy()) for l in range(L)]
    npm = lambda ms: None if ms is None else [m.numpy() for m in ms]
    logits, final, cache = om.forward(p, x, lengths, L, state=state, keep_cache=True, in_masks=npm(im), out_masks=npm(om_))
    grads = om.backward(p, cache, dz.numpy(), lengths, L, in_masks=npm(im), out_masks=npm(om_))
    assert _rel(f["ztop"], logits) < 1e-12
    for l in range(L):
        assert _rel(f["cT"][l], final[l][0]) < 1e-12 and _rel(f["hT"][l], final[l][1]) < 1e-12
        assert _rel(f["h"][l] * torch.as_tensor(np.arange(T)[:, None] < lengths[None, :])[:, :, None], cache["layers"][l]["out"]) < 1e-12
        assert _rel(r["dK"][l], grads["kernel_%d" % l]) < 1e-12 and _rel(r["db"][l], grads["bias_%d" % l]) < 1e-12
    assert _rel(r["dz0"].reshape(T * B, H), grads["input_w"]) < 1e-12


# ------------------------------------------------------------------------------------------------ the slice metric
def test_slice_metric_catches_what_the_whole_tensor_metric_misses():
    T, B, H, L = 12, 33, 32, 2
    k, b, z0, dz, h0, c0, lengths = _small(T, B, H, L, seed=9, lengths=np.full(33, 12, np.int32))
    b[1, 2 * H:3 * H] = 9.0         # layer 1's forget gate saturated: its bias gradient is small against the other gates'
    dz[:, 32:] *= 5e-4              # the last batch tile (one row) hardly matters to the loss
    f = R.forward(z0, k, b, lengths, h0, c0)
    ref = R.backward(f["cache"], dz)
    # 1. layer 1's forget-gate block of db with the wrong sign
    bad = ref["db"].clone()
    bad[1, 2 * H:3 * H] *= -1
    assert R.rel_err(bad, ref["db"]) < 2e-3                      # tests/test_gpu_model.py's metric at its f32 tolerance: passes
    err, label = R.worst(R.slice_errors(bad, ref["db"], "db"))
    assert err == pytest.approx(2.0) and label.startswith("layer 1 gate f"), (err, label)
    # 2. the last batch tile of dz0 never written
    bad = ref["dz0"].clone()
    bad[:, 32:] = 0
    assert R.rel_err(bad, ref["dz0"]) < 2e-3
    err, label = R.worst(R.slice_errors(bad, ref["dz0"], "dz0", lengths))
    assert err == pytest.approx(1.0) and label.startswith("rows 32:33"), (err, label)
    # ... and neither slice is under the floor, the intact tensors have no error, and padding is checked exactly
    for kind in ("db", "dz0"):
        e = R.slice_errors(ref[kind], ref[kind], kind, lengths)
        assert max(x[1] for x in e) == 0.0 and min(x[2] for x in e) >= R.FLOOR
    lengths2 = lengths.copy()
    lengths2[5] = 7
    leak = torch.zeros(T, B, H)
    assert R.padding_is_zero(leak, lengths2)
    leak[9, 5, 3] = 1e-30
    assert not R.padding_is_zero(leak, lengths2)


def test_slices_tile_every_tensor_exactly_once():
    T, B, H, L = 7, 20, 144, 2
    lengths = np.array([7, 6, 1, 0] + [5] * 16, np.int32)
    for kind, shape in (("dK", (L, 2 * H, 4 * H)), ("db", (L, 4 * H)), ("hT", (L, B, H)), ("ztop", (T, B, H)), ("h", (L, T, B, H))):
        count = torch.zeros(shape)
        for _, idx in R.slices(kind, shape, lengths):
            if kind in ("ztop", "h"):
                idx, valid = idx
                count[idx] += torch.as_tensor(valid, dtype=torch.float32)[:, :, None]
            else:
                count[idx] += 1
        if kind in ("ztop", "h"):
            want = torch.as_tensor(np.arange(T)[:, None] < lengths[None, :], dtype=torch.float32)[:, :, None].expand(T, B, H)
            assert torch.equal(count, want.expand(shape)), kind
        else:
            assert bool((count == 1).all()), kind
    assert len(R.slices("dK", (L, 2 * H, 4 * H))) == L * 2 * 4 * 2          # H = 144: K blocks 0:128 and 128:144
    assert len(R.slices("dK", (1, 64, 128))) == 8                           # H = 32 < 128: the whole half


# ------------------------------------------------------------------------------------------------ the matrix's inputs
_REF = {}


def _case_ref(case):
    if case["name"] not in _REF:
        inp = R.make_inputs(case)
        im, om_ = R.cpu_masks(case)
        _REF[case["name"]] = (inp, R.reference(case, inp, im, om_))
    return _REF[case["name"]]


@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_no_case_of_the_matrix_leaves_out_a_slice(case):
    inp, ref = _case_ref(case)
    for kind in R.OUTPUT_KINDS + R.GRAD_KINDS:
        errs = R.slice_errors(ref[kind], ref[kind], kind, inp["lengths"])
        assert errs, kind
        label, _, frac = min(errs, key=lambda e: e[2])
        assert frac >= R.FLOOR, "%s: slice %s has %.1e of the tensor's maximum" % (kind, label, frac)
    assert R.padding_is_zero(ref["ztop"], inp["lengths"]) and R.padding_is_zero(ref["dz0"], inp["lengths"])
    # what the case promises about its inputs
    valid = ~inp["dead"]
    assert bool((inp["dztop"][valid].abs() >= 0.01).all()), "dztop dense on every valid frame"
    assert bool((inp["garbage"].abs() >= 1.0).all()) and bool(torch.isfinite(inp["garbage"]).all()) and float(inp["garbage"].abs().max()) <= 1e3
    lens = inp["lengths"]
    if case["lens"] == "full":
        assert (lens == case["T"]).all()
    else:
        assert lens[0] == case["T"] or case["lens"] == "last_tile_empty" and case["B"] <= 16
        if case["lens"] == "last_tile_empty":
            assert (lens[(case["B"] - 1) // 16 * 16:] == 0).all() and case["state"]


@pytest.mark.parametrize("case", [c for c in R.CASES if c["regime"] == "saturating"],
                         ids=[c["name"] for c in R.CASES if c["regime"] == "saturating"])
def test_saturating_cases_run_the_gates_in_their_tails(case):
    inp = R.make_inputs(case)
    gates = R.gate_values(inp["z0"], inp["k"], inp["b"], inp["lengths"], inp["h0"], inp["c0"])
    frac = float(((gates < 1e-2) | (gates > 1 - 1e-2)).double().mean())
    assert 0.1 <= frac <= 0.5, frac


def test_matrix_covers_the_edges_the_issue_lists():
    by = lambda key: {c[key] for c in R.CASES}
    assert {1, 15, 16, 17, 33, 64} <= by("B")
    assert {1, 2, 8, 10, 63, 64, 65} <= by("T")
    fams = {R.family(c) for c in R.CASES}
    assert fams == {"diag", "diag_bf3", "hoist", "flow", "flow-reduced", "big"}
    for fam in fams:
        mine = [c for c in R.CASES if R.family(c) == fam]
        assert any(c["T"] >= 200 for c in mine), fam
        assert any(c["state"] for c in mine), fam
        assert {c["regime"] for c in mine} == {"nominal", "saturating"}, fam
        for extra in ("padding", "accumulate", "dropout"):
            assert any(extra in c["extras"] for c in mine), (fam, extra)
    assert any(c["lens"] == "full" for c in R.CASES) and any(c["lens"] == "last_tile_empty" for c in R.CASES)
    covered = {v for c in R.CASES for v in c["covers"]}
    assert covered == set(R.VARIANTS), covered ^ set(R.VARIANTS)
    assert len({c["name"] for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:       # every (family, regime, precision) has its measured row, every kind a bound under its cap
        for kind in R.OUTPUT_KINDS + R.GRAD_KINDS:
            cap = R.CAPS[c["precision"]][0 if kind in R.OUTPUT_KINDS else 1]
            assert 0 < R.bound(c, kind) <= cap


def test_measured_table_is_the_emulated_arithmetic_of_this_matrix():
    """The table in lstm_stack_ref.py's docstring is a recorded run; float32 on another CPU sums in another order, so the figures
    move a little -- but a table that no longer belongs to the matrix (a case added, a scale changed) is off by more than 4x."""
    now = R.measure()
    assert set(now) == set(R.MEASURED)
    for key, row in now.items():
        for kind, e in row.items():
            assert R.MEASURED[key][kind] / 4 <= e <= 4 * R.MEASURED[key][kind], (key, kind, e, R.MEASURED[key][kind])


# ------------------------------------------------------------------------------------------------ the plan query, without a GPU
_BUILT = []


def _library():
    if not _BUILT:
        import __graft_entry__ as g
        g.build()
        _BUILT.append(True)
    from rnn_speech_amd import lib
    return lib


def _plan(case, head=None):
    lib = _library()
    from rnn_speech_amd import ops
    ws = types.SimpleNamespace(lib=lib.load(), desc=lib.LstmDesc(case["T"], case["B"], case["H"], case["L"], 1.0, 1.0, 0, case["precision"], 0))
    return ops.lstm_plan(ws, head=head, per_diagonal="per_diagonal" in case["extras"])


def test_plan_query_wrapper_and_struct_layout():
    lib = _library()
    handle = lib.load()
    names = [n for n, _ in lib.LstmPlanInfo._fields_]
    assert names == ["fwd_path", "bwd_path", "nmt", "kb", "mv", "wpx", "uw", "fwd_mt", "pair", "bf16p", "bf16p_reserved", "xw_parts", "nfw",
                     "w_pieces", "dz0_inkernel", "flow2_q"]
    assert ctypes.sizeof(lib.LstmPlanInfo) == 4 * len(names)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_lstm_plan_info {")[1].split("}")[0]
    assert [w.strip() for w in decl.replace("int ", "").replace(";", "").split(",")] == names
    for i, name in enumerate(lib.LSTM_PATHS):
        assert "AMDSPEECH_LSTM_PATH_%s = %d" % (name.upper(), i) in header
    # the call writes its 16 ints and nothing past them
    buf = (ctypes.c_int * 20)(*([-7] * 20))
    d = lib.LstmDesc(10, 33, 64, 6, 1.0, 1.0, 0, 0, 0)
    assert handle.amdspeech_lstm_plan(ctypes.byref(d), 0, 0, ctypes.cast(buf, ctypes.POINTER(lib.LstmPlanInfo))) == 0
    assert list(buf[16:]) == [-7] * 4 and -7 not in list(buf[:16])
    # errors: a bad descriptor, half a head
    bad = lib.LstmDesc(10, 2, 50, 1, 1.0, 1.0, 0, 0, 0)
    assert handle.amdspeech_lstm_plan(ctypes.byref(bad), 0, 0, ctypes.cast(buf, ctypes.POINTER(lib.LstmPlanInfo))) != 0
    assert handle.amdspeech_lstm_plan(ctypes.byref(d), 80, 0, ctypes.cast(buf, ctypes.POINTER(lib.LstmPlanInfo))) != 0
    assert handle.amdspeech_lstm_plan(ctypes.byref(d), 0, 0, None) != 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="with a GPU the plans are the MI355X's: tests/test_gpu_lstm_stack.py asserts them")
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_without_a_gpu_every_shape_plans_the_launch_per_diagonal_kernels(case):
    """use_flow / use_big_fwd ask the device for its CU count; without one the answer is diag (diag_bf3 in reduced precision), with
    the hoisted backward where its rule holds -- and the device-independent fields are what csrc/lstm.hip's rules give."""
    p = _plan(case)
    T, B, H, L, pr = (case[k] for k in ("T", "B", "H", "L", "precision"))
    nmt = (B + 15) // 16
    assert p["fwd_path"] == ("diag" if pr == 0 else "diag_bf3")
    assert p["bwd_path"] == ("hoist" if pr == 0 and H >= 768 and nmt >= 2 else p["fwd_path"])
    assert p["nmt"] == nmt and p["fwd_mt"] == (2 if nmt % 2 == 0 else 1)
    assert p["uw"] == (8 if L * (H // 8) * ((B + 31) // 32) >= 96 else 4)                     # pick_uw
    assert (p["kb"], p["mv"], p["wpx"], p["pair"], p["nfw"], p["w_pieces"], p["flow2_q"]) == (0,) * 7
    assert p["xw_parts"] == int(pr == 0 and H == 512 and L * nmt < 8)                           # fwd_workers_fit: the layout reserves it
    assert p["bf16p_reserved"] == int(pr == 2 and H == 1024)
    assert p["bf16p"] == int(pr == 2 and H == 1024 and (T * B) % 64 == 0 and T * B >= 256)
    assert _plan(case, head=(80, 20))["nfw"] == 0                                                # no head off the dataflow path
