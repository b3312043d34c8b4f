"""The transducer checker and the host side of csrc/transducer.hip, no GPU needed: the float64 lattice loss of transducer_ref against
brute-force enumeration of every alignment and against finite differences, the float32 emulation under the caps on every slice of
the case table, planted faults caught, the plan query with its boundaries and refusals, the label sparsification against CTC's, and
a safe top-two margin on every decoder case."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402
import transducer_ref as R  # noqa: E402
from oracle import model as om  # noqa: E402
from rnn_speech_amd import lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3      # include/amdspeech.h
CASE_NAMES = [c["name"] for c in R.cases(ops.rnnt_plan)]


def _log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


# ---- 1. the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 3, 4))
@pytest.mark.parametrize("n", (0, 1, 2, 3))
def test_the_reference_loss_equals_brute_force_enumeration_of_every_alignment(T, n):
    C = 4
    rng = np.random.RandomState(10 * T + n)
    x = rng.randn(1, T, n + 1, C) * 2.0
    y = np.array([[1, 1, 2][:n] + [0] * (3 - n)], np.int32)      # (a repeated label among them)
    loss, _ = R.loss_ref(x, y, [n], [T])
    want = R.brute_force_loss(_log_softmax(x[0]), y[0], C - 1)
    assert abs(loss[0] - want) <= 1e-12 * max(1.0, abs(want))


def test_the_reference_gradient_equals_finite_differences_in_float64():
    T, U, C = 4, 3, 5
    rng = np.random.RandomState(3)
    x = rng.randn(3, T, U + 1, C)
    y = np.array([[1, 1, 3], [2, 0, 0], [0, 0, 0]], np.int32)
    n, lengths = [3, 1, 0], [4, 3, 9]
    _, d = R.loss_ref(x, y, n, lengths)
    live = R.live_mask(lengths, n, T, U)
    assert not d[~live].any()
    h = 1e-6
    for idx in [(0, 0, 0, 1), (0, 3, 3, 4), (0, 2, 1, 1), (1, 2, 1, 4), (1, 0, 0, 2), (2, 3, 0, 4), (2, 1, 0, 0), (1, 3, 0, 0)]:
        xp, xm = x.copy(), x.copy()
        xp[idx] += h; xm[idx] -= h
        fd = (R.loss_ref(xp, y, n, lengths)[0].sum() - R.loss_ref(xm, y, n, lengths)[0].sum()) / (2 * h)
        assert abs(fd - d[idx]) < 1e-8, (idx, fd, d[idx])
    assert np.abs(d.sum(axis=-1)).max() < 1e-14                  # a row of the gradient sums to zero


# ---- 2. the emulation and the bounds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_emulation_stays_under_the_caps_on_every_slice(name):
    ev = R.evaluated(name, ops.rnnt_plan)
    for k, e in ev["emu_errors"].items():
        assert e <= (R.LOSS_CAP if k[0] == "loss" else R.D_CAP) / R.FACTOR, (k, e)
        assert ev["bounds"][k] <= (R.LOSS_CAP if k[0] == "loss" else R.D_CAP)
    assert not R.judge(ev, ev["emu_loss"], ev["emu_d"])
    live = ev["live"]
    assert (np.abs(ev["logits_emu"] - ev["logits_ref"]) <= ev["logits_bound"])[live].all()
    for emu, ref, bound in zip(ev["bwd_emu"], ev["bwd_ref"], ev["bwd_bounds"]):
        assert (np.abs(emu - ref) <= bound).all()
        assert (bound <= 2e-3 * max(np.abs(ref).max(), 1.0) * max(1.0, live.sum() / 64.0)).all()      # the formulas stay small
    # the float32 recursion state, for the record of the choice (transducer_ref's docstring): harmless at the table's sizes
    for k, e in R.state32_errors(name, ops.rnnt_plan).items():
        assert e <= (R.LOSS_CAP if k[0] == "loss" else R.D_CAP), (k, e)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_in_the_emulation_are_caught(fault):
    caught = 0
    for name in ("t-tile", "large", "t2-ragged"):
        ev = R.evaluated(name, ops.rnnt_plan)
        loss, d = R.emulate_loss(ev["logits32"], ev["targets"], ev["n"], ev["lengths"], fault=fault)
        caught += bool(R.judge(ev, loss, d))
    assert caught == 3


# ---- 3. the plan query -------------------------------------------------------------------------------------------------------
def test_the_plan_struct_is_the_header_s_and_the_table_reaches_every_instantiation():
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_rnnt_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.RnntPlanInfo._fields_]
    assert ctypes.sizeof(lib.RnntPlanInfo) == 4 * len(lib.RnntPlanInfo._fields_)
    consts = sorted((int(v), n.lower()) for n, v in re.findall(r"AMDSPEECH_RNNT_REC_([A-Z0-9]+) (\d+)", header))
    assert consts == list(enumerate(lib.RNNT_REC_KERNELS))
    for name in ("amdspeech_rnnt_joint_fwd", "amdspeech_rnnt_joint_bwd", "amdspeech_rnnt_loss_fwd_bwd", "amdspeech_rnnt_targets",
                 "amdspeech_rnnt_greedy_step", "amdspeech_lm_step_state"):
        proto = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert len(proto.group(1).split(",")) == len(lib.PROTOTYPES[name][1]), name
    cols, recs = set(), set()
    for c in R.cases(ops.rnnt_plan):
        p = ops.rnnt_plan(c["T"], c["B"], c["U"], c["J"], c["C"])
        cols.add(p["col_tiles"]); recs.add(p["rec_kernel"])
    assert cols == {2, 5, 8, 16} and recs == set(lib.RNNT_REC_KERNELS)


def test_the_plan_s_ranges_tile_the_limits_and_the_headline_shape():
    c, classes = 2, []
    while c <= 256:
        p = ops.rnnt_plan(4, 1, 4, 16, c)
        assert p["c_min"] == c and p["c_max"] >= c and ops.rnnt_plan(4, 1, 4, 16, p["c_max"])["col_tiles"] == p["col_tiles"]
        assert 16 * p["col_tiles"] >= p["c_max"]
        classes.append((p["c_min"], p["c_max"], p["col_tiles"], p["fwd_u_tile"], p["bwd_k_slice"]))
        c = p["c_max"] + 1
    assert classes == [(2, 32, 2, 64, 64), (33, 80, 5, 64, 64), (81, 128, 8, 32, 32), (129, 256, 16, 16, 16)]
    u, recs = 1, []
    while u <= 2559:
        p = ops.rnnt_plan(1, 1, u, 16, 5)
        assert p["u_min"] == u and p["rec_threads"] * p["rec_states"] >= p["u_max"] + 1
        recs.append((p["rec_kernel"], p["u_max"]))
        u = p["u_max"] + 1
    assert recs == [("wave", 63), ("block1", 255), ("block4", 1023), ("block10", 2559)]
    p = ops.rnnt_plan(334, 32, 161, 512, 80)
    assert (p["j_min"], p["j_max"]) == (16, 1024)
    assert (p["fwd_t_tiles"], p["fwd_u_tiles"], p["fwd_grid"]) == (84, 3, 84 * 3 * 32)
    assert (p["bwd_t_chunk"], p["bwd_t_chunks"], p["bwd_k_slices"], p["bwd_grid"]) == (44, 8, 8, 32 * 8 * 8)
    assert p["rec_kernel"] == "block1" and p["rec_grid"] == 64
    assert max(p["fwd_lds_bytes"], p["bwd_lds_bytes"], p["rec_lds_bytes"]) <= 64 * 1024
    # the workspace: the documented sum, and nothing of the size of z (N J floats = 3.5 GB here)
    N = 32 * 334 * 162
    up = lambda v: -(-v // 256) * 256      # noqa: E731
    want = 2 * up(4 * N) + 2 * up(8 * N) + up(8 * 32) + up(4 * 8 * 162 * 32 * 512) + up(4 * 256 * 512 * 80) + up(4 * 256 * 80)
    assert p["workspace_bytes"] == want and want < 4 * N * 512 // 16
    assert ops.rnnt_plan(1001, 32, 161, 512, 80)["bwd_t_chunks"] == 8


def test_every_refusal_names_its_limit_and_launches_nothing():
    handle = lib.load()
    info = lib.RnntPlanInfo()
    for args, rc, word in (((4, 1, 4, 24, 5), EINVAL, "multiple of 16"), ((4, 1, 4, 0, 5), EINVAL, "multiple of 16"),
                           ((4, 1, 4, 1040, 5), EUNSUPPORTED, "limit of 1024"), ((4, 1, 4, 16, 1), EINVAL, "at least 2"),
                           ((4, 1, 4, 16, 257), EUNSUPPORTED, "limit of 256"), ((4, 1, 0, 16, 5), EINVAL, "at least 1"),
                           ((4, 1, 2560, 16, 5), EUNSUPPORTED, "limit of 2559"), ((0, 1, 4, 16, 5), EINVAL, "must be positive"),
                           ((4, 0, 4, 16, 5), EINVAL, "must be positive"), ((4096, 64, 2048, 16, 4), EUNSUPPORTED, "below 2^31")):
        assert handle.amdspeech_rnnt_plan(*args, ctypes.byref(info)) == rc, args
        assert word.encode() in handle.amdspeech_last_error(), (args, handle.amdspeech_last_error())
        assert handle.amdspeech_rnnt_workspace_bytes(*args) == 0
        with pytest.raises(lib.AmdSpeechError, match=re.escape(word)):
            ops.rnnt_plan(*args)
        # the calls check their shape before anything else: no pointer is looked at, nothing is launched
        T, B, U, J, C = args
        assert handle.amdspeech_rnnt_joint_fwd(None, None, None, None, None, None, None, T, B, U, J, C, None) == rc
        assert handle.amdspeech_rnnt_joint_bwd(None, None, None, None, None, None, None, T, B, U, J, C, None, None, None, None, None) == rc
    assert handle.amdspeech_rnnt_plan(4, 1, 4, 16, 5, None) == EINVAL
    assert handle.amdspeech_rnnt_loss_fwd_bwd(None, None, None, None, None, 4, 1, 2560, 5, None, None, None) == EUNSUPPORTED
    assert handle.amdspeech_rnnt_targets(None, None, 1, 2560, 5, None, None, None, None) == EUNSUPPORTED
    assert handle.amdspeech_rnnt_joint_fwd(None, None, None, None, None, None, None, 4, 1, 4, 16, 5, None) == EINVAL
    assert b"null pointer" in handle.amdspeech_last_error()
    assert handle.amdspeech_rnnt_greedy_step(None, None, None, 4, 1, 4, 16, 5, None, 9, 16, *([None] * 11)) == EINVAL
    assert b"1 .. 8" in handle.amdspeech_last_error()
    assert handle.amdspeech_lm_step_state(None, 1, None, None, None, None, None, 4, 1, 24, 6, None, None, None, 0, None, 0) == EINVAL
    assert b"multiple of 16" in handle.amdspeech_last_error()


# ---- 4. the targets ----------------------------------------------------------------------------------------------------------
def test_the_sparsification_agrees_with_ctc_s_on_the_golden_label_rows_except_for_empty_rows():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "labels.json")))
    rows = [e["ids"] for e in g["encode"]] + [[0, 0], [79], [0, 79, 5], [5, 0, 5, 80, 7], []]
    U, C = max(len(r) for r in rows) + 2, 80
    dense = np.zeros((len(rows), U), np.int32)
    for b, r in enumerate(rows):
        dense[b, :len(r)] = r
    targets, n, tok, tok_len = R.targets_ref(dense, C)
    empties = 0
    for b, kept in enumerate(om.sparsify_labels(dense, C)):
        want, _ = om.ctc_targets(kept, C)
        if not any(v != 0 for v in dense[b]):
            empties += 1
            assert kept == [C - 1] and n[b] == 0                 # CTC fills an empty row with EOS; here it is a valid empty target
        assert list(targets[b, :n[b]]) == want and not targets[b, n[b]:].any()
        assert list(tok[b]) == [C - 1] + want + [C - 1] * (U + 1 - len(want)) and tok_len[b] == len(want) + 1
    # negative ids are no labels: dropped with the zeros (CTC's kernel keeps them; no dataset of this project produces one)
    t2, n2, tok2, _ = R.targets_ref(np.array([[7, -2, 8, -1, 79, 5]], np.int32), C)
    assert n2[0] == 2 and list(t2[0]) == [7, 8, 0, 0, 0, 0] and list(tok2[0, :4]) == [C - 1, 7, 8, C - 1]
    assert empties == 2 and n.max() > 20 and any(0 in r[:-1] for r in rows)      # (a dropped zero inside a row is among them)


# ---- 5. the decoder cases are decidable ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.GREEDY_CASES])
def test_every_decoder_case_has_a_safe_top_two_margin_at_every_node_visited(name):
    c = R.greedy_case(name)
    args = (c["p"], c["L"], c["f"], c["lengths"], c["U"], c["w"], c["bias"])
    ids, out_len, choices, rows64 = R.greedy_walk(*args, F.lm_step_ref)
    _, _, _, rows32 = R.greedy_walk(*args, F.lm_step_f32, dtype=np.float32, forced=choices)
    margin, err = R.greedy_margins(rows64, rows32)
    assert margin > 2 * R.greedy_logit_bound(err), (margin, err)
    assert sum(len(ch) for ch in choices) >= 6
    if name == "capped":
        assert (out_len == c["U"]).any()                          # a row that stops at m = U with frames left
    assert out_len[list(c["lengths"]).index(0)] == 0              # an empty utterance
    if name != "capped":
        assert 0 < out_len.max() and any(k == c["C"] - 1 for ch in choices for k in ch)


# ---- 6. the configuration keys and the checkpoint names -------------------------------------------------------------------------
def _config(tmp_path, *pairs):
    src = open(os.path.join(ROOT, "config.ini")).read()
    src = src.replace("checkpoint_dir", "checkpoint_dir : %s\n#" % (tmp_path / "ckpt"), 1)
    for old, new in pairs:
        assert old in src, old
        src = src.replace(old, new, 1)
    path = tmp_path / "config.ini"
    path.write_text(src)
    return str(path)


def test_the_config_keys_have_their_defaults_refuse_what_is_outside_and_are_structural(tmp_path):
    from rnn_speech_amd import hyperparams as hp
    d = hp.read_config_file(_config(tmp_path))
    assert (d["objective"], d["transducer_joint_size"], d["transducer_pred_layers"], d["transducer_pred_hidden"]) == ("ctc", 512, 1, 0)
    assert hp.read_objective_keys(lambda key, dflt: dflt) == {k: d[k] for k in hp._STRUCTURAL_OBJECTIVE}      # absent keys: the same
    d = hp.read_config_file(_config(tmp_path, ("objective : ctc", "objective : transducer"), ("transducer_joint_size : 512", "transducer_joint_size : 48"),
                                    ("transducer_pred_layers : 1", "transducer_pred_layers : 2"), ("transducer_pred_hidden : 0", "transducer_pred_hidden : 64")))
    assert (d["objective"], d["transducer_joint_size"], d["transducer_pred_layers"], d["transducer_pred_hidden"]) == ("transducer", 48, 2, 64)
    for pair, word in ((("objective : ctc", "objective : rnnt"), "objective"), (("transducer_joint_size : 512", "transducer_joint_size : 40"), "transducer_joint_size"),
                       (("transducer_joint_size : 512", "transducer_joint_size : 2048"), "transducer_joint_size"),
                       (("transducer_pred_layers : 1", "transducer_pred_layers : 9"), "transducer_pred_layers"),
                       (("transducer_pred_hidden : 0", "transducer_pred_hidden : 24"), "transducer_pred_hidden")):
        with pytest.raises(ValueError, match=word):
            hp.read_config_file(_config(tmp_path, pair))
    handler = hp.HyperParameterHandler(_config(tmp_path))
    params = dict(handler.get_hyper_params())
    assert not handler.check_changed(params)
    for k, v in (("objective", "transducer"), ("transducer_joint_size", 256), ("transducer_pred_layers", 2), ("transducer_pred_hidden", 64)):
        assert handler.check_changed(dict(params, **{k: v})), k
    import pickle
    with open(handler.file_path, "wb") as fh:      # a pickle from before the keys existed
        pickle.dump({k: v for k, v in params.items() if k not in hp._STRUCTURAL_OBJECTIVE}, fh)
    assert not handler.check_changed(params) and handler.check_changed(dict(params, objective="transducer"))


def test_checkpoint_names_round_trip_through_pack_and_unpack_on_a_stand_in_store():
    from rnn_speech_amd import checkpoint

    class Layout(object):
        slots = {"encoder/input_w": (3, 4), "encoder/kernel_0": (4, 8), "encoder/bw_bias_1": (8,), "encoder/lookahead_w": (2, 2),
                 "prediction/input_w": (5, 2), "prediction/bias_0": (8,), "prediction/output_b": (4,), "joint_w": (4, 5), "joint_b": (5,)}

        def names(self):
            return list(self.slots)

    class Store(object):
        def __init__(self, seed):
            rng = np.random.RandomState(seed)
            self.layout, self.adam_step = Layout(), seed
            self.bufs = {f: {k: rng.randn(*s).astype(np.float32) for k, s in Layout.slots.items()} for f in ("p", "m", "v")}
            self.adam_m, self.adam_v = "m", "v"

        def to_numpy(self, flat=None):
            return {k: v.copy() for k, v in self.bufs[flat or "p"].items()}

        def load_numpy(self, arrays, flat=None):
            self.bufs[flat or "p"] = {k: np.array(v) for k, v in arrays.items()}

    a, b = Store(3), Store(4)
    packed = checkpoint.pack(a, 12, 0.5)
    names = {checkpoint.tf_name(k) for k in Layout.slots}
    assert len(names) == len(Layout.slots) and names <= set(packed)
    assert {"Encoder/Input_Layer/input_w", "Encoder/rnn/multi_rnn_cell/cell_0/basic_lstm_cell/kernel", "Encoder/Lookahead_Layer/lookahead_w",
            "Encoder/bidirectional_rnn/bw/multi_rnn_cell/cell_1/basic_lstm_cell/bias", "Prediction/Output_layer/output_b",
            "Joint_Layer/joint_w", "Joint_Layer/joint_b"} <= names
    assert checkpoint.tf_name("input_w") == "Input_Layer/input_w"            # (a plain store's names are what they were)
    assert checkpoint.unpack(packed, b) == (12, 0.5, True) and b.adam_step == 3
    for f in ("p", "m", "v"):
        assert all(a.bufs[f][k].tobytes() == b.bufs[f][k].tobytes() for k in Layout.slots)
