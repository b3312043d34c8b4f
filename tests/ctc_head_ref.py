"""Cases, expected plans, stage references and bounds for the CTC head INSIDE the whole-sequence LSTM launches
(amdspeech_lstm_fwd_ctc / amdspeech_lstm_bwd_ctc, csrc/ctc_flow.h: ctc_follower behind the forward recurrence, ctc_leader ahead of
the backward one).  Checker only: numpy and torch on the CPU, nothing of the product is imported.  The glue between tests/ctc_ref.py
(float64 CTC, the `fam="head"` emulation, `judge`) and tests/lstm_stack_ref.py (float64 LSTM, slices, `bound`).

One forward and one backward call per case; then five stages, each judged against float64 ON THE STAGE'S OWN GPU INPUT, so that no
stage inherits the error of the one before it and a wrong tile shows up in the stage that made it:

  1  LSTM forward with the follower attached: ztop, the h history, hT, cT against lstm_stack_ref.forward, slice by slice.
  2  output Linear: logits[t, b, :] against float64 ztop_gpu[t, b, :] . W_o + b_o (ztop_gpu: the masked top-layer output read back
     from the workspace; the follower reads its own packed copy, so a wrong panel shows here).  Slices: (utterance, 16-frame chunk,
     16-label tile).  At frames lengths[b] <= t < T the operand is exactly zero: the logits are b_o bit for bit.
  3  loss and dlogits against ctc_ref.reference on the GPU logits, judged by ctc_ref.judge with fam="head" (the head always runs
     the shift recursion: the ("shift", 2, 256) emulation at every S); exact zeros for padded rows, over-long targets and frames at
     and past a row's length; an all-zero label row takes the [C-1] target.
  4  dZ_top against float64 dlogits_gpu . W_o^T (K = C).  Slices: (utterance, 16-frame chunk, the wave's 16-unit tile).  The
     dataflow backward kernel only READS the buffer (lstm_flow_bwd.h: `const float* dztop`, polled against the sentinel; only the
     hoisted backward of other shapes reuses it), so after lstm_bwd returns ws.dztop still holds what ctc_leader wrote: it is
     compared directly, and is exactly zero past the lengths and on rows without a gradient.
  5  BPTT behind the leader: dK, db, dz0 against lstm_stack_ref.backward run on the float64 product of stage 4 as dztop, with the
     slices and the padding-is-zero checks of the stack test.  This is where the dealt weight-gradient workers (w_deal) and the
     late-joining leader teams are judged.

The `nopath` branch of ctc_leader (log p(l|x) = -inf on a valid row) cannot be reached with finite weights through an LSTM: every
label row of every case fits its frames (the deliberate over-long row is INVALID, not impossible).  It has no case.

Bounds.  None comes from a GPU.
  stages 1, 5  min(cap, 8 x measured), lstm_stack_ref.bound's form with its CAPS and FACTOR; `measured` is the largest per-slice
               relative error the emulated arithmetic of the precision (lstm_stack_ref `emulate`) shows against float64 over the
               head cases of a (regime, precision): MEASURED below, family "flow+head".  For stage 5 the emulated dztop goes
               through an f32 K = C product first (emulate_dztop), so the leader's rounding is part of the measurement.
  stage 2      min(2e-6, 8 x measured) of the slice's max(|reference|, 1) -- today's whole-tensor 2e-6 x max(scale, 1) applied per
               slice; `measured`: the per-slice error of emulate_linear (the kernel's order: four K quarters accumulated separately
               in f32, then ((p0 + p1) + p2) + p3 + b_o) against float64, largest over the cases of an H: LINEAR_MEASURED.
  stage 4      min(8 x D_FLOOR, 8 x measured) of the slice's largest sum_c |dlogits| |W_o|; `measured`: emulate_dztop (f32, 16-label
               K blocks in the leader's order) against float64, largest over the cases of a C: DZTOP_MEASURED.  The cap is
               ctc_ref.D_FLOOR (2^-21: four float32 roundings of a number of the magnitude of the sum's terms) in the form
               ctc_ref.bounds applies it, FACTOR x D_FLOOR, per slice.  D_FLOOR x the scale WITHOUT the factor is no usable cap:
               a float32 product over K = 80 labels is 0.43e-6 of that scale away from float64 in the emulation itself (the
               order of 80 roundings, not four), which leaves the emulation no margin under 0.48e-6 and the matrix cores' other
               summation order none at all -- on an MI355X the worst slice of the 3x512 case sits at 0.54e-6, 7 of 2592 slices
               over 0.48e-6.  Every planted mistake below is 1e-5 of the scale or more.
  stage 3      ctc_ref.bounds(..., "head", ...) as it stands.
A slice is left out only if it holds no valid frame of a valid row; it is then asserted exactly zero (stage 4) or equal to b_o
(stage 2).  tests/test_cpu_ctc_head_ref.py asserts, with the float64 reference alone, that every other slice of every case has a
reference maximum above FLOOR of its tensor.

`PYTHONPATH=. python tests/ctc_head_ref.py` (CPU only, seconds) measures the tables; the figures below are that run.

MEASURED (family flow+head; largest per-slice relative error of the emulated arithmetic against float64; bound = min(cap, 8 x)):
regime     pr | ztop            | h               | hT              | cT              | dK              | db              | dz0            
nominal    0  | 7.3e-07>5.8e-06  | 9.5e-07>7.6e-06  | 6.4e-07>5.1e-06  | 4.6e-07>3.7e-06  | 9.1e-07>7.3e-06  | 1.0e-06>8.3e-06  | 1.2e-06>9.7e-06 
nominal    1  | 5.9e-06>4.8e-05  | 9.4e-06>7.6e-05  | 6.6e-06>5.3e-05  | 4.1e-06>3.3e-05  | 5.9e-06>4.7e-05  | 8.7e-06>6.9e-05  | 1.0e-05>8.3e-05 
nominal    2  | 7.6e-03>1.0e-02c | 7.6e-03>1.0e-02c | 3.9e-03>1.0e-02c | 3.0e-03>1.0e-02c | 4.5e-03>3.0e-02c | 4.2e-03>3.0e-02c | 5.1e-03>3.0e-02c
saturating 0  | 8.4e-06>6.7e-05  | 8.4e-06>6.7e-05  | 8.4e-06>6.7e-05  | 1.5e-06>1.2e-05  | 5.7e-06>4.5e-05  | 1.4e-05>1.1e-04  | 9.1e-06>7.3e-05 
stage 2 (by H, of max(|slice|, 1); cap 2e-06): 128: 2.7e-07>2.0e-06  256: 4.4e-07>2.0e-06  384: 3.5e-07>2.0e-06  512: 5.3e-07>2.0e-06
stage 4 (by C, of the slice's sum |dlogits| |W_o|; cap 3.8e-06): 16: 2.2e-07>1.8e-06  32: 1.1e-07>8.8e-07  48: 1.8e-07>1.4e-06  64: 2.4e-07>1.9e-06  80: 4.3e-07>3.4e-06
(measured>bound; c: the bound is the cap)
"""
import functools

import numpy as np
import torch

import ctc_ref as CR
import lstm_stack_ref as S

F32, F64 = np.float32, np.float64
FAMILY = "flow+head"
FLOOR = S.FLOOR
FACTOR = S.FACTOR
LOGIT_CAP = 2e-6              # tests/test_gpu_ctc_head.py: |logits - other path| < 2e-6 * max(scale, 1), here per slice
DZTOP_CAP = FACTOR * CR.D_FLOOR      # of the slice's sum |dlogits| |W_o|: see "stage 4" above
GRAD_TOL_OLD = 5e-4           # ... and its whole-tensor tolerance on dz0 and the parameter gradients
HEAD_PLAN = ("shift", 2, 256)
PATTERN = 0x7FC0BEEF          # the guard pattern of tests/test_gpu_lm_step.py


# ------------------------------------------------------------------------------------------------ the case table
# Shapes as L x H, B, T, C, U.  `plan`: what ops.lstm_plan(ws, head=(C, U)) must answer on an MI355X -- the keys that define the
# variant; the GPU test asserts it before anything runs.  extras: "accumulate" (dK, db start non-zero, dz0 with garbage), "dropout"
# (keep 0.8 / 0.7), "prefix" (the run is ws.prefix(T) of an allocation and a CTC workspace of alloc_T frames), "second" (a first
# mini-batch of first_T frames runs on the same workspace with training=True; the case is the second, shorter one).  state: h0 / c0
# drawn at 0.3 sigma.
def _case(name, L, H, B, T, C, U, covers, mv=0, w=0, precision=0, regime="nominal", extras=(), labels="standard", alloc_T=None,
          first_T=None, nfw=4, state=False):
    nmt = (B + 15) // 16
    plan = dict(fwd_path="flow", bwd_path="flow", kb=H // 128, nmt=nmt, mv=mv, nfw=nfw, w_pieces=w)
    return dict(name=name, L=L, H=H, B=B, T=T, C=C, U=U, covers=tuple(covers), plan=plan, precision=precision, regime=regime,
                extras=tuple(extras), labels=labels, alloc_T=alloc_T or first_T or T, first_T=first_T, state=state)


CASES = [
    _case("c16-1x128", 1, 128, 5, 17, 16, 4, ["C16", "kb1"]),
    _case("c48-2x256-b17", 2, 256, 17, 33, 48, 12, ["C48", "kb2", "ragged-tile"]),
    _case("c32-1x128", 1, 128, 6, 18, 32, 5, ["C32"]),
    _case("c64-2x128", 2, 128, 7, 19, 64, 6, ["C64"]),
    _case("h384-2x384", 2, 384, 20, 31, 80, 10, ["kb3", "C80"]),
    _case("h512-xw-upt2-cap", 3, 512, 32, 48, 80, 12, ["kb4-xw", "upt2-cap"], mv=1),
    _case("upt2-unreal", 1, 128, 47, 20, 80, 6, ["upt2-unreal"]),
    _case("upt1-b40", 1, 128, 40, 20, 80, 6, ["upt1-edge"]),
    _case("upt2-b41", 1, 128, 41, 20, 80, 6, ["upt2-edge"]),
    _case("waves4", 1, 128, 3, 160, 80, 150, ["waves4", "w8"], w=8, labels="waves"),
    _case("t1", 2, 128, 3, 1, 80, 4, ["T1"], state=True),      # (from a zero state one frame leaves the forget gate and dK's h half without a gradient)
    _case("t15", 2, 128, 3, 15, 80, 4, ["T15"]),
    _case("t16", 2, 128, 3, 16, 80, 4, ["T16"], state=True),
    _case("t17", 2, 128, 3, 17, 80, 4, ["T17"]),
    _case("w8-t64", 2, 256, 17, 64, 80, 20, ["w8", "T64"], w=8, extras=["accumulate"]),
    _case("w8-t65-h512", 3, 512, 15, 65, 80, 20, ["w8", "T65", "kb4-xw"], mv=1, w=8, extras=["accumulate"], state=True),
    _case("w0-t63", 2, 256, 17, 63, 80, 20, ["w0-T63"]),
    _case("bf16x3-h256", 2, 256, 17, 65, 80, 20, ["bf16x3"], w=8, precision=1),
    _case("bf16-h512", 1, 512, 16, 20, 80, 8, ["bf16"], precision=2),
    _case("dropout", 2, 256, 20, 33, 80, 12, ["dropout"], extras=["dropout"]),
    _case("prefix-23-of-40", 2, 128, 5, 23, 80, 8, ["prefix"], extras=["prefix"], alloc_T=40),
    _case("second-31-after-48", 3, 512, 32, 31, 80, 10, ["second-batch"], mv=1, extras=["second"], first_T=48),
    _case("saturating", 2, 256, 17, 20, 80, 8, ["saturating"], regime="saturating"),
]

# What the head's code can do differently from shape to shape, each with the rule it comes from.  The GPU test asserts that the
# table covers all of it and that the plan of every covering case has the property its name claims.
VARIANTS = {
    "C16": "ctc_head_nfw: the smallest C; one label tile, ctc_pack_wo_kernel zero-fills tiles 1..4, the leader's K loop runs once",
    "C32": "C = 32: two label tiles", "C48": "C = 48: not a power of two, three label tiles", "C64": "C = 64: four label tiles",
    "C80": "C = 80 = 16 CF_NTC: no zero-filled tile",
    "kb1": "ctc_follower<128, .> / ctc_leader<128>: two K blocks per wave, one 16-unit tile of dZ_top per wave",
    "kb2": "H = 256", "kb3": "H = 384: six K blocks per wave (f32 only on the dataflow kernels)",
    "kb4-xw": "H = 512 in f32: x-product workers (mv = 1) on the spare XCDs beside the followers",
    "upt2-cap": "ctc_follower_call: B > 2 followers -> UPT = 2, at the cap of ctc_head_nfw (B = 4 x followers)",
    "upt2-unreal": "UPT = 2 with unreal second utterances (u.real == false, clamped to B - 1) in the last teams",
    "upt1-edge": "B = 2 x followers exactly: UPT = 1", "upt2-edge": "B = 2 x followers + 1: UPT = 2, one real second utterance",
    "ragged-tile": "a second batch tile that holds row 16 alone",
    "waves4": "S >= 289: all four waves of the recursion live; repeats on states 97 / 193 / 289",
    "T1": "one frame: one chunk, no refresh", "T15": "T = 15: a short single chunk", "T16": "T = 16: one whole chunk",
    "T17": "T = 17: a second chunk of one frame (the clamp to T - 1)",
    "w8": "lstm_plan: T >= 64 with a spare XCD -> w_pieces = 8, and with a head the workers are DEALT (w_deal)",
    "T64": "T = 64: the smallest T with in-kernel weight-gradient workers", "T65": "T = 65: a fifth chunk of one frame, with workers",
    "w0-T63": "T = 63: a head without in-kernel weight-gradient workers (w_pieces = 0)",
    "bf16x3": "flow_*_kernel<true>(kb, 1): the bf16x3 dataflow kernels with a head; worker share percent / 2 - 1",
    "bf16": "flow_*_kernel<true>(kb, 2): the bf16 dataflow kernels with a head",
    "dropout": "keep 0.8 / 0.7: the follower reads the MASKED output of the top layer",
    "prefix": "the head on ws.prefix(T_run) of a longer allocation and CTC workspace",
    "second-batch": "two mini-batches in a row with training=True, the second shorter: armed panels, the sentinel under dZ_top re-filled",
    "saturating": "regime saturating (lstm_stack_ref SAT_*)",
}

# the refusals: (what, L, H, B, T, C, U).  lstm_ctc_fusable answers false, lstm_fwd(..., head=) raises and writes nothing.
REFUSALS = [("C = 24", 1, 128, 5, 17, 24, 4), ("C = 96", 1, 128, 5, 17, 96, 4), ("2 U + 1 = 385", 1, 128, 3, 20, 80, 192),
            ("L * nmt = 8", 2, 128, 64, 17, 80, 4), ("B above four per follower", 1, 128, 100, 17, 80, 4)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def teams(case, plan=None):
    """Follower teams of the forward launch: two per follower workgroup, nfw workgroups on each XCD without a recurrence group."""
    plan = plan or case["plan"]
    return 2 * (8 - case["L"] * plan["nmt"]) * plan["nfw"]


def upt(case, plan=None):
    """ctc_follower_call: B > 2 (8 - L nmt) nfw gives two utterances per team."""
    return 2 if case["B"] > teams(case, plan) else 1


def stack_case(case, T=None):
    """The case as lstm_stack_ref sees it (its make_inputs, cpu_masks, reference and CAPS)."""
    return dict(name=case["name"], T=T or case["T"], B=case["B"], H=case["H"], L=case["L"], precision=case["precision"], lens="full",
                regime=case["regime"], state=case["state"], extras=tuple(e for e in case["extras"] if e in ("accumulate", "dropout")))


# ------------------------------------------------------------------------------------------------ inputs
def make_batch(case, T=None):
    """lengths [B] and dense labels [B,U].  Every label row fits its frames (labels + repeats <= frames, the EOS too where there is
    one).  B > 3 carries the four special rows of tests/test_gpu_ctc_head.py's make_batch: row 0 full length, row 1 padded
    (lengths == 0), row 2 an empty label row, row 3 an over-long target (the one row that does NOT fit)."""
    T = T or case["T"]
    B, C, U = case["B"], case["C"], case["U"]
    rng = np.random.RandomState(sum(map(ord, case["name"])) + 31 * T)
    dense = np.zeros((B, U), np.int32)
    if case["labels"] == "waves":      # every label slot used (S = 2 U + 1), one repeat per row on a wave boundary of the recursion
        lengths = np.array([T - (0, 1, 3)[b % 3] for b in range(B)], np.int32)
        for b in range(B):
            dense[b] = CR._labels(rng, U, C, ((97, 193, 289)[b % 3],))
        return lengths, dense
    lengths = rng.randint(max(1, (T + 1) // 2), T + 1, size=B).astype(np.int32)
    lengths[0] = T
    for b in range(B):
        n = rng.randint(1, min(U, max(1, int(lengths[b]) // 2)) + 1)
        dense[b, :n] = CR._labels(rng, n, C, ())
        if n < U and n + 1 <= lengths[b]:
            dense[b, n] = C - 1
    if B > 3:
        lengths[1] = 0
        dense[2, :] = 0
        dense[3, :] = 0
        dense[3, :U - 1] = 5
        lengths[3] = max(1, min(T, (U - 1) // 2))
    return lengths, dense


def row_facts(dense, lengths, C):
    """Per row: (valid, required frames, labels + repeats).  valid: lengths > 0 and the raw label count fits (the oracle's rule)."""
    out = []
    for b, raw in enumerate(CR.om.sparsify_labels(dense, C)):
        tgt, required = CR.om.ctc_targets(raw, C)
        nrep = sum(1 for u in range(1, len(tgt)) if tgt[u] == tgt[u - 1])
        out.append((bool(lengths[b] > 0 and required <= lengths[b]), required, len(tgt) + nrep))
    return out


def make_inputs(case, T=None):
    """Everything a case feeds the two calls, as float32 CPU tensors / numpy arrays: lstm_stack_ref.make_inputs for the stack (z0 zero
    past the rows' lengths), W_o [H,C], b_o [C], lengths, dense labels."""
    T = T or case["T"]
    name = case["name"] if T == case["T"] else case["name"] + "-first"
    inp = S.make_inputs(stack_case(dict(case, name=name), T))
    lengths, dense = make_batch(case, T)
    dead = torch.as_tensor(np.arange(T)[:, None] >= lengths[None, :])
    inp["z0"][dead] = 0.0
    del inp["dztop"]
    g = torch.Generator(device="cpu").manual_seed(sum(map(ord, name)) + 7)
    # logits of a standard deviation around 1 on top-layer outputs of 0.1 .. 0.5; a bias in every class: no logits slice is empty
    wo = torch.randn(case["H"], case["C"], generator=g) * (4.0 / np.sqrt(case["H"]))
    bo = torch.randn(case["C"], generator=g) * 0.5
    bo = torch.where(bo.abs() < 0.05, torch.full_like(bo, 0.05), bo)
    inp.update(lengths=lengths, dead=dead, dense=dense, wo=wo, bo=bo, T=T)
    return inp


# ------------------------------------------------------------------------------------------------ the two matrix products
def linear_ref(ztop, wo, bo):
    """float64 ztop [T,B,H] . W_o [H,C] + b_o."""
    return np.asarray(ztop, F64) @ np.asarray(wo, F64) + np.asarray(bo, F64)


def dztop_ref(dlogits, wo):
    """float64 dlogits [T,B,C] . W_o^T [C,H]."""
    return np.asarray(dlogits, F64) @ np.asarray(wo, F64).T


LINEAR_FAULTS = ("drop_k", "second_tile", "clamp_last")
DZTOP_FAULTS = ("neighbour_tile", "ignore_64")


def emulate_linear(ztop, wo, bo, fault=None, nteams=None):
    """ctc_follower's logits in float32 in its order: wave w multiplies the K slice [H/4 w, H/4 w + H/4), the four partial sums meet
    as ((p0 + p1) + p2) + p3 + b_o.  fault (the proof that the slices have teeth):
      "drop_k"       wave 2 drops its last K block of 16
      "second_tile"  the second utterance of a UPT-2 team (b = team + nteams) gets the first one's label tile 0
      "clamp_last"   the last frame of every chunk is taken from frame T - 1 (the probe's clamp) when T % 16 != 0"""
    z, w, b = np.asarray(ztop, F32), np.asarray(wo, F32), np.asarray(bo, F32)
    T, B, H = z.shape
    if fault == "clamp_last" and T % 16 != 0:
        z = z.copy()
        z[15::16] = z[T - 1]
    q = H // 4
    parts = []
    for k in range(4):
        hi = q * (k + 1) - (16 if fault == "drop_k" and k == 2 else 0)
        parts.append(z[:, :, q * k:hi] @ w[q * k:hi])
    out = (((parts[0] + parts[1]) + parts[2]) + parts[3]) + b
    if fault == "second_tile":
        assert nteams is not None and B > nteams
        out[:, nteams:B, :16] = out[:, :B - nteams, :16]
    return out


def emulate_dztop(dlogits, wo, fault=None):
    """ctc_leader's dZ_top in float32 in its order: K blocks of 16 labels accumulated one after the other.  fault:
      "neighbour_tile"  utterance 0's units 16:32 are computed from W_o's rows 0:16
      "ignore_64"       label columns >= 64 are left out"""
    d, w = np.asarray(dlogits, F32), np.asarray(wo, F32)
    C = d.shape[2]
    acc = np.zeros(d.shape[:2] + (w.shape[0],), F32)
    for k0 in range(0, min(C, 64) if fault == "ignore_64" else C, 16):
        acc = acc + d[:, :, k0:k0 + 16] @ w[:, k0:k0 + 16].T
    if fault == "neighbour_tile":
        acc[:, 0, 16:32] = acc[:, 0, 0:16]
    return acc


def _chunks(T):
    return [(t0, min(t0 + 16, T)) for t0 in range(0, T, 16)]


def linear_slice_errors(got, ref, lengths):
    """(label, error, slice maximum / tensor maximum) per (utterance, 16-frame chunk, 16-label tile) that holds a valid frame; the
    error is the largest difference over the slice's valid frames by max(the slice's largest |reference|, 1)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    T, B, C = ref.shape
    whole = np.abs(ref).max() + 1e-300
    out = []
    for b in range(B):
        for t0, t1 in _chunks(min(int(lengths[b]), T)):
            for c0 in range(0, C, 16):
                r, g = ref[t0:t1, b, c0:c0 + 16], got[t0:t1, b, c0:c0 + 16]
                top = np.abs(r).max()
                e = np.abs(g - r).max()
                out.append(("row %d frames %d:%d labels %d:%d" % (b, t0, t1, c0, c0 + 16), float(np.inf if np.isnan(e) else e / max(top, 1.0)),
                            top / whole))
    return out


def dztop_slice_errors(got, ref, dlogits, wo, lengths, valid):
    """(label, error, slice maximum / tensor maximum) per (utterance, 16-frame chunk, 16-unit tile) that holds a valid frame of a
    valid row; the error is the largest difference by the slice's largest sum_c |dlogits| |W_o| (what the float32 roundings of the
    product scale with)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    T, B, H = ref.shape
    mag = np.abs(np.asarray(dlogits, F64)) @ np.abs(np.asarray(wo, F64)).T
    whole = np.abs(ref).max() + 1e-300
    out = []
    for b in range(B):
        if not valid[b]:
            continue
        for t0, t1 in _chunks(min(int(lengths[b]), T)):
            for u0 in range(0, H, 16):
                r, g = ref[t0:t1, b, u0:u0 + 16], got[t0:t1, b, u0:u0 + 16]
                e = np.abs(g - r).max()
                out.append(("row %d frames %d:%d units %d:%d" % (b, t0, t1, u0, u0 + 16),
                            float(np.inf if np.isnan(e) else e / (mag[t0:t1, b, u0:u0 + 16].max() + 1e-300)), np.abs(r).max() / whole))
    return out


def no_gradient_mask(T, lengths, valid):
    """[T,B] True where dlogits and dZ_top must be exactly zero: rows without a gradient, frames at and past a row's length."""
    lens = np.where(np.asarray(valid), np.minimum(lengths, T), 0)
    return np.arange(T)[:, None] >= lens[None, :]


# ------------------------------------------------------------------------------------------------ the bounds
# (regime, precision) -> {kind: largest per-slice error of the emulated arithmetic}; H -> stage 2; C -> stage 4: the recorded run
MEASURED = {
    ('flow+head', 'nominal', 0): {'ztop': 7.3e-07, 'h': 9.5e-07, 'hT': 6.4e-07, 'cT': 4.6e-07, 'dK': 9.1e-07, 'db': 1.0e-06, 'dz0': 1.2e-06},
    ('flow+head', 'nominal', 1): {'ztop': 5.9e-06, 'h': 9.4e-06, 'hT': 6.6e-06, 'cT': 4.1e-06, 'dK': 5.9e-06, 'db': 8.7e-06, 'dz0': 1.0e-05},
    ('flow+head', 'nominal', 2): {'ztop': 7.6e-03, 'h': 7.6e-03, 'hT': 3.9e-03, 'cT': 3.0e-03, 'dK': 4.5e-03, 'db': 4.2e-03, 'dz0': 5.1e-03},
    ('flow+head', 'saturating', 0): {'ztop': 8.4e-06, 'h': 8.4e-06, 'hT': 8.4e-06, 'cT': 1.5e-06, 'dK': 5.7e-06, 'db': 1.4e-05, 'dz0': 9.1e-06},
}
LINEAR_MEASURED = {128: 2.7e-07, 256: 4.4e-07, 384: 3.5e-07, 512: 5.3e-07}
DZTOP_MEASURED = {16: 2.2e-07, 32: 1.1e-07, 48: 1.8e-07, 64: 2.4e-07, 80: 4.3e-07}


def bound(case, kind):
    """Stages 1 and 5: lstm_stack_ref.bound's form on this file's rows."""
    cap = S.CAPS[case["precision"]][0 if kind in S.OUTPUT_KINDS else 1]
    return min(cap, FACTOR * MEASURED[(FAMILY, case["regime"], case["precision"])][kind])


def linear_bound(case):
    return min(LOGIT_CAP, FACTOR * LINEAR_MEASURED[case["H"]])


def dztop_bound(case):
    return min(DZTOP_CAP, FACTOR * DZTOP_MEASURED[case["C"]])


# ------------------------------------------------------------------------------------------------ the judge
def _worst(errs, lim, what, fails, check_floor=True):
    e, lab = max((x[1], x[0]) for x in errs)
    if check_floor:
        lab_f, _, frac = min(errs, key=lambda x: x[2])
        if frac < FLOOR:
            fails.append("%s: slice %s has %.1e of the tensor's maximum: the inputs must not produce one" % (what, lab_f, frac))
    if not e <= lim:
        bad = sorted(((x[1], x[0]) for x in errs if not x[1] <= lim), reverse=True)
        fails.append("%s: %d of %d slices over %.1e, worst %s" % (what, len(bad), len(errs), lim, "; ".join("%.2e %s" % x for x in bad[:5])))
    return e / lim, lab


def judge(case, inp, got, in_mult=None, out_mult=None):
    """Every stage of a result `got` (ztop, h, hT, cT, logits, loss, dlogits, dztop, dK, db, dz0: float32 arrays or tensors) against
    float64 on the stage's own input.  -> (failures, {stage: worst error / bound}, lines for the log)."""
    T, B, C = inp["T"], case["B"], case["C"]
    lengths, dense, wo, bo = inp["lengths"], inp["dense"], inp["wo"].numpy(), inp["bo"].numpy()
    fails, ratios, lines = [], {}, []
    np_ = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    # ---- 1: the stack's forward pass
    f = S.forward(inp["z0"], inp["k"], inp["b"], lengths, inp["h0"], inp["c0"], in_mult, out_mult)
    r1 = 0.0
    for kind in S.OUTPUT_KINDS:
        ratio, lab = _worst(S.slice_errors(got[kind], f[kind], kind, lengths), bound(case, kind), "stage 1 " + kind, fails)
        lines.append("1 %-7s %.3f of its bound  %s" % (kind, ratio, lab))
        r1 = max(r1, ratio)
    if not S.padding_is_zero(got["ztop"], lengths):
        fails.append("stage 1: ztop is not exactly zero at and past the rows' lengths")
    ratios[1] = r1
    # ---- 2: the output Linear on the GPU's own ztop
    logits = np_(got["logits"])
    ref2 = linear_ref(np_(got["ztop"]), wo, bo)
    errs = linear_slice_errors(logits, ref2, lengths)
    ratios[2], lab = _worst(errs, linear_bound(case), "stage 2 logits", fails) if errs else (0.0, "")
    lines.append("2 logits  %.3f of its bound  %s" % (ratios[2], lab))
    past = np.arange(T)[:, None] >= lengths[None, :]
    if not np.array_equal(logits[past].view(np.int32), np.broadcast_to(bo.astype(F32), logits.shape)[past].view(np.int32)):
        fails.append("stage 2: logits at and past a row's length are not b_o bit for bit")
    # ---- 3: the CTC loss and gradient on the GPU's own logits
    facts = row_facts(dense, lengths, C)
    valid, inf = [v for v, _, _ in facts], [False] * B
    ref_loss, ref_d = CR.reference(logits, dense, lengths)
    with np.errstate(all="ignore"):
        emu_loss, emu_d = CR.emulate(logits, dense, lengths, HEAD_PLAN, fam="head")
    ev = dict(ref_loss=ref_loss, ref_d=ref_d, lengths=lengths, valid=valid, inf=inf, case=dict(C=C),
              emu_err=CR.slice_errors(emu_loss, emu_d, ref_loss, ref_d, lengths),
              emu_rowsum=CR.invariants(emu_loss, emu_d, lengths, valid, inf)[0])
    ev["bounds"] = CR.bounds(ev["emu_err"], "head", ref_d)
    dlogits = np_(got["dlogits"])
    f3, ratios[3] = CR.judge(ev, np_(got["loss"]), dlogits)
    fails += ["stage 3 " + x for x in f3[:8]]
    e3 = CR.slice_errors(np_(got["loss"]), dlogits, ref_loss, ref_d, lengths)
    key = max(e3, key=lambda k: e3[k] / ev["bounds"][k])
    lines.append("3 ctc     %.3f of its bound  (worst slice %s: %.2e of %.2e)" % (ratios[3], key, e3[key], ev["bounds"][key]))
    zero = no_gradient_mask(T, lengths, valid)
    if dlogits[zero].any():
        fails.append("stage 3: dlogits is not exactly zero on rows without a gradient / past the lengths")
    # ---- 4: dZ_top on the GPU's own dlogits
    dztop = np_(got["dztop"])
    ref4 = dztop_ref(dlogits, wo)
    errs = dztop_slice_errors(dztop, ref4, dlogits, wo, lengths, valid)
    ratios[4], lab = _worst(errs, dztop_bound(case), "stage 4 dztop", fails)
    lines.append("4 dztop   %.3f of its bound  %s" % (ratios[4], lab))
    if dztop[zero].any():
        fails.append("stage 4: dZ_top is not exactly zero on rows without a gradient / past the lengths")
    # ---- 5: BPTT from the float64 product of stage 4
    r5 = S.backward(f["cache"], torch.as_tensor(ref4))
    if inp["dk0"] is not None:
        r5["dK"], r5["db"] = r5["dK"] + inp["dk0"].double(), r5["db"] + inp["db0"].double()
    worst5 = 0.0
    for kind in S.GRAD_KINDS:
        ratio, lab = _worst(S.slice_errors(got[kind], r5[kind], kind, lengths), bound(case, kind), "stage 5 " + kind, fails)
        lines.append("5 %-7s %.3f of its bound  %s" % (kind, ratio, lab))
        worst5 = max(worst5, ratio)
    if not S.padding_is_zero(got["dz0"], lengths):
        fails.append("stage 5: dz0 is not exactly zero at and past the rows' lengths")
    ratios[5] = worst5
    return fails, ratios, lines


# ------------------------------------------------------------------------------------------------ the emulated result, on the CPU
@functools.lru_cache(maxsize=None)
def emulated(name):
    """(inp, masks, got) of a case with every stage in the emulated arithmetic of its precision -- what the tables are measured on
    and what the CPU tests judge.  Each stage runs on the previous stage's emulated output, as the kernels do."""
    case = by_name(name)
    inp = make_inputs(case)
    sc = stack_case(case)
    im, om = S.cpu_masks(sc)
    f = S.forward(inp["z0"], inp["k"], inp["b"], inp["lengths"], inp["h0"], inp["c0"], im, om, S.emulation(sc))
    got = {k: f[k].numpy() for k in S.OUTPUT_KINDS}
    got["logits"] = emulate_linear(got["ztop"], inp["wo"], inp["bo"])
    with np.errstate(all="ignore"):
        got["loss"], got["dlogits"] = CR.emulate(got["logits"], inp["dense"], inp["lengths"], HEAD_PLAN, fam="head")
    got["dztop"] = emulate_dztop(got["dlogits"], inp["wo"])
    r = S.backward(f["cache"], torch.as_tensor(got["dztop"]))
    if inp["dk0"] is not None:
        r["dK"], r["db"] = r["dK"] + inp["dk0"], r["db"] + inp["db0"]
    got.update({k: r[k].numpy() for k in S.GRAD_KINDS})
    return inp, (im, om), got


@functools.lru_cache(maxsize=None)
def reference_chain(name):
    """The five stages by the float64 reference alone (each on the stage before it, the logits and dlogits stored as float32 as the
    kernels store them): what the floor check of tests/test_cpu_ctc_head_ref.py looks at.  -> (inp, dict of every tensor)."""
    case = by_name(name)
    inp = make_inputs(case)
    im, om = S.cpu_masks(stack_case(case))
    f = S.forward(inp["z0"], inp["k"], inp["b"], inp["lengths"], inp["h0"], inp["c0"], im, om)
    ref = {k: f[k].numpy() for k in S.OUTPUT_KINDS}
    ref["logits"] = linear_ref(ref["ztop"].astype(F32), inp["wo"], inp["bo"]).astype(F32)
    loss, d = CR.reference(ref["logits"], inp["dense"], inp["lengths"])
    ref["loss"], ref["dlogits"] = loss, d.astype(F32)
    ref["dztop"] = dztop_ref(ref["dlogits"], inp["wo"])
    r = S.backward(f["cache"], torch.as_tensor(ref["dztop"]))
    ref.update({k: r[k].numpy() for k in S.GRAD_KINDS})
    return inp, ref


def measure(cases=CASES, verbose=False):
    """-> (MEASURED, LINEAR_MEASURED, DZTOP_MEASURED) of the emulated results of `cases` against float64."""
    table, lin, dzt = {}, {}, {}
    for case in cases:
        inp, (im, om), got = emulated(case["name"])
        lengths = inp["lengths"]
        f = S.forward(inp["z0"], inp["k"], inp["b"], lengths, inp["h0"], inp["c0"], im, om)
        row = table.setdefault((FAMILY, case["regime"], case["precision"]), {k: 0.0 for k in S.OUTPUT_KINDS + S.GRAD_KINDS})
        for kind in S.OUTPUT_KINDS:
            row[kind] = max(row[kind], max(x[1] for x in S.slice_errors(got[kind], f[kind], kind, lengths)))
        e2 = max(x[1] for x in linear_slice_errors(got["logits"], linear_ref(got["ztop"], inp["wo"], inp["bo"]), lengths))
        lin[case["H"]] = max(lin.get(case["H"], 0.0), e2)
        valid = [v for v, _, _ in row_facts(inp["dense"], lengths, case["C"])]
        ref4 = dztop_ref(got["dlogits"], inp["wo"])
        e4 = max(x[1] for x in dztop_slice_errors(got["dztop"], ref4, got["dlogits"], inp["wo"], lengths, valid))
        dzt[case["C"]] = max(dzt.get(case["C"], 0.0), e4)
        r5 = S.backward(f["cache"], torch.as_tensor(ref4))
        if inp["dk0"] is not None:
            r5["dK"], r5["db"] = r5["dK"] + inp["dk0"].double(), r5["db"] + inp["db0"].double()
        for kind in S.GRAD_KINDS:
            row[kind] = max(row[kind], max(x[1] for x in S.slice_errors(got[kind], r5[kind], kind, lengths)))
        if verbose:
            print("  %-20s linear %.1e dztop %.1e" % (case["name"], e2, e4), flush=True)
    return table, lin, dzt


if __name__ == "__main__":
    import time
    t0 = time.time()
    table, lin, dzt = measure(verbose=True)
    names = S.OUTPUT_KINDS + S.GRAD_KINDS
    print("\nMEASURED = {")
    for key in sorted(table):
        print("    %r: {%s}," % (key, ", ".join("%r: %.1e" % (k, table[key][k]) for k in names)))
    print("}")
    print("LINEAR_MEASURED = {%s}" % ", ".join("%d: %.1e" % (h, lin[h]) for h in sorted(lin)))
    print("DZTOP_MEASURED = {%s}\n" % ", ".join("%d: %.1e" % (c, dzt[c]) for c in sorted(dzt)))
    print("%-10s pr | %s" % ("regime", " | ".join("%-15s" % k for k in names)))
    for key in sorted(table):
        cells = []
        for k in names:
            cap = S.CAPS[key[2]][0 if k in S.OUTPUT_KINDS else 1]
            cells.append("%.1e>%.1e%s" % (table[key][k], min(cap, FACTOR * table[key][k]), "c" if FACTOR * table[key][k] > cap else " "))
        print("%-10s %d  | %s" % (key[1], key[2], " | ".join(cells)))
    print("stage 2 (by H, of max(|slice|, 1); cap %.0e): %s" % (LOGIT_CAP, "  ".join("%d: %.1e>%.1e" % (h, lin[h], min(LOGIT_CAP, FACTOR * lin[h])) for h in sorted(lin))))
    print("stage 4 (by C, of the slice's sum |dlogits| |W_o|; cap %.1e): %s" % (DZTOP_CAP, "  ".join("%d: %.1e>%.1e" % (c, dzt[c], min(DZTOP_CAP, FACTOR * dzt[c])) for c in sorted(dzt))))
    print("(measured > bound; c: bound is the cap)   %.0f s" % (time.time() - t0))
