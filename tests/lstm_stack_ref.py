"""float64 reference of the unidirectional LSTM stack as ops.lstm_fwd / ops.lstm_bwd state it (include/amdspeech.h, "LSTM
stack"), the slice metric the GPU matrix is judged by, and the matrix itself.  Checker only: plain torch, no GPU, nothing of the
product is imported.

The cell is TF's BasicLSTMCell under dynamic_rnn: kernel [2H, 4H] (rows: x then h; columns: i | j | f | o blocks of H),
forget bias 1.0 added at run time, c' = sigmoid(f + 1) c + sigmoid(i) tanh(j), h' = sigmoid(o) tanh(c'); a frame at or past a
row's length emits 0 and copies the state through.  Dropout: layer l's input is multiplied by in_mult[l], its output by
out_mult[l] ([T,B,H] multipliers, mask / keep); the state is never masked.  The backward pass is written out by hand (not
autograd) so that it can be run in float32 and with rounded matrix operands, product by product, in the same order.

Tolerances.  The bound of a slice kind is 8 x the largest error the SAME arithmetic shows on the CPU against float64, slice by
slice, in the arithmetic of the precision under test (`emulate`: float32; operands cut to 16 significant bits -- bf16 hi + bf16 lo
-- before each product; operands rounded to bf16), taken over every case of a (precision, regime) family, and never looser than
the suite's whole-tensor figures applied per slice (CAPS).  The factor 8 covers MFMA accumulation order, K-split partial sums and
the hardware's exp / rcp.  `python tests/lstm_stack_ref.py` (CPU only, ~1 min) measures the table; the figures below are that run.
A (precision, regime, kind) whose 8 x measured error exceeds the cap is bound by the cap: the arithmetic of that precision itself
may then sit near the bound, which is a statement about the precision, recorded here and not tuned on the GPU.

MEASURED (largest per-slice relative error of the emulated arithmetic against float64; bound = min(cap, 8 x measured)):

family        regime     pr | ztop            | h               | hT              | cT              | dK              | db              | dz0
big           nominal    0  | 9.5e-07>7.6e-06  | 1.0e-06>8.2e-06  | 5.9e-07>4.7e-06  | 4.4e-07>3.5e-06  | 7.5e-07>6.0e-06  | 9.2e-07>7.3e-06  | 8.9e-07>7.1e-06
big           nominal    2  | 6.5e-03>1.0e-02c | 7.9e-03>1.0e-02c | 4.3e-03>1.0e-02c | 3.6e-03>1.0e-02c | 6.7e-03>3.0e-02c | 1.2e-02>3.0e-02c | 7.4e-03>3.0e-02c
big           saturating 1  | 6.3e-05>2.0e-04c | 6.3e-05>2.0e-04c | 4.7e-05>2.0e-04c | 2.2e-05>1.8e-04  | 3.7e-05>3.0e-04  | 1.1e-04>8.6e-04  | 5.6e-05>4.5e-04
diag          nominal    0  | 9.8e-07>7.8e-06  | 9.8e-07>7.8e-06  | 4.9e-07>3.9e-06  | 4.2e-07>3.4e-06  | 7.1e-07>5.7e-06  | 8.6e-07>6.8e-06  | 1.1e-06>8.9e-06
diag          saturating 0  | 1.2e-05>9.5e-05  | 1.2e-05>9.5e-05  | 1.1e-05>9.1e-05  | 3.6e-06>2.9e-05  | 1.4e-05>1.1e-04  | 2.5e-05>2.0e-04  | 2.1e-05>1.7e-04
diag_bf3      nominal    1  | 8.4e-06>6.7e-05  | 8.8e-06>7.0e-05  | 7.1e-06>5.7e-05  | 5.0e-06>4.0e-05  | 8.1e-06>6.4e-05  | 1.5e-05>1.2e-04  | 9.4e-06>7.5e-05
diag_bf3      nominal    2  | 4.3e-03>1.0e-02c | 6.9e-03>1.0e-02c | 3.6e-03>1.0e-02c | 3.0e-03>1.0e-02c | 5.5e-03>3.0e-02c | 6.8e-03>3.0e-02c | 7.3e-03>3.0e-02c
diag_bf3      saturating 1  | 5.1e-05>2.0e-04c | 5.1e-05>2.0e-04c | 3.8e-05>2.0e-04c | 1.5e-05>1.2e-04  | 3.8e-05>3.0e-04  | 7.0e-05>5.6e-04  | 6.7e-05>5.4e-04
flow          nominal    0  | 5.2e-07>4.2e-06  | 9.2e-07>7.4e-06  | 6.4e-07>5.1e-06  | 4.3e-07>3.4e-06  | 7.7e-07>6.1e-06  | 1.1e-06>9.2e-06  | 1.4e-06>1.2e-05
flow          saturating 0  | 5.8e-06>4.6e-05  | 5.8e-06>4.6e-05  | 5.0e-06>4.0e-05  | 1.5e-06>1.2e-05  | 4.7e-06>3.7e-05  | 9.5e-06>7.6e-05  | 8.3e-06>6.6e-05
flow-reduced  nominal    1  | 6.2e-06>4.9e-05  | 9.4e-06>7.6e-05  | 6.9e-06>5.5e-05  | 6.0e-06>4.8e-05  | 7.9e-06>6.3e-05  | 9.8e-06>7.8e-05  | 8.7e-06>6.9e-05
flow-reduced  nominal    2  | 6.6e-03>1.0e-02c | 7.5e-03>1.0e-02c | 5.2e-03>1.0e-02c | 3.5e-03>1.0e-02c | 5.8e-03>3.0e-02c | 6.1e-03>3.0e-02c | 6.6e-03>3.0e-02c
flow-reduced  saturating 1  | 5.3e-05>2.0e-04c | 6.4e-05>2.0e-04c | 4.8e-05>2.0e-04c | 1.0e-05>8.3e-05  | 4.3e-05>3.5e-04  | 1.1e-04>8.4e-04  | 5.7e-05>4.5e-04
hoist         nominal    0  | 1.3e-06>1.1e-05  | 1.5e-06>1.2e-05  | 7.0e-07>5.6e-06  | 5.8e-07>4.7e-06  | 7.1e-07>5.7e-06  | 1.1e-06>8.9e-06  | 1.1e-06>8.9e-06
hoist         saturating 0  | 6.2e-06>4.9e-05  | 6.2e-06>4.9e-05  | 4.8e-06>3.9e-05  | 1.5e-06>1.2e-05  | 3.9e-06>3.2e-05  | 5.4e-06>4.3e-05  | 4.8e-06>3.9e-05
(measured>bound; c: the bound is the cap)
"""
import numpy as np
import torch

FORGET_BIAS = 1.0
FLOOR = 1e-6            # a slice is left out only if its reference maximum is below FLOOR x the tensor's maximum
FACTOR = 8.0
# today's whole-tensor tolerances (tests/test_gpu_model.py), applied per slice: (outputs and state, gradients)
CAPS = {0: (1e-4, 2e-3), 1: (2e-4, 5e-3), 2: (1e-2, 3e-2)}
OUTPUT_KINDS = ("ztop", "h", "hT", "cT")
GRAD_KINDS = ("dK", "db", "dz0")


# ------------------------------------------------------------------------------------------------ operand rounding
def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _cut16(x):
    hi = _bf16(x)
    return hi + _bf16(x - hi)


def _operand_fn(emulate):
    return {None: None, "f32": None, "bf16x3": _cut16, "bf16": _bf16}[emulate]


def _mm(a, b, rnd):
    return a @ b if rnd is None else rnd(a) @ rnd(b)


# ------------------------------------------------------------------------------------------------ the reference
def forward(z0, kernels, biases, lengths, h0=None, c0=None, in_mult=None, out_mult=None, emulate=None):
    """z0 [T,B,H], kernels [L,2H,4H], biases [L,4H], lengths [B], h0/c0 [L,B,H] or None, in_mult/out_mult: lists of L [T,B,H]
    multipliers (or None).  emulate None: float64; "f32" / "bf16x3" / "bf16": the same op order in float32, the operands of every
    matrix product rounded as the precision does.  Returns a dict: ztop [T,B,H], h [L,T,B,H] (the state after every frame: the
    cell's output on valid frames, carried through past a row's length), hT / cT [L,B,H], and `cache` for backward()."""
    dt = torch.float64 if emulate is None else torch.float32
    rnd = _operand_fn(emulate)
    z0, kernels, biases = (torch.as_tensor(a).to(dt) for a in (z0, kernels, biases))
    T, B, H = z0.shape
    L = kernels.shape[0]
    lengths = torch.as_tensor(np.asarray(lengths)).to(torch.int64)
    cur = z0
    layers, hs, hT, cT = [], [], [], []
    for l in range(L):
        K, bias = kernels[l], biases[l]
        h = torch.zeros(B, H, dtype=dt) if h0 is None else torch.as_tensor(h0[l]).to(dt).clone()
        c = torch.zeros(B, H, dtype=dt) if c0 is None else torch.as_tensor(c0[l]).to(dt).clone()
        xin = cur if in_mult is None or in_mult[l] is None else cur * torch.as_tensor(in_mult[l]).to(dt)
        out = torch.zeros(T, B, H, dtype=dt)
        st = {k: torch.zeros(T, B, H, dtype=dt) for k in ("i", "j", "f", "o", "c", "hprev", "cprev", "hstate")}
        for t in range(T):
            live = (t < lengths).view(B, 1)
            g = _mm(torch.cat([xin[t], h], dim=1), K, rnd) + bias
            i, j = torch.sigmoid(g[:, :H]), torch.tanh(g[:, H:2 * H])
            f, o = torch.sigmoid(g[:, 2 * H:3 * H] + FORGET_BIAS), torch.sigmoid(g[:, 3 * H:])
            cn = c * f + i * j
            hn = torch.tanh(cn) * o
            st["hprev"][t], st["cprev"][t] = h, c
            st["i"][t], st["j"][t], st["f"][t], st["o"][t], st["c"][t] = i, j, f, o, cn
            out[t] = torch.where(live, hn, torch.zeros_like(hn))
            c = torch.where(live, cn, c)
            h = torch.where(live, hn, h)
            st["hstate"][t] = h
        st["xin"] = xin
        layers.append(st)
        hs.append(st["hstate"])
        hT.append(h)
        cT.append(c)
        cur = out if out_mult is None or out_mult[l] is None else out * torch.as_tensor(out_mult[l]).to(dt)
    cache = dict(layers=layers, kernels=kernels, lengths=lengths, in_mult=in_mult, out_mult=out_mult, emulate=emulate)
    return dict(ztop=cur, h=torch.stack(hs), hT=torch.stack(hT), cT=torch.stack(cT), cache=cache)


def backward(cache, dztop):
    """BPTT of forward() from dztop [T,B,H]: dict dK [L,2H,4H], db [L,4H], dz0 [T,B,H] (sums over the batch)."""
    kernels, lengths, emulate = cache["kernels"], cache["lengths"], cache["emulate"]
    dt = kernels.dtype
    rnd = _operand_fn(emulate)
    L, H = kernels.shape[0], kernels.shape[1] // 2
    dy = torch.as_tensor(dztop).to(dt)
    T, B, _ = dy.shape
    dK, db = torch.zeros_like(kernels), torch.zeros(L, 4 * H, dtype=dt)
    for l in range(L - 1, -1, -1):
        st, K = cache["layers"][l], kernels[l]
        if cache["out_mult"] is not None and cache["out_mult"][l] is not None:
            dy = dy * torch.as_tensor(cache["out_mult"][l]).to(dt)
        dg_all = torch.zeros(T, B, 4 * H, dtype=dt)
        dh, dc = torch.zeros(B, H, dtype=dt), torch.zeros(B, H, dtype=dt)
        for t in range(T - 1, -1, -1):
            live = (t < lengths).view(B, 1)
            i, j, f, o, c = st["i"][t], st["j"][t], st["f"][t], st["o"][t], st["c"][t]
            dh_tot = dh + dy[t]
            tc = torch.tanh(c)
            dc_tot = dc + dh_tot * o * (1.0 - tc * tc)
            dg = torch.cat([dc_tot * j * i * (1.0 - i), dc_tot * i * (1.0 - j * j),
                            dc_tot * st["cprev"][t] * f * (1.0 - f), dh_tot * tc * o * (1.0 - o)], dim=1)
            dg = torch.where(live, dg, torch.zeros_like(dg))
            dg_all[t] = dg
            dh = torch.where(live, _mm(dg, K[H:].t(), rnd), dh)
            dc = torch.where(live, dc_tot * f, dc)
        flat = dg_all.reshape(T * B, 4 * H)
        # the batched products, each over all frames at once (what the kernels hoist out of the recurrence)
        dx = _mm(flat, K[:H].t(), rnd).reshape(T, B, H)
        xh = torch.cat([st["xin"], st["hprev"]], dim=2).reshape(T * B, 2 * H)
        dK[l] = _mm(xh.t(), flat, rnd)
        db[l] = flat.sum(dim=0)
        if cache["in_mult"] is not None and cache["in_mult"][l] is not None:
            dx = dx * torch.as_tensor(cache["in_mult"][l]).to(dt)
        dy = dx
    return dict(dK=dK, db=db, dz0=dy)


def gate_values(z0, kernels, biases, lengths, h0=None, c0=None):
    """The activated gates of every valid frame (float64), tanh(j) mapped onto (0, 1): what the saturation check counts near 0 / 1."""
    res = forward(z0, kernels, biases, lengths, h0, c0)
    vals = []
    lengths = np.asarray(lengths)
    for st in res["cache"]["layers"]:
        T = st["i"].shape[0]
        live = torch.as_tensor(np.arange(T)[:, None] < lengths[None, :])
        vals.append(torch.cat([st["i"][live], st["f"][live], st["o"][live], (st["j"][live] + 1) / 2], dim=1))
    return torch.cat(vals)


# ------------------------------------------------------------------------------------------------ the slice metric
def _thirds(n):
    """The time axis 0..n-1 cut into (up to) three non-empty contiguous parts."""
    if n <= 0:
        return []
    k = min(3, n)
    edges = [round(i * n / k) for i in range(k + 1)]
    return [(edges[i], edges[i + 1]) for i in range(k) if edges[i + 1] > edges[i]]


def slices(kind, shape, lengths=None):
    """[(label, index)] of a tensor of `kind`: index selects the slice (a tuple of slices, or a boolean mask for frame tensors)."""
    out = []
    if kind == "dK":
        L, H2, H4 = shape
        H = H2 // 2
        kblk = 128 if H >= 128 else H
        for l in range(L):
            for half, r0 in (("x", 0), ("h", H)):
                for g in range(4):
                    for k0 in range(0, H, kblk):
                        out.append(("layer %d %s-half gate %s rows %d:%d" % (l, half, "ijfo"[g], k0, min(H, k0 + kblk)),
                                    (l, slice(r0 + k0, r0 + min(H, k0 + kblk)), slice(g * H, (g + 1) * H))))
    elif kind == "db":
        L, H4 = shape
        H = H4 // 4
        for l in range(L):
            for g in range(4):
                for u in range(0, H, 16):
                    out.append(("layer %d gate %s units %d:%d" % (l, "ijfo"[g], u, u + 16), (l, slice(g * H + u, g * H + u + 16))))
    elif kind in ("hT", "cT"):
        L, B, H = shape
        for l in range(L):
            for b0 in range(0, B, 16):
                out.append(("layer %d rows %d:%d" % (l, b0, min(B, b0 + 16)), (l, slice(b0, min(B, b0 + 16)))))
    elif kind in ("ztop", "dz0", "h"):
        lead = ()
        if kind == "h":
            lead, shape = tuple(range(shape[0])), shape[1:]
        T, B, H = shape
        lengths = np.asarray(lengths)
        for l in (lead or (None,)):
            for b0 in range(0, B, 16):
                rows = np.arange(b0, min(B, b0 + 16))
                longest = int(lengths[rows].max())
                for t0, t1 in _thirds(longest):
                    valid = (np.arange(t0, t1)[:, None] < lengths[rows][None, :])       # [frames, rows]
                    for u in range(0, H, 16):
                        label = "%srows %d:%d frames %d:%d units %d:%d" % ("" if l is None else "layer %d " % l, b0, rows[-1] + 1, t0, t1, u, u + 16)
                        idx = (slice(t0, t1), slice(b0, rows[-1] + 1), slice(u, u + 16))
                        out.append((label, ((l,) + idx if l is not None else idx, valid)))
    else:
        raise ValueError(kind)
    return out


def slice_errors(got, ref, kind, lengths=None):
    """One relative error per slice of `kind`, each normalised by THAT slice's own reference maximum: a list of
    (label, error, slice maximum / tensor maximum).  Frame tensors (ztop, dz0, h) count valid frames only; that ztop and dz0 are
    exactly zero at and past a row's length is padding_is_zero()'s business.  Nothing is left out here: the caller compares the
    third field with FLOOR (no case of the matrix may have a slice under it: tests/test_cpu_lstm_stack_ref.py)."""
    got = torch.as_tensor(got).detach().to("cpu", torch.float64)
    ref = torch.as_tensor(ref).detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, (kind, got.shape, ref.shape)
    whole = float(ref.abs().max()) + 1e-300
    out = []
    for label, idx in slices(kind, tuple(ref.shape), lengths):
        if kind in ("ztop", "dz0", "h"):
            idx, valid = idx
            m = torch.as_tensor(valid)[:, :, None]
            g, r = got[idx] * m, ref[idx] * m
        else:
            g, r = got[idx], ref[idx]
        top = float(r.abs().max())
        out.append((label, float((g - r).abs().max()) / (top + 1e-300), top / whole))
    return out


def worst(errors):
    """(error, label) of the worst slice; a slice under FLOOR counts as infinitely wrong (the inputs must not produce one)."""
    return max(((float("inf") if frac < FLOOR else e), label) for label, e, frac in errors)


def padding_is_zero(x, lengths):
    """ztop / dz0 [T,B,H]: every frame at or past a row's length is EXACTLY zero."""
    x = torch.as_tensor(x).detach().cpu()
    T = x.shape[0]
    dead = torch.as_tensor(np.arange(T)[:, None] >= np.asarray(lengths)[None, :])
    return bool((x[dead] == 0).all())


def rel_err(a, b):
    """The whole-tensor metric of tests/test_gpu_model.py."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


# ------------------------------------------------------------------------------------------------ the matrix
# Every case names the plan it expects on an MI355X (ops.lstm_plan) -- only the keys that define its variant -- and the variants of
# VARIANTS below it stands for.  Sizes: the float64 reference of every case runs on a CPU in seconds.
#   lens: "ragged" (one row of T, one of T-1, one of 1, one of 0 where B allows, the rest random), "full", "last_tile_empty"
#   regime: "nominal" (weights 0.6/sqrt(H), biases 0.1 sigma: tests/test_gpu_lstm_pair.py) or "saturating" (SAT_* below)
#   state: h0/c0 drawn at 0.3 sigma;  extras: "padding" (garbage past the lengths must not matter), "accumulate" (dK, db start
#   non-zero, dz0 starts with garbage), "dropout" (keep_in 0.8, keep_out 0.7), "per_diagonal" (AMDSPEECH_LSTM_PER_DIAGONAL)
def _case(name, T, B, H, L, precision, plan, covers, lens="ragged", regime="nominal", state=False, extras=()):
    return dict(name=name, T=T, B=B, H=H, L=L, precision=precision, plan=plan, covers=tuple(covers), lens=lens, regime=regime,
                state=state, extras=tuple(extras))


def _diag(uw, mt, bwd="diag"):
    return dict(fwd_path="diag", bwd_path=bwd, uw=uw, fwd_mt=mt)


def _bf3():
    return dict(fwd_path="diag_bf3", bwd_path="diag_bf3")


def _flow(kb, mv, w, q, nmt):
    return dict(fwd_path="flow", bwd_path="flow", kb=kb, mv=mv, w_pieces=w, flow2_q=q, nmt=nmt, dz0_inkernel=1)


def _big(bwd, bf16p=0, pair=0):
    return dict(fwd_path="big", bwd_path=bwd, bf16p=bf16p, pair=pair, uw=16)


CASES = [
    # ---- launch-per-diagonal, f32 (lstm_fwd_step<UW, ., ., ., MT> / lstm_bwd_step)
    _case("diag-h16-b1-t1", 1, 1, 16, 2, 0, _diag(4, 1), ["diag:H16", "diag:uw4", "diag:mt1"], lens="full", state=True),
    _case("diag-h48-b17-t2", 2, 17, 48, 3, 0, _diag(4, 2), ["diag:H48", "diag:mt2"], state=True, extras=["padding"]),
    _case("diag-h64-b15-t8", 8, 15, 64, 3, 0, _diag(4, 1), ["diag:uw4"], extras=["accumulate"]),
    _case("diag-h64-b33-uw8", 10, 33, 64, 6, 0, _diag(8, 1), ["diag:uw8", "diag:mt1"], regime="saturating", extras=["dropout"]),
    _case("diag-h96-b64-uw8-mt2", 65, 64, 96, 4, 0, _diag(8, 2), ["diag:uw8", "diag:mt2"], lens="last_tile_empty", state=True),
    _case("diag-h32-b16-long", 300, 16, 32, 2, 0, _diag(4, 1), ["diag:long"], state=True),
    # ---- launch-per-diagonal, reduced precision (lstm_fwd_step_bf3 / lstm_bwd_step_bf3)
    _case("bf3-h32-p1", 9, 17, 32, 2, 1, _bf3(), ["bf3:p1", "bf3:H32"], state=True, extras=["padding"]),
    _case("bf3-h64-p2", 10, 33, 64, 3, 2, _bf3(), ["bf3:p2", "bf3:H64"], extras=["accumulate"]),
    _case("bf3-h128-p1", 64, 16, 128, 2, 1, _bf3(), ["bf3:H128"], extras=["dropout"]),
    _case("bf3-h384-p2", 12, 20, 384, 2, 2, _bf3(), ["bf3:H384"], state=True),
    _case("bf3-h384-p1", 8, 15, 384, 1, 1, _bf3(), ["bf3:H384", "bf3:p1"], lens="full", regime="saturating"),
    _case("bf3-h64-p1-long", 300, 16, 64, 2, 1, _bf3(), ["bf3:long"]),
    # ---- hoisted backward (forward: launch-per-diagonal)
    _case("hoist-h768-b17", 10, 17, 768, 2, 0, _diag(8, 2, "hoist"), ["hoist:H768"], state=True, extras=["padding", "accumulate"]),
    _case("hoist-h1024-b65", 8, 65, 1024, 1, 0, _diag(8, 1, "hoist"), ["hoist:H1024x5"], extras=["dropout"]),
    _case("hoist-h768-b33-sat", 9, 33, 768, 1, 0, _diag(8, 1, "hoist"), ["hoist:H768"], regime="saturating", lens="last_tile_empty", state=True),
    _case("hoist-h768-long", 200, 17, 768, 1, 0, _diag(8, 2, "hoist"), ["hoist:long"]),
    # ---- dataflow kernels, f32 (lstm_fwd_flow2<KB, 0, MV> / lstm_bwd_flow2<KB, 0>)
    _case("flow-kb1-b17", 63, 17, 128, 2, 0, _flow(1, 0, 0, 1, 2), ["flow:kb1", "flow:w0"], state=True, extras=["padding"]),
    _case("flow-kb1-b1-one-group", 64, 1, 128, 1, 0, _flow(1, 0, 8, 1, 1), ["flow:groups1", "flow:w8"], lens="full", extras=["accumulate"]),
    _case("flow-kb2-b64-all-xcds", 65, 64, 256, 2, 0, _flow(2, 0, 0, 2, 4), ["flow:kb2", "flow:groups8", "flow:w0"], extras=["dropout"]),
    _case("flow-kb2-long", 300, 16, 256, 2, 0, _flow(2, 0, 8, 2, 1), ["flow:long", "flow:w8"]),
    _case("flow-kb3-b33", 10, 33, 384, 2, 0, _flow(3, 0, 0, 1, 3), ["flow:kb3"], regime="saturating", state=True),
    _case("flow-kb4-mv1", 64, 15, 512, 3, 0, _flow(4, 1, 8, 4, 1), ["flow:kb4", "flow:mv1", "flow:w8"], state=True),
    _case("flow-kb4-b33-mv1", 9, 33, 512, 2, 0, _flow(4, 1, 0, 4, 3), ["flow:kb4", "flow:mv1"], lens="last_tile_empty", state=True),
    _case("flow-kb4-b64-mv0", 8, 64, 512, 2, 0, _flow(4, 0, 0, 4, 4), ["flow:mv0-all-xcds", "flow:groups8"], extras=["padding"]),
    # ---- dataflow kernels, reduced precision (lstm_fwd_flow2<KB, PR> / lstm_bwd_flow2<KB, PR>)
    _case("flowr-kb2-p1", 64, 17, 256, 2, 1, _flow(2, 0, 8, 1, 2), ["flowr:kb2p1"], state=True, extras=["padding"]),
    _case("flowr-kb2-p2", 10, 33, 256, 2, 2, _flow(2, 0, 0, 1, 3), ["flowr:kb2p2"], extras=["accumulate"]),
    _case("flowr-kb4-p1", 9, 16, 512, 1, 1, _flow(4, 0, 0, 1, 1), ["flowr:kb4p1"], regime="saturating", extras=["dropout"]),
    _case("flowr-kb4-p2", 65, 64, 512, 2, 2, _flow(4, 0, 0, 1, 4), ["flowr:kb4p2"], state=True, lens="last_tile_empty"),
    _case("flowr-kb2-p2-long", 300, 16, 256, 1, 2, _flow(2, 0, 8, 1, 1), ["flowr:long"]),
    # ---- H = 1024, one launch per layer (lstm_fwd_big<PR> / lstm_bwd_big<PR> / lstm_bwd_big1)
    _case("big-p0-b64", 8, 64, 1024, 2, 0, _big("big"), ["big:fwd-p0", "big:bwd-big"], state=True, extras=["padding", "accumulate"]),
    _case("big-p1-b17", 10, 17, 1024, 1, 1, _big("big"), ["big:fwd-p1"], regime="saturating", extras=["dropout"]),
    _case("big-p2-b1", 9, 1, 1024, 2, 2, _big("big", 0, 1), ["big:fwd-p2"], lens="full"),
    _case("big1-p2-tb256", 16, 16, 1024, 1, 2, _big("big1", 1, 1), ["big:bwd-big1-copies"], state=True, extras=["padding"]),
    _case("big-p2-tb250", 10, 25, 1024, 1, 2, _big("big", 0, 1), ["big:copies-reserved-unused"], extras=["accumulate"]),
    _case("big-p0-long", 200, 16, 1024, 1, 0, _big("big"), ["big:long"]),
    # ---- AMDSPEECH_LSTM_PER_DIAGONAL: a dataflow and a per-layer shape on the launch-per-diagonal kernels
    _case("perdiag-flow-shape", 10, 17, 128, 2, 0, _diag(4, 2), ["perdiag:flow"], extras=["per_diagonal"], state=True),
    _case("perdiag-big-shape", 8, 33, 1024, 1, 0, _diag(8, 1, "hoist"), ["perdiag:big"], extras=["per_diagonal"]),
]

# The reachable variants, each with the rule of csrc/lstm.hip it comes from (tests/test_gpu_lstm_stack.py asserts the matrix covers all)
VARIANTS = {
    "diag:H16": "check_desc: H a multiple of 16; the smallest accepted",
    "diag:H48": "check_desc: H % 16 == 0 but not a power of two (three 16-unit groups)",
    "diag:uw4": "pick_uw: L * (H/8) * ceil(B/32) < 96 workgroups -> 4 units per workgroup",
    "diag:uw8": "pick_uw: >= 96 workgroups -> 8 units per workgroup",
    "diag:mt1": "lstm_plan: fwd_mt = 1 for an odd number of batch tiles",
    "diag:mt2": "lstm_plan: fwd_mt = 2 for an even number of batch tiles",
    "diag:long": "a few hundred frames on lstm_fwd_step / lstm_bwd_step",
    "bf3:p1": "lstm_plan: precision 1 outside flow_shape_ok / use_big_fwd -> diag_bf3",
    "bf3:p2": "lstm_plan: precision 2 outside flow_shape_ok / use_big_fwd -> diag_bf3 (batched products single bf16)",
    "bf3:H32": "check_desc: reduced precision needs H % 32 == 0; the smallest",
    "bf3:H64": "lstm_fwd_step_bf3 at two K blocks of 32",
    "bf3:H128": "flow_shape_ok: reduced precision needs H % 256 == 0, so H = 128 stays on diag_bf3",
    "bf3:H384": "flow_shape_ok: H = 384 is f32-only on the dataflow kernels -> diag_bf3",
    "bf3:long": "a few hundred frames on the bf16x3 step kernels",
    "hoist:H768": "lstm_plan: pr == 0 && H >= 768 && nmt >= 2, not a use_big_fwd shape",
    "hoist:H1024x5": "use_big_fwd: ceil(B/16) <= 4 fails at five batch tiles -> forward diag, backward hoist",
    "hoist:long": "a few hundred frames on the hoisted backward",
    "flow:kb1": "flow_fwd_kernel / flow_bwd_kernel: kb = H/128 = 1",
    "flow:kb2": "kb = 2 (flow2_q = 2)",
    "flow:kb3": "kb = 3 (flow2_q = 1: three tiles per wave do not split)",
    "flow:kb4": "kb = 4 (flow2_q = 4)",
    "flow:mv1": "fwd_workers_fit: f32, H = 512, a spare XCD -> x-product workers (lstm_fwd_flow2<4, 0, 1>)",
    "flow:mv0-all-xcds": "fwd_workers_fit: H = 512 with L * nmt = 8 -> no spare XCD, lstm_fwd_flow2<4, 0, 0>",
    "flow:w8": "lstm_plan: T >= 64 and groups < 8 -> in-kernel weight-gradient workers (w_pieces = 8)",
    "flow:w0": "lstm_plan: T < 64 or no spare XCD -> w_pieces = 0",
    "flow:groups8": "use_flow: L * nmt = 8, every XCD carries a recurrence group (the largest B the path takes)",
    "flow:groups1": "one recurrence group",
    "flow:long": "a few hundred frames on the dataflow kernels",
    "flowr:kb2p1": "flow_shape_ok: precision 1 at H = 256", "flowr:kb2p2": "precision 2 at H = 256",
    "flowr:kb4p1": "precision 1 at H = 512", "flowr:kb4p2": "precision 2 at H = 512",
    "flowr:long": "a few hundred frames on the reduced-precision dataflow kernels",
    "big:fwd-p0": "use_big_fwd: H = 1024, <= 4 batch tiles -> lstm_fwd_big<0>", "big:fwd-p1": "lstm_fwd_big<1>",
    "big:fwd-p2": "lstm_fwd_big<2> (one stack alone runs on the XCD pairs)",
    "big:bwd-big": "lstm_plan: bwd = big unless the pair condition and the bf16 copies hold",
    "big:bwd-big1-copies": "bf16p_layout_on: precision 2, T*B % 64 == 0 and >= 256 -> lstm_bwd_big1 + gemm_bf16p",
    "big:copies-reserved-unused": "bf16p_layout_reserved but T*B = 250: the region is laid out, gemm_bf16 runs",
    "big:long": "a few hundred frames on the per-layer kernels",
    "perdiag:flow": "use_flow: AMDSPEECH_LSTM_PER_DIAGONAL reroutes a dataflow shape to diag",
    "perdiag:big": "use_big_fwd: AMDSPEECH_LSTM_PER_DIAGONAL reroutes a per-layer shape to diag (backward: hoist)",
}

FAMILY_OF = {"diag": "diag", "bf3": "diag_bf3", "hoist": "hoist", "flow": "flow", "flowr": "flow-reduced", "big": "big", "big1": "big",
             "perdiag": "diag"}


def family(case):
    return FAMILY_OF[case["name"].split("-")[0]]


# Saturating regime: weights and biases scaled so that the gate pre-activations have a standard deviation around 4 and a fifth of
# the biases sit at +-3.  Fixed from the float64 reference (tests/test_cpu_lstm_stack_ref.py asserts the saturated fraction).
SAT_WEIGHT, SAT_BIAS, SAT_BIAS_PINNED = 4.0, 1.0, 3.0


def make_lengths(case):
    T, B = case["T"], case["B"]
    rng = np.random.RandomState(1000 + T + 7 * B)
    if case["lens"] == "full":
        return np.full(B, T, np.int32)
    lengths = rng.randint(1, T + 1, size=B).astype(np.int32)
    for pos, val in ((0, T), (1, T - 1), (2, 1), (3, 0)):
        if pos < B:
            lengths[pos] = max(val, 0)
    if case["lens"] == "last_tile_empty":
        lengths[(B - 1) // 16 * 16:] = 0
    return lengths


def make_inputs(case):
    """Everything a case feeds the kernels, as float32 CPU tensors (the reference takes the same values in float64)."""
    T, B, H, L = case["T"], case["B"], case["H"], case["L"]
    g = torch.Generator(device="cpu").manual_seed(sum(map(ord, case["name"])))
    sat = case["regime"] == "saturating"
    # x . W has variance ~ |x|^2 w^2 2H: nominal 0.6/sqrt(H); saturating: sigma(pre-activation) ~ SAT_WEIGHT on a unit input
    k = torch.randn(L, 2 * H, 4 * H, generator=g) * ((SAT_WEIGHT if sat else 0.6) / np.sqrt(H))
    b = torch.randn(L, 4 * H, generator=g) * (SAT_BIAS if sat else 0.1)
    if sat:
        pin = torch.rand(L, 4 * H, generator=g)
        b = torch.where(pin < 0.1, torch.full_like(b, SAT_BIAS_PINNED), torch.where(pin > 0.9, torch.full_like(b, -SAT_BIAS_PINNED), b))
    z0 = torch.randn(T, B, H, generator=g)
    lengths = make_lengths(case)
    # dense and non-zero on every valid frame: no gradient slice is structurally empty
    dztop = torch.randn(T, B, H, generator=g) * 0.1
    dztop = torch.where(dztop.abs() < 0.01, torch.full_like(dztop, 0.01), dztop)
    dead = torch.as_tensor(np.arange(T)[:, None] >= lengths[None, :])
    z0[dead] = 0.0
    dztop[dead] = 0.0
    h0 = c0 = None
    if case["state"]:
        h0, c0 = torch.randn(L, B, H, generator=g) * 0.3, torch.randn(L, B, H, generator=g) * 0.3
    dk0 = db0 = None
    if "accumulate" in case["extras"]:
        dk0, db0 = torch.randn(L, 2 * H, 4 * H, generator=g) * 0.05, torch.randn(L, 4 * H, generator=g) * 0.05
    garbage = (torch.rand(T, B, H, generator=g) - 0.5) * 2e3
    garbage = torch.where(garbage.abs() < 1.0, torch.full_like(garbage, 1e3), garbage)
    return dict(k=k, b=b, z0=z0, dztop=dztop, lengths=lengths, h0=h0, c0=c0, dk0=dk0, db0=db0, garbage=garbage, dead=dead)


KEEP_IN, KEEP_OUT = 0.8, 0.7


def cpu_masks(case):
    """Stand-in multipliers for a "dropout" case where no GPU is at hand (the measurement below, the floor check): Bernoulli(keep) /
    keep from torch's generator.  The GPU test feeds the reference the multipliers the library exports instead."""
    if "dropout" not in case["extras"]:
        return None, None
    g = torch.Generator(device="cpu").manual_seed(77 + case["T"])
    shape = (case["T"], case["B"], case["H"])
    draw = lambda keep: [(torch.rand(shape, generator=g) < keep).to(torch.float64) / keep for _ in range(case["L"])]
    return draw(KEEP_IN), draw(KEEP_OUT)


def reference(case, inp, in_mult=None, out_mult=None, emulate=None):
    """Outputs and gradients of a case by the reference: dict of ztop, h, hT, cT, dK, db, dz0 (dK / db include the initial values
    of an "accumulate" case)."""
    f = forward(inp["z0"], inp["k"], inp["b"], inp["lengths"], inp["h0"], inp["c0"], in_mult, out_mult, emulate)
    r = backward(f["cache"], inp["dztop"])
    out = {k: f[k] for k in OUTPUT_KINDS}
    out.update(r)
    if inp["dk0"] is not None:
        out["dK"] = out["dK"] + inp["dk0"].to(out["dK"].dtype)
        out["db"] = out["db"] + inp["db0"].to(out["db"].dtype)
    return out


def emulation(case):
    return {0: "f32", 1: "bf16x3", 2: "bf16"}[case["precision"]]


def all_slice_errors(got, ref, lengths):
    return {kind: slice_errors(got[kind], ref[kind], kind, lengths) for kind in OUTPUT_KINDS + GRAD_KINDS}


# (family, regime, precision) -> {kind: largest per-slice error of the emulated arithmetic}: the run recorded in the docstring
MEASURED = {
    ('big', 'nominal', 0): {'ztop': 9.5e-07, 'h': 1.0e-06, 'hT': 5.9e-07, 'cT': 4.4e-07, 'dK': 7.5e-07, 'db': 9.2e-07, 'dz0': 8.9e-07},
    ('big', 'nominal', 2): {'ztop': 6.5e-03, 'h': 7.9e-03, 'hT': 4.3e-03, 'cT': 3.6e-03, 'dK': 6.7e-03, 'db': 1.2e-02, 'dz0': 7.4e-03},
    ('big', 'saturating', 1): {'ztop': 6.3e-05, 'h': 6.3e-05, 'hT': 4.7e-05, 'cT': 2.2e-05, 'dK': 3.7e-05, 'db': 1.1e-04, 'dz0': 5.6e-05},
    ('diag', 'nominal', 0): {'ztop': 9.8e-07, 'h': 9.8e-07, 'hT': 4.9e-07, 'cT': 4.2e-07, 'dK': 7.1e-07, 'db': 8.6e-07, 'dz0': 1.1e-06},
    ('diag', 'saturating', 0): {'ztop': 1.2e-05, 'h': 1.2e-05, 'hT': 1.1e-05, 'cT': 3.6e-06, 'dK': 1.4e-05, 'db': 2.5e-05, 'dz0': 2.1e-05},
    ('diag_bf3', 'nominal', 1): {'ztop': 8.4e-06, 'h': 8.8e-06, 'hT': 7.1e-06, 'cT': 5.0e-06, 'dK': 8.1e-06, 'db': 1.5e-05, 'dz0': 9.4e-06},
    ('diag_bf3', 'nominal', 2): {'ztop': 4.3e-03, 'h': 6.9e-03, 'hT': 3.6e-03, 'cT': 3.0e-03, 'dK': 5.5e-03, 'db': 6.8e-03, 'dz0': 7.3e-03},
    ('diag_bf3', 'saturating', 1): {'ztop': 5.1e-05, 'h': 5.1e-05, 'hT': 3.8e-05, 'cT': 1.5e-05, 'dK': 3.8e-05, 'db': 7.0e-05, 'dz0': 6.7e-05},
    ('flow', 'nominal', 0): {'ztop': 5.2e-07, 'h': 9.2e-07, 'hT': 6.4e-07, 'cT': 4.3e-07, 'dK': 7.7e-07, 'db': 1.1e-06, 'dz0': 1.4e-06},
    ('flow', 'saturating', 0): {'ztop': 5.8e-06, 'h': 5.8e-06, 'hT': 5.0e-06, 'cT': 1.5e-06, 'dK': 4.7e-06, 'db': 9.5e-06, 'dz0': 8.3e-06},
    ('flow-reduced', 'nominal', 1): {'ztop': 6.2e-06, 'h': 9.4e-06, 'hT': 6.9e-06, 'cT': 6.0e-06, 'dK': 7.9e-06, 'db': 9.8e-06, 'dz0': 8.7e-06},
    ('flow-reduced', 'nominal', 2): {'ztop': 6.6e-03, 'h': 7.5e-03, 'hT': 5.2e-03, 'cT': 3.5e-03, 'dK': 5.8e-03, 'db': 6.1e-03, 'dz0': 6.6e-03},
    ('flow-reduced', 'saturating', 1): {'ztop': 5.3e-05, 'h': 6.4e-05, 'hT': 4.8e-05, 'cT': 1.0e-05, 'dK': 4.3e-05, 'db': 1.1e-04, 'dz0': 5.7e-05},
    ('hoist', 'nominal', 0): {'ztop': 1.3e-06, 'h': 1.5e-06, 'hT': 7.0e-07, 'cT': 5.8e-07, 'dK': 7.1e-07, 'db': 1.1e-06, 'dz0': 1.1e-06},
    ('hoist', 'saturating', 0): {'ztop': 6.2e-06, 'h': 6.2e-06, 'hT': 4.8e-06, 'cT': 1.5e-06, 'dK': 3.9e-06, 'db': 5.4e-06, 'dz0': 4.8e-06},
}


def bound(case, kind):
    """The tolerance of a slice of `kind` in `case`: min(cap, FACTOR x measured), see the module docstring."""
    cap = CAPS[case["precision"]][0 if kind in OUTPUT_KINDS else 1]
    return min(cap, FACTOR * MEASURED[(family(case), case["regime"], case["precision"])][kind])


def measure(cases=CASES, verbose=False):
    """Runs the emulated arithmetic of every case against float64 and returns the MEASURED dict."""
    table = {}
    for case in cases:
        inp = make_inputs(case)
        im, om = cpu_masks(case)
        ref, emu = reference(case, inp, im, om), reference(case, inp, im, om, emulate=emulation(case))
        errs = all_slice_errors(emu, ref, inp["lengths"])
        key = (family(case), case["regime"], case["precision"])
        row = table.setdefault(key, {k: 0.0 for k in OUTPUT_KINDS + GRAD_KINDS})
        for kind, e in errs.items():
            row[kind] = max(row[kind], max(x[1] for x in e))
        if verbose:
            print("  %-26s " % case["name"] + " ".join("%s %.1e" % (k, max(x[1] for x in e)) for k, e in errs.items()), flush=True)
    return table


if __name__ == "__main__":
    import time
    t0 = time.time()
    table = measure(verbose=True)
    names = OUTPUT_KINDS + GRAD_KINDS
    print("\nMEASURED = {")
    for key in sorted(table):
        print("    %r: {%s}," % (key, ", ".join("%r: %.1e" % (k, table[key][k]) for k in names)))
    print("}\n")
    print("%-13s %-10s pr | %s" % ("family", "regime", " | ".join("%-15s" % k for k in names)))
    for key in sorted(table):
        cells = []
        for k in names:
            cap = CAPS[key[2]][0 if k in OUTPUT_KINDS else 1]
            cells.append("%.1e>%.1e%s" % (table[key][k], min(cap, FACTOR * table[key][k]), "c" if FACTOR * table[key][k] > cap else " "))
        print("%-13s %-10s %d  | %s" % (key[0], key[1], key[2], " | ".join(cells)))
    print("(measured > bound; c: bound is the cap)   %.0f s" % (time.time() - t0))
