"""float64 reference of the layer-wise bidirectional stack (tf.contrib.rnn.stack_bidirectional_dynamic_rnn over TF
BasicLSTMCell + DropoutWrapper).  Checker only: plain torch and numpy, no GPU, nothing of the product is imported.

Two parts.  forward() / forward_backward(): the whole model (input and output Linear around the stack) as a short torch-autograd
cell that takes explicit dropout masks -- what the engine tests compare with.  call_forward() / call_backward() (further down): one
ops.lstm_bidir_fwd / ops.lstm_bidir_bwd call as include/amdspeech.h states it, every layer's outputs, the forward cells' final state
and every cell's gradients, with a HAND-WRITTEN backward pass so that it also runs in the arithmetic under test; with it the slice
metric, the matrix of cases (CASES, VARIANTS) and the bounds of tests/test_gpu_bidir_layer_paths.py.  The comment above
call_forward() states the slices, what may be left out of them and how a bound is formed.

MEASURED (`python tests/bidir_layer_ref.py`, CPU only: the largest per-slice relative error of the emulated arithmetic -- float32
for precision 0; float32 with the operands of every product cut to bf16 hi + bf16 lo for precision 1 -- against float64, over the
cases of a (precision, regime) family; bound = min(cap, 8 x measured), caps (1e-4, 2e-3) and (2e-4, 5e-3)):

pr regime     | y               | hT              | cT              | dK              | db              | dz0
0  nominal    | 2.0e-06>1.6e-05  | 1.2e-06>9.6e-06  | 8.5e-07>6.8e-06  | 2.5e-06>2.0e-05  | 2.5e-06>2.0e-05  | 1.2e-06>9.6e-06
0  saturating | 3.4e-06>2.7e-05  | 1.5e-06>1.2e-05  | 9.5e-07>7.6e-06  | 3.8e-06>3.0e-05  | 4.1e-06>3.3e-05  | 2.8e-06>2.2e-05
1  nominal    | 1.7e-05>1.4e-04  | 1.3e-05>1.0e-04  | 9.5e-06>7.6e-05  | 2.2e-05>1.8e-04  | 2.9e-05>2.3e-04  | 1.4e-05>1.1e-04
1  saturating | 5.1e-05>2.0e-04c | 2.7e-05>2.0e-04c | 1.3e-05>1.0e-04  | 7.4e-05>5.9e-04  | 1.0e-04>8.0e-04  | 8.6e-05>6.9e-04
(measured>bound; c: the bound is the cap)
"""
import numpy as np
import torch


def reverse_sequence(x, lengths):
    """tf.reverse_sequence on time-major [T,B,W], zeros past each length (what the kernels store there)."""
    T = x.shape[0]
    out = torch.zeros_like(x)
    for b, n in enumerate(lengths):
        n = int(n)
        if n > 0:
            out[:n, b] = torch.flip(x[:n, b], dims=[0])
    return out


def _cell_run(xs, kernel, bias, lengths, H, forget_bias, m_out, h0=None, c0=None):
    """One direction's cell over its inputs in its own step order: outputs [T,B,H] (0 past the length), final (h, c)."""
    T, B, _ = xs.shape
    h = torch.zeros(B, H, dtype=xs.dtype, device=xs.device) if h0 is None else h0
    c = torch.zeros(B, H, dtype=xs.dtype, device=xs.device) if c0 is None else c0
    live = torch.as_tensor(np.asarray(lengths), device=xs.device).view(B, 1)
    outs = []
    for s in range(T):
        g = torch.cat([xs[s], h], dim=1) @ kernel + bias
        i, j, f, o = torch.split(g, H, dim=1)
        cn = torch.sigmoid(f + forget_bias) * c + torch.sigmoid(i) * torch.tanh(j)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        on = (s < live).to(xs.dtype)
        c = on * cn + (1 - on) * c
        h = on * hn + (1 - on) * h
        y = on * hn
        outs.append(y * m_out[s] if m_out is not None else y)
    return torch.stack(outs), (h, c)


def forward(p, x, lengths, L, H, masks=None, forget_bias=1.0, h0=None, c0=None):
    """p: dict of float64 torch tensors in the engine's layout names (kernel_l / bw_kernel_l: (2H|3H, 4H)); x [T,B,D].
    masks: {("fw"|"bw", "in"|"out", l): [T,B,W] multipliers in the cell's step order} or None.  Returns logits, final fw state."""
    z0 = x @ p["input_w"] + p["input_b"]
    below = [z0]
    finals = []
    for l in range(L):
        inp = torch.cat(below, dim=2) if l > 0 else z0
        ys = {}
        for d, name in (("fw", "kernel_%d"), ("bw", "bw_kernel_%d")):
            xs = inp if d == "fw" else reverse_sequence(inp, lengths)
            if masks is not None:
                xs = xs * masks[(d, "in", l)]
            y, fin = _cell_run(xs, p[name % l], p[name.replace("kernel", "bias") % l], lengths, H, forget_bias,
                               masks[(d, "out", l)] if masks is not None else None,
                               h0[l] if (d == "fw" and h0 is not None) else None, c0[l] if (d == "fw" and c0 is not None) else None)
            ys[d] = y if d == "fw" else reverse_sequence(y, lengths)
            if d == "fw":
                finals.append(fin)
        below = [ys["fw"], ys["bw"]]
    logits = torch.cat(below, dim=2) @ p["output_w"] + p["output_b"]
    return logits, finals


def forward_backward(p_np, x, lengths, L, H, dlogits_fn, masks=None, device="cpu"):
    """-> logits (numpy), loss, gradients {name: numpy} of sum_b loss_b; dlogits_fn(logits_np) -> (loss, dlogits).  `device`: where
    torch evaluates the float64 graph (the GPU tests use the GPU for the full-size shapes: same arithmetic, float64)."""
    p = {k: torch.tensor(np.asarray(v, np.float64), device=device, requires_grad=True) for k, v in p_np.items()}
    m = None if masks is None else {k: torch.as_tensor(np.asarray(v, np.float64), device=device) for k, v in masks.items()}
    logits, _ = forward(p, torch.as_tensor(np.asarray(x, np.float64), device=device), lengths, L, H, m)
    ln = logits.detach().cpu().numpy()
    loss, dl = dlogits_fn(ln)
    logits.backward(torch.as_tensor(dl, device=device))
    return ln, loss, {k: v.grad.cpu().numpy() for k, v in p.items()}


def torch_lstm_forward(p, x, lengths, L, H, forget_bias=1.0):
    """The same model through torch.nn.LSTM(bidirectional=True, num_layers=L) on packed sequences: TF gate order i, j, f, o ->
    torch i, f, g, o, forget_bias folded into the f bias.  Returns logits (float64 numpy)."""
    D = p["input_w"].shape[1]
    lstm = torch.nn.LSTM(H, H, num_layers=L, bidirectional=True).double()

    def remap(kernel, bias, W):
        i, j, f, o = np.split(np.asarray(kernel, np.float64), 4, axis=1)
        bi, bj, bf, bo = np.split(np.asarray(bias, np.float64), 4)
        k = np.concatenate([i, f, j, o], axis=1)       # [W+H, 4H] torch order
        return (torch.as_tensor(k[:W].T.copy()), torch.as_tensor(k[W:].T.copy()),
                torch.as_tensor(np.concatenate([bi, bf + forget_bias, bj, bo])))

    with torch.no_grad():
        for l in range(L):
            W = H if l == 0 else 2 * H
            for suffix, name in (("", "kernel_%d"), ("_reverse", "bw_kernel_%d")):
                wi, wh, b = remap(p[name % l], p[name.replace("kernel", "bias") % l], W)
                getattr(lstm, "weight_ih_l%d%s" % (l, suffix)).copy_(wi)
                getattr(lstm, "weight_hh_l%d%s" % (l, suffix)).copy_(wh)
                getattr(lstm, "bias_ih_l%d%s" % (l, suffix)).copy_(b)
                getattr(lstm, "bias_hh_l%d%s" % (l, suffix)).zero_()
        xt = torch.as_tensor(np.asarray(x, np.float64))
        z0 = xt @ torch.as_tensor(np.asarray(p["input_w"], np.float64)) + torch.as_tensor(np.asarray(p["input_b"], np.float64))
        T, B = z0.shape[:2]
        keep = [b for b in range(B) if lengths[b] > 0]
        y = torch.zeros(T, B, 2 * H, dtype=torch.float64)
        if keep:
            packed = torch.nn.utils.rnn.pack_padded_sequence(z0[:, keep], torch.as_tensor([int(lengths[b]) for b in keep]),
                                                             enforce_sorted=False)
            out, _ = lstm(packed)
            out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
            y[:, keep] = out
        return (y @ torch.as_tensor(np.asarray(p["output_w"], np.float64)) + torch.as_tensor(np.asarray(p["output_b"], np.float64))).numpy()


def torch_lstm_states(kernels, biases, z0, lengths, h0=None, c0=None, forget_bias=1.0):
    """torch.nn.LSTM(bidirectional=True, num_layers=L) in float64 on packed sequences, fed the per-call tensors of call_forward()
    (the 2L cell kernels / biases, forward cells first) and an initial state for the FORWARD direction (zeros for the reverse one).
    Returns the top outputs [T,B,2H] (fw half first) and the forward cells' final (h, c) [L,B,H]; rows of length 0, which nn.LSTM
    does not take, keep their initial state and emit 0."""
    L = len(kernels) // 2
    H = kernels[0].shape[1] // 4
    T, B = z0.shape[:2]
    lstm = torch.nn.LSTM(H, H, num_layers=L, bidirectional=True).double()
    with torch.no_grad():
        for l in range(L):
            W = H if l == 0 else 2 * H
            for k, suffix in ((0, ""), (1, "_reverse")):
                kern = np.asarray(kernels[k * L + l], np.float64)
                i, j, f, o = np.split(kern, 4, axis=1)
                bi, bj, bf, bo = np.split(np.asarray(biases[k * L + l], np.float64), 4)
                kt = np.concatenate([i, f, j, o], axis=1)
                getattr(lstm, "weight_ih_l%d%s" % (l, suffix)).copy_(torch.as_tensor(kt[:W].T.copy()))
                getattr(lstm, "weight_hh_l%d%s" % (l, suffix)).copy_(torch.as_tensor(kt[W:].T.copy()))
                getattr(lstm, "bias_ih_l%d%s" % (l, suffix)).copy_(torch.as_tensor(np.concatenate([bi, bf + forget_bias, bj, bo])))
                getattr(lstm, "bias_hh_l%d%s" % (l, suffix)).zero_()
        keep = [b for b in range(B) if lengths[b] > 0]
        zt = torch.as_tensor(np.asarray(z0, np.float64))
        s0 = torch.zeros(2 * L, len(keep), H, dtype=torch.float64)      # nn.LSTM's order: layer-major, direction inside
        s1 = torch.zeros(2 * L, len(keep), H, dtype=torch.float64)
        hT = torch.zeros(L, B, H, dtype=torch.float64) if h0 is None else torch.as_tensor(np.asarray(h0, np.float64)).clone()
        cT = torch.zeros(L, B, H, dtype=torch.float64) if c0 is None else torch.as_tensor(np.asarray(c0, np.float64)).clone()
        if h0 is not None:
            s0[0::2], s1[0::2] = hT[:, keep], cT[:, keep]
        y = torch.zeros(T, B, 2 * H, dtype=torch.float64)
        if keep:
            packed = torch.nn.utils.rnn.pack_padded_sequence(zt[:, keep], torch.as_tensor([int(lengths[b]) for b in keep]), enforce_sorted=False)
            out, (hn, cn) = lstm(packed, (s0, s1))
            out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
            y[:, keep] = out
            hT[:, keep], cT[:, keep] = hn[0::2], cn[0::2]
    return y, hT, cT


# ================================================================================================ the per-call reference
# ops.lstm_bidir_fwd / ops.lstm_bidir_bwd as include/amdspeech.h states them ("layer-wise bidirectional stacks"), without the input
# and output Linear around them, the slice metric the GPU matrix (tests/test_gpu_bidir_layer_paths.py) is judged by, and the matrix.
#
# The backward pass is written out by hand (not autograd), product by product in the order the library forms them, so that the whole
# call can also run in the arithmetic under test (`emulate`): "f32" = float32 for precision 0, "bf16x3" = float32 with the operands
# of EVERY matrix product, forward and backward, cut to bf16 hi + bf16 lo (16 significant bits) for precision 1.
# tests/test_cpu_bidir_layer_paths.py ties the float64 run to autograd of forward() above and to torch.nn.LSTM.
#
# Slices.  An error is judged per slice, relative to the slice's OWN reference maximum:
#   y    [L,2,T,B,H]  per layer, direction, 16 batch rows, third of the rows' frames, 16 hidden units (valid frames only)
#   hT/cT [L,B,H]     per layer, 16 batch rows, 16 hidden units
#   dK   2L x [W+H,4H] per cell (layer, direction), row part (the x rows -- above layer 0 the fw half and the bw half apart -- and the
#                     h rows), gate block of the 4H columns, 16 hidden units
#   db   2L x [4H]    per cell, gate block, 16 hidden units
#   dz0  [T,B,H]      per 16 batch rows, third of the rows' frames, 16 hidden units (valid frames only)
# A slice is left out only where the result is STRUCTURALLY zero, whatever the weights:
#   - frames at and past a row's length (y, dz0; that they are exactly 0 is asserted apart), hence a 16-row block of rows of length 0;
#   - hT / cT of a 16-row block whose rows all have length 0 when no initial state is given;
#   - where no row is longer than one frame, for a cell that starts from zero (every backward cell; a forward cell without h0 / c0):
#     h_prev = c_prev = 0 at its only step, so the h rows of dK and the f-gate columns of dK and db are 0.
# Every other slice must hold something: its maximum at least FLOOR x its tensor's (the CPU test asserts it for every case and kind,
# and that everything outside the slices is exactly 0 in the reference).
#
# Bounds.  bound(case, kind) = min(cap, FACTOR x the largest per-slice error the emulated arithmetic shows on the CPU against float64
# over the cases of the (precision, regime) family).  FACTOR = 8 stands for accumulation order, the MFMA's K order, the LDS reduction
# order and the hardware's exp / rcp (the allowance of tests/lstm_stack_ref.py); the caps are the suite's whole-tensor tolerances
# applied per slice.  `python tests/bidir_layer_ref.py` measures the table (CPU only); nothing here comes from what the kernels return.
FORGET_BIAS = 1.0
FLOOR = 1e-6
FACTOR = 8.0
CAPS = {0: (1e-4, 2e-3), 1: (2e-4, 5e-3)}        # lstm_stack_ref.CAPS[0], [1]: (outputs and state, gradients)
OUTPUT_KINDS = ("y", "hT", "cT")
GRAD_KINDS = ("dK", "db", "dz0")
KINDS = OUTPUT_KINDS + GRAD_KINDS
DIRS = ("fw", "bw")


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _cut16(x):
    hi = _bf16(x)
    return hi + _bf16(x - hi)


def _operand_fn(emulate):
    return {None: None, "f32": None, "bf16x3": _cut16}[emulate]


def _mm(a, b, rnd):
    return a @ b if rnd is None else rnd(a) @ rnd(b)


def _mask(masks, d, which, l, dt):
    if masks is None or masks.get((d, which, l)) is None:
        return None
    return torch.as_tensor(masks[(d, which, l)]).to(dt)


def call_forward(z0, kernels, biases, lengths, h0=None, c0=None, masks=None, emulate=None):
    """z0 [T,B,H]; kernels / biases: the 2L cell tensors, forward cells' layers first ((2H|3H, 4H), [4H]); h0 / c0 [L,B,H] or None
    (forward cells; the backward cells start from zero); masks {("fw"|"bw", "in"|"out", l): multipliers in the cell's step order}.
    Returns y [L,2,T,B,H] (both directions' outputs of every layer in forward time, output mask applied, 0 past the length), the
    forward cells' hT / cT [L,B,H], and `cache` for call_backward()."""
    dt = torch.float64 if emulate is None else torch.float32
    rnd = _operand_fn(emulate)
    z0 = torch.as_tensor(z0).to(dt)
    T, B, H = z0.shape
    L = len(kernels) // 2
    lens = np.asarray(lengths).astype(np.int64)
    live_all = torch.as_tensor(np.arange(T)[:, None] < lens[None, :])          # [T,B]: step s of row b runs (either direction)
    y = torch.zeros(L, 2, T, B, H, dtype=dt)
    hT, cT = torch.zeros(L, B, H, dtype=dt), torch.zeros(L, B, H, dtype=dt)
    cells = {}
    inp = z0
    for l in range(L):
        W = inp.shape[2]
        for k, d in enumerate(DIRS):
            K, bias = torch.as_tensor(kernels[k * L + l]).to(dt), torch.as_tensor(biases[k * L + l]).to(dt)
            assert K.shape == (W + H, 4 * H), (l, d, K.shape)
            xs = inp if k == 0 else reverse_sequence(inp, lens)
            xs = xs * live_all[:, :, None].to(dt)                                # the pack: 0 at and past the length
            m_in, m_out = _mask(masks, d, "in", l, dt), _mask(masks, d, "out", l, dt)
            if m_in is not None:
                xs = xs * m_in
            G = (_mm(xs.reshape(T * B, W), K[:W], rnd) + bias).reshape(T, B, 4 * H)      # the batched product, bias in its epilogue
            h = torch.as_tensor(h0[l]).to(dt).clone() if (k == 0 and h0 is not None) else torch.zeros(B, H, dtype=dt)
            c = torch.as_tensor(c0[l]).to(dt).clone() if (k == 0 and c0 is not None) else torch.zeros(B, H, dtype=dt)
            st = {n: torch.zeros(T, B, H, dtype=dt) for n in ("i", "j", "f", "o", "c", "hprev", "cprev")}
            ys = torch.zeros(T, B, H, dtype=dt)
            for s in range(T):
                live = live_all[s].view(B, 1)
                g = _mm(h, K[W:], rnd) + G[s]
                i, j = torch.sigmoid(g[:, :H]), torch.tanh(g[:, H:2 * H])
                f, o = torch.sigmoid(g[:, 2 * H:3 * H] + FORGET_BIAS), torch.sigmoid(g[:, 3 * H:])
                cn = f * c + i * j
                hn = o * torch.tanh(cn)
                st["hprev"][s], st["cprev"][s] = h, c
                st["i"][s], st["j"][s], st["f"][s], st["o"][s], st["c"][s] = i, j, f, o, cn
                ys[s] = torch.where(live, hn, torch.zeros_like(hn))
                h, c = torch.where(live, hn, h), torch.where(live, cn, c)
            if m_out is not None:
                ys = ys * m_out
            y[l, k] = ys if k == 0 else reverse_sequence(ys, lens)
            if k == 0:
                hT[l], cT[l] = h, c
            st.update(xs=xs, K=K, W=W, m_in=m_in, m_out=m_out)
            cells[(l, k)] = st
        inp = torch.cat([y[l, 0], y[l, 1]], dim=2)
    cache = dict(cells=cells, lens=lens, live=live_all, T=T, B=B, H=H, L=L, dt=dt, rnd=rnd)
    return dict(y=y, hT=hT, cT=cT, cache=cache)


def call_backward(cache, dytop_fw, dytop_bw):
    """BPTT of call_forward() from the gradients of the top outputs (forward time): dK / db (lists of 2L, forward cells first; sums
    over the batch, NOT including what the caller's buffers held) and dz0 [T,B,H].  Hand-written."""
    T, B, H, L, dt, rnd, lens, live_all = (cache[n] for n in ("T", "B", "H", "L", "dt", "rnd", "lens", "live"))
    dy = [torch.as_tensor(dytop_fw).to(dt), torch.as_tensor(dytop_bw).to(dt)]
    dK, db = [None] * (2 * L), [None] * (2 * L)
    dz0 = None
    for l in range(L - 1, -1, -1):
        dinp = None
        for k in range(2):
            st = cache["cells"][(l, k)]
            K, W = st["K"], st["W"]
            dys = dy[k] if k == 0 else reverse_sequence(dy[k], lens)
            if st["m_out"] is not None:
                dys = dys * st["m_out"]
            dg_all = torch.zeros(T, B, 4 * H, dtype=dt)
            dh, dc = torch.zeros(B, H, dtype=dt), torch.zeros(B, H, dtype=dt)
            for s in range(T - 1, -1, -1):
                live = live_all[s].view(B, 1)
                i, j, f, o = st["i"][s], st["j"][s], st["f"][s], st["o"][s]
                dh_tot = dys[s] + dh
                tc = torch.tanh(st["c"][s])
                dc_tot = dc + dh_tot * o * (1.0 - tc * tc)
                dg = torch.cat([dc_tot * j * i * (1.0 - i), dc_tot * i * (1.0 - j * j),
                                dc_tot * st["cprev"][s] * f * (1.0 - f), dh_tot * tc * o * (1.0 - o)], dim=1)
                dg = torch.where(live, dg, torch.zeros_like(dg))
                dg_all[s] = dg
                # (the live steps of a row are a prefix of the step axis: below its length nothing is carried over a dead step)
                dh = _mm(dg, K[W:].t(), rnd)
                dc = torch.where(live, dc_tot * f, torch.zeros_like(dc))
            flat = dg_all.reshape(T * B, 4 * H)
            dK[k * L + l] = torch.cat([_mm(st["xs"].reshape(T * B, W).t(), flat, rnd), _mm(st["hprev"].reshape(T * B, H).t(), flat, rnd)])
            db[k * L + l] = flat.sum(dim=0)
            dx = _mm(flat, K[:W].t(), rnd).reshape(T, B, W)
            if st["m_in"] is not None:
                dx = dx * st["m_in"]
            dx = dx if k == 0 else reverse_sequence(dx, lens)
            dinp = dx if dinp is None else dinp + dx
        if l > 0:
            dy = [dinp[:, :, :H], dinp[:, :, H:]]
        else:
            dz0 = dinp
    return dict(dK=dK, db=db, dz0=dz0)


def gate_values(cache):
    """The activated gates of every valid step of every cell, tanh(j) mapped onto (0, 1): what the saturation check counts near 0 / 1."""
    vals = []
    for st in cache["cells"].values():
        live = cache["live"]
        vals.append(torch.cat([st["i"][live], st["f"][live], st["o"][live], (st["j"][live] + 1) / 2], dim=1))
    return torch.cat(vals)


# ------------------------------------------------------------------------------------------------ the slice metric
def _thirds(n):
    """The axis 0..n-1 cut into (up to) three non-empty contiguous parts."""
    if n <= 0:
        return []
    k = min(3, n)
    edges = [round(i * n / k) for i in range(k + 1)]
    return [(edges[i], edges[i + 1]) for i in range(k) if edges[i + 1] > edges[i]]


def starts_from_zero_for_one_step(info, k):
    """Cell of direction k never sees a non-zero h_prev / c_prev: no row runs a second step and the cell has no initial state."""
    return int(np.asarray(info["lengths"]).max()) <= 1 and (k == 1 or not info["state"])


def slices(kind, info):
    """[(label, key, group, index, valid)] of `kind` for a call of info = dict(T, B, H, L, lengths, state): `key` picks the tensor of
    a list kind (dK, db: the cell k * L + l), `group` indexes the tensor the slice belongs to (whose maximum FLOOR refers to),
    `index` the slice, `valid` a [frames, rows] mask for frame tensors (None elsewhere)."""
    T, B, H, L = (info[n] for n in ("T", "B", "H", "L"))
    lens = np.asarray(info["lengths"])
    out = []

    def frame_slices(prefix, lead):
        for b0 in range(0, B, 16):
            rows = np.arange(b0, min(B, b0 + 16))
            for t0, t1 in _thirds(int(lens[rows].max())):
                valid = np.arange(t0, t1)[:, None] < lens[rows][None, :]
                for u in range(0, H, 16):
                    out.append(("%srows %d:%d frames %d:%d units %d:%d" % (prefix, b0, rows[-1] + 1, t0, t1, u, u + 16), None, lead,
                                lead + (slice(t0, t1), slice(b0, rows[-1] + 1), slice(u, u + 16)), valid))

    if kind == "y":
        for l in range(L):
            for k, d in enumerate(DIRS):
                frame_slices("layer %d %s " % (l, d), (l, k))
    elif kind == "dz0":
        frame_slices("", ())
    elif kind in ("hT", "cT"):
        for l in range(L):
            for b0 in range(0, B, 16):
                b1 = min(B, b0 + 16)
                if not info["state"] and int(lens[b0:b1].max()) == 0:
                    continue
                for u in range(0, H, 16):
                    out.append(("layer %d rows %d:%d units %d:%d" % (l, b0, b1, u, u + 16), None, (l,), (l, slice(b0, b1), slice(u, u + 16)), None))
    elif kind in ("dK", "db"):
        for k, d in enumerate(DIRS):
            cold = starts_from_zero_for_one_step(info, k)
            for l in range(L):
                parts = [("x", 0)] if l == 0 else [("x-fw", 0), ("x-bw", H)]
                parts.append(("h", H if l == 0 else 2 * H))
                for g in range(4):
                    if cold and g == 2:
                        continue
                    for u in range(0, H, 16):
                        cols = slice(g * H + u, g * H + u + 16)
                        if kind == "db":
                            out.append(("layer %d %s gate %s units %d:%d" % (l, d, "ijfo"[g], u, u + 16), k * L + l, (), (cols,), None))
                            continue
                        for part, r0 in parts:
                            if cold and part == "h":
                                continue
                            out.append(("layer %d %s %s rows gate %s units %d:%d" % (l, d, part, "ijfo"[g], u, u + 16), k * L + l, (),
                                        (slice(r0, r0 + H), cols), None))
    else:
        raise ValueError(kind)
    return out


def _as64(x):
    return torch.as_tensor(x).detach().to("cpu", torch.float64)


def slice_errors(got, ref, kind, info):
    """One relative error per slice of `kind`, each normalised by THAT slice's own reference maximum: a list of (label, error,
    slice maximum / its tensor's maximum).  The caller compares the third field with FLOOR."""
    lists = kind in ("dK", "db")
    got = [_as64(t) for t in got] if lists else _as64(got)
    ref = [_as64(t) for t in ref] if lists else _as64(ref)
    tops = {}
    out = []
    for label, key, group, idx, valid in slices(kind, info):
        g, r = (got[key], ref[key]) if lists else (got, ref)
        assert g.shape == r.shape, (kind, key, g.shape, r.shape)
        if (key, group) not in tops:
            tops[(key, group)] = float(r[group].abs().max()) + 1e-300
        gs, rs = g[idx], r[idx]
        if valid is not None:
            m = torch.as_tensor(valid)[:, :, None]
            gs, rs = gs * m, rs * m
        top = float(rs.abs().max())
        out.append((label, float((gs - rs).abs().max()) / (top + 1e-300), top / tops[(key, group)]))
    return out


def outside_slices(ref, kind, info):
    """The largest |reference| over everything NO slice of `kind` covers (must be exactly 0: only structural zeros are left out)."""
    lists = kind in ("dK", "db")
    ref = [_as64(t) for t in ref] if lists else _as64(ref)
    seen = [torch.zeros(t.shape, dtype=torch.bool) for t in ref] if lists else torch.zeros(ref.shape, dtype=torch.bool)
    for _, key, _, idx, valid in slices(kind, info):
        s = seen[key] if lists else seen
        if valid is None:
            s[idx] = True
        else:
            s[idx] |= torch.as_tensor(valid)[:, :, None]
    if lists:
        return max(float(r[~s].abs().max()) if bool((~s).any()) else 0.0 for r, s in zip(ref, seen))
    return float(ref[~seen].abs().max()) if bool((~seen).any()) else 0.0


def worst(errors):
    """(error, label) of the worst slice; a slice under FLOOR counts as infinitely wrong (the inputs must not produce one)."""
    return max(((float("inf") if frac < FLOOR else e), label) for label, e, frac in errors)


def padding_is_zero(x, lengths):
    """[..., T, B, H]: every frame at or past a row's length is EXACTLY zero."""
    x = torch.as_tensor(x).detach().cpu()
    T = x.shape[-3]
    dead = torch.as_tensor(np.arange(T)[:, None] >= np.asarray(lengths)[None, :])
    return bool((x[..., dead, :] == 0).all())


def rel_err(a, b):
    """The whole-tensor metric of the engine tests (tests/test_gpu_bidir_layer.py)."""
    a, b = _as64(a), _as64(b)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def whole_errors(got, ref, kind):
    """rel_err per tensor of `kind` (per cell for dK / db, per layer and direction for y): the largest."""
    if kind in ("dK", "db"):
        return max(rel_err(g, r) for g, r in zip(got, ref))
    if kind == "y":
        got, ref = _as64(got), _as64(ref)
        return max(rel_err(got[l, k], ref[l, k]) for l in range(ref.shape[0]) for k in range(2))
    return rel_err(got, ref)


# ------------------------------------------------------------------------------------------------ csrc/lstm_bidir.h's rules, mirrored
def bf3_kpw(nkb, max_waves, max_kpw):
    """bf3_pick of csrc/lstm_bidir.h: K blocks of 32 per wave, the smallest instantiated count whose waves take the whole K."""
    kpw = 1
    while kpw <= max_kpw:
        if nkb % kpw == 0 and nkb // kpw <= max_waves:
            return kpw
        kpw *= 2
    return 0


def bf3_shape(H):
    """((forward KPW, waves), (backward KPW, waves)) of the bf16x3 kernels at hidden size H (bidir_plan)."""
    kf, kb = bf3_kpw(H // 32, 8, 4), bf3_kpw(4 * H // 32, 8, 16)
    return (kf, H // 32 // kf), (kb, 4 * H // 32 // kb)


def expected_path(case, cus=256):
    """The path of bidir_plan() (csrc/lstm_bidir.h) on a device of `cus` CUs whose CUs each take (at least) one workgroup of every kernel."""
    if "per_frame" in case["extras"]:
        return 0
    if case["precision"] == 1:
        nmt = (case["B"] + 15) // 16
        nwg = max(case["H"] // 8 * ((nmt + 3) // 4), case["H"] // 16 * ((nmt + 1) // 2))
    else:
        nwg = case["H"] // 8
    return 2 if 2 * nwg <= cus else (1 if nwg <= cus else 0)


PLAN_FIELDS = ("path", "cus", "fwd_kpw", "fwd_waves", "fwd_groups", "fwd_wgs", "fwd_lds", "bwd_kpw", "bwd_waves", "bwd_groups", "bwd_wgs",
               "bwd_lds")


def expected_plan(case, cus=256):
    """The twelve ints of amdspeech_lstm_bidir_plan on a device of `cus` CUs whose CUs each take (at least) one workgroup of every
    kernel (cus = 0: no device), from the driver's rules as they stood before the plan existed -- bf3_kpw, bf3_launch, bidir_lds and
    bidir_path of csrc/lstm.hip then -- written out here, not read back from the library:
      f32     8 waves, H / 8 workgroups per direction, LDS H x 36 floats forward (the padded slice) and H x 32 backward
      bf16x3  waves = K blocks / KPW; forward 8 units x groups of 4 row tiles, backward 16 units x groups of 2;
              LDS = waves x MB x NT KiB with (MB, NT) = (4, 2) forward and (2, 1) backward
      path    by the larger of the two kernels' workgroups per direction against the CUs; 0 by the flag ("per_frame")"""
    H, nmt = case["H"], (case["B"] + 15) // 16
    if case["precision"] == 1:
        (kf, wf), (kb, wb) = bf3_shape(H)
        gf, gb = (nmt + 3) // 4, (nmt + 1) // 2
        fwd = dict(kpw=kf, waves=wf, groups=gf, wgs=H // 8 * gf, lds=wf * 4 * 2 * 1024)
        bwd = dict(kpw=kb, waves=wb, groups=gb, wgs=H // 16 * gb, lds=wb * 2 * 1 * 1024)
    else:
        fwd = dict(kpw=0, waves=8, groups=1, wgs=H // 8, lds=H * 36 * 4)
        bwd = dict(kpw=0, waves=8, groups=1, wgs=H // 8, lds=H * 32 * 4)
    nwg = max(fwd["wgs"], bwd["wgs"])
    path = 0 if "per_frame" in case["extras"] else (2 if 2 * nwg <= cus else (1 if nwg <= cus else 0))
    plan = dict(path=path, cus=cus)
    plan.update({"fwd_" + k: v for k, v in fwd.items()})
    plan.update({"bwd_" + k: v for k, v in bwd.items()})
    assert tuple(plan) == PLAN_FIELDS
    return plan


WORKLOAD_SHAPES = ((998, 64, 1024, 5), (1001, 32, 512, 3))      # (T, B, H, L) of tools/bidir_layer_bench.py's two shapes


# ------------------------------------------------------------------------------------------------ the matrix
#   path: what amdspeech_lstm_bidir_path answers on a 256-CU device (2: one launch for both directions, 1: one per direction,
#         0: one per frame); a "per_frame" case asks for 0 by the flag, in-process
#   lens: "ragged" (rows of T, T-1, 1 and 0 frames where B allows, the rest random in 1..T), "full", "short" (every row shorter than
#         T, one of them empty), "ones" (every row one frame)
#   regime: "nominal" (weights 0.6/sqrt(H), biases 0.1 sigma) or "saturating" (SAT_* below)
#   state: h0 / c0 of the forward cells drawn at 0.5 sigma;  extras: "padding" (run twice: zeros, then finite values of magnitude 1e3
#   past every row's length in z0 and both dytop), "accumulate" (dK / db start from random values, dz0 from garbage), "dropout"
#   (keep_in 0.8, keep_out 0.5), "per_frame" (AMDSPEECH_LSTM_PER_DIAGONAL on both calls)
def _case(name, T, B, H, L, precision, path, covers, lens="ragged", regime="nominal", state=False, extras=()):
    return dict(name=name, T=T, B=B, H=H, L=L, precision=precision, path=path, covers=tuple(covers), lens=lens, regime=regime,
                state=state, extras=tuple(extras))


CASES = [
    # ---- precision 0: lstm_layer_fwd / lstm_layer_bwd
    _case("f32-h16-b1", 5, 1, 16, 2, 0, 2, ["f32:H16", "f32:B1"]),
    _case("f32-h48-l3-b5", 7, 5, 48, 3, 0, 2, ["f32:H48", "f32:L3", "lens:0-1-T"]),
    _case("f32-h1008-b3", 4, 3, 1008, 2, 0, 2, ["f32:H1008"]),
    _case("f32-h1024-b2-t4", 4, 2, 1024, 2, 0, 2, ["f32:H1024"]),
    _case("f32-h128-b64", 6, 64, 128, 2, 0, 2, ["f32:one-pass"]),
    _case("f32-h128-b65", 6, 65, 128, 2, 0, 2, ["f32:second-pass-one-row"]),
    _case("f32-h128-b130", 5, 130, 128, 2, 0, 2, ["f32:three-passes"]),
    _case("f32-t1", 1, 5, 64, 2, 0, 2, ["f32:T1"], state=True),
    _case("f32-short", 8, 6, 32, 2, 0, 2, ["f32:lens-short"], lens="short"),
    _case("f32-ones", 5, 7, 32, 2, 0, 2, ["f32:lens-ones"], lens="ones", state=True),
    _case("f32-state", 9, 17, 64, 2, 0, 2, ["f32:state"], state=True),
    _case("f32-dropout", 8, 12, 64, 3, 0, 2, ["f32:dropout"], extras=["dropout"]),
    _case("f32-accumulate", 7, 9, 32, 2, 0, 2, ["f32:accumulate"], extras=["accumulate"]),
    _case("f32-padding", 9, 20, 64, 2, 0, 2, ["f32:padding"], extras=["padding"]),
    _case("f32-per-frame", 6, 21, 64, 2, 0, 0, ["f32:per-frame"], extras=["per_frame"]),
    _case("f32-saturating", 8, 10, 64, 2, 0, 2, ["f32:saturating"], regime="saturating"),
    # ---- precision 1: lstm_layer_fwd_bf3<KPW> / lstm_layer_bwd_bf3<KPW>
    _case("bf3-h32", 9, 5, 32, 2, 1, 2, ["bf3:fwd-kpw1", "bf3:bwd-kpw1", "bf3:waves1"]),
    _case("bf3-h96", 8, 18, 96, 2, 1, 2, ["bf3:bwd-kpw2", "bf3:waves3", "bf3:waves6"]),
    _case("bf3-h160", 7, 7, 160, 2, 1, 2, ["bf3:bwd-kpw4", "bf3:waves5"]),
    _case("bf3-h320", 6, 20, 320, 2, 1, 2, ["bf3:fwd-kpw2", "bf3:bwd-kpw8", "bf3:waves5"]),
    _case("bf3-h224", 7, 4, 224, 2, 1, 2, ["bf3:waves7"]),
    _case("bf3-h768", 5, 6, 768, 2, 1, 2, ["bf3:fwd-kpw4", "bf3:bwd-kpw16", "bf3:waves6"]),
    _case("bf3-h1024-t4", 4, 3, 1024, 2, 1, 2, ["bf3:H1024", "bf3:waves8"]),
    _case("bf3-h128-b1", 6, 1, 128, 2, 1, 2, ["bf3:B1"]),
    _case("bf3-h128-b16", 6, 16, 128, 2, 1, 2, ["bf3:B16"]),
    _case("bf3-h128-b17", 6, 17, 128, 2, 1, 2, ["bf3:B17"]),
    _case("bf3-h128-b33", 6, 33, 128, 2, 1, 2, ["bf3:B33"]),
    _case("bf3-h128-b65", 6, 65, 128, 2, 1, 2, ["bf3:B65"]),
    _case("bf3-h1024-b65-path1", 4, 65, 1024, 1, 1, 1, ["bf3:path1"]),
    _case("bf3-h1024-b129-path0", 3, 129, 1024, 1, 1, 0, ["bf3:path0-by-plan"]),
    _case("bf3-state", 9, 17, 64, 2, 1, 2, ["bf3:state"], state=True),
    _case("bf3-dropout", 8, 12, 64, 3, 1, 2, ["bf3:dropout"], extras=["dropout"]),
    _case("bf3-accumulate", 7, 9, 64, 2, 1, 2, ["bf3:accumulate"], extras=["accumulate"]),
    _case("bf3-padding", 9, 20, 64, 2, 1, 2, ["bf3:padding"], extras=["padding"]),
    _case("bf3-per-frame", 6, 21, 128, 2, 1, 0, ["bf3:per-frame"], extras=["per_frame"]),
    _case("bf3-saturating", 8, 10, 64, 2, 1, 2, ["bf3:saturating"], regime="saturating"),
]

# What the matrix has to reach, each with the rule of csrc/lstm_bidir.h (or of the kernels) it comes from
VARIANTS = {
    "f32:H16": "bidir_check: H a multiple of 16; the smallest: two workgroups per direction, one trip of lstm_layer_fwd's K loop",
    "f32:H48": "a hidden size that is no power of two (six workgroups per direction)",
    "f32:H1008": "bidir_plan: nwg = H / 8 = 126, 2 * 126 <= 256 -> path 2; the largest size below 1024",
    "f32:H1024": "bidir_plan: the 144 KiB forward slice; 2 * 128 workgroups = every CU",
    "f32:L3": "bidir_fwd / bidir_bwd: a middle layer reads a 2H-wide input and hands [h_fw ; h_bw] on both ways",
    "f32:B1": "one batch row: 63 of a pass's 64 row slots idle",
    "f32:one-pass": "lstm_layer_fwd / _bwd: for (rb = 0; rb < B; rb += LAYER_ROWS): B = 64 is exactly one pass",
    "f32:second-pass-one-row": "... B = 65: a second pass that holds one row",
    "f32:three-passes": "... B = 130: three passes, the last with two rows",
    "f32:T1": "one frame: the backward kernel never has a next step (has_next false throughout)",
    "lens:0-1-T": "rows of length 0, 1 and T in one batch",
    "f32:lens-short": "no row reaches T: the last frames belong to nobody",
    "f32:lens-ones": "every row one frame long",
    "f32:state": "bidir_fwd: h0 / c0 copied into slot 0 of the forward cells' histories; HFINAL / CFINAL per layer",
    "f32:dropout": "layer_mask in bidir_pack_kernel, the recurrence kernels and bidir_split_kernel",
    "f32:accumulate": "bidir_bwd: gemm_f32(..., accumulate, bias gradient) adds to the caller's dK / db",
    "f32:padding": "bidir_pack_kernel / lstm_layer_bwd mask s >= len: what the caller left past the lengths must not matter",
    "f32:per-frame": "bidir_plan: flags & AMDSPEECH_LSTM_PER_DIAGONAL -> 0, one launch per frame",
    "f32:saturating": "gates in their tails",
    "bf3:fwd-kpw1": "bf3_fwd_kernel: H / 32 <= 8 K blocks", "bf3:fwd-kpw2": "bf3_fwd_kernel: 9..16 K blocks, even",
    "bf3:fwd-kpw4": "bf3_fwd_kernel: 17..32 K blocks, a multiple of 4",
    "bf3:bwd-kpw1": "bf3_bwd_kernel: 4H / 32 <= 8", "bf3:bwd-kpw2": "bf3_bwd_kernel: <= 16, even", "bf3:bwd-kpw4": "bf3_bwd_kernel: <= 32",
    "bf3:bwd-kpw8": "bf3_bwd_kernel: <= 64", "bf3:bwd-kpw16": "bf3_bwd_kernel: <= 128",
    "bf3:waves1": "lbf3_sum over one wave (H = 32 forward)", "bf3:waves3": "three forward waves (H = 96)",
    "bf3:waves5": "five waves (H = 160 both kernels, H = 320 both kernels)", "bf3:waves6": "six waves (H = 96 backward, H = 768 both)",
    "bf3:waves7": "seven waves (H = 224 both kernels)", "bf3:waves8": "eight waves (H = 1024 both kernels)",
    "bf3:H1024": "the largest size: KPW 4 / 16",
    "bf3:B1": "one row of one tile", "bf3:B16": "exactly one 16-row tile", "bf3:B17": "a second tile of one row: mv < MB in both kernels",
    "bf3:B33": "bidir_plan: backward ngrp = 2, its second group holds one tile",
    "bf3:B65": "bidir_plan: forward ngrp = 2 (a fifth tile), backward ngrp = 3",
    "bf3:path1": "bidir_plan: nwg = 1024 / 8 * 2 = 256: 2 * nwg > 256 CUs >= nwg -> one persistent launch per direction",
    "bf3:path0-by-plan": "bidir_plan: nwg = 1024 / 8 * 3 = 384 > 256 CUs -> one launch per frame, chosen by the plan",
    "bf3:state": "pack_rows_bf3_kernel: the initial h, split, into ring slot 0", "bf3:dropout": "layer_mask in the bf16x3 kernels",
    "bf3:accumulate": "bidir_bwd: gemm_reduced(..., accumulate) and colsum_accumulate", "bf3:padding": "as f32:padding",
    "bf3:per-frame": "bidir_plan: the flag, on the bf16x3 kernels (each launch splits its W_hh slice again)",
    "bf3:saturating": "gates in their tails",
}

# Saturating regime (tests/lstm_stack_ref.py): pre-activations with a standard deviation around 4, a fifth of the biases at +-3
SAT_WEIGHT, SAT_BIAS, SAT_BIAS_PINNED = 4.0, 1.0, 3.0
KEEP_IN, KEEP_OUT = 0.8, 0.5
STATE_SIGMA = 0.5


def family(case):
    return (case["precision"], case["regime"])


def info_of(case, lengths):
    return dict(T=case["T"], B=case["B"], H=case["H"], L=case["L"], lengths=np.asarray(lengths), state=bool(case["state"]))


def make_lengths(case):
    T, B = case["T"], case["B"]
    rng = np.random.RandomState(2000 + T + 7 * B)
    if case["lens"] == "full":
        return np.full(B, T, np.int32)
    if case["lens"] == "ones":
        return np.ones(B, np.int32)
    if case["lens"] == "short":
        lengths = rng.randint(1, T, size=B).astype(np.int32)
        lengths[0], lengths[B - 1] = T - 1, 0
        return lengths
    lengths = rng.randint(1, T + 1, size=B).astype(np.int32)
    for pos, val in ((0, T), (1, T - 1), (2, 1), (3, 0)):
        if pos < B:
            lengths[pos] = max(val, 0)
    return lengths


def make_inputs(case):
    """Everything a case feeds the kernels, as float32 CPU tensors (the reference takes the same values in float64)."""
    T, B, H, L = case["T"], case["B"], case["H"], case["L"]
    g = torch.Generator(device="cpu").manual_seed(sum(map(ord, case["name"])))
    sat = case["regime"] == "saturating"
    ks, bs = [], []
    for k in range(2):
        for l in range(L):
            W = H if l == 0 else 2 * H
            ks.append(torch.randn(W + H, 4 * H, generator=g) * ((SAT_WEIGHT if sat else 0.6) / np.sqrt(H)))
            b = torch.randn(4 * H, generator=g) * (SAT_BIAS if sat else 0.1)
            if sat:
                pin = torch.rand(4 * H, generator=g)
                b = torch.where(pin < 0.1, torch.full_like(b, SAT_BIAS_PINNED), torch.where(pin > 0.9, torch.full_like(b, -SAT_BIAS_PINNED), b))
            bs.append(b)
    lengths = make_lengths(case)
    dead = torch.as_tensor(np.arange(T)[:, None] >= lengths[None, :])
    z0 = torch.randn(T, B, H, generator=g)
    z0[dead] = 0.0
    dytop = []
    for _ in range(2):      # dense and non-zero on every valid frame: no gradient slice is empty by accident
        d = torch.randn(T, B, H, generator=g) * 0.1
        d = torch.where(d.abs() < 0.01, torch.full_like(d, 0.01), d)
        d[dead] = 0.0
        dytop.append(d)
    h0 = c0 = None
    if case["state"]:
        h0, c0 = torch.randn(L, B, H, generator=g) * STATE_SIGMA, torch.randn(L, B, H, generator=g) * STATE_SIGMA
    dk0 = db0 = None
    if "accumulate" in case["extras"]:
        dk0, db0 = [torch.randn(k.shape, generator=g) * 0.05 for k in ks], [torch.randn(b.shape, generator=g) * 0.05 for b in bs]
    garbage = (torch.rand(T, B, H, generator=g) - 0.5) * 2e3
    garbage = torch.where(garbage.abs() < 1.0, torch.full_like(garbage, 1e3), garbage)
    return dict(ks=ks, bs=bs, z0=z0, dytop_fw=dytop[0], dytop_bw=dytop[1], lengths=lengths, h0=h0, c0=c0, dk0=dk0, db0=db0,
                garbage=garbage, dead=dead)


def cpu_masks(case):
    """Stand-in multipliers for a "dropout" case where no GPU is at hand (the measurement, the CPU tests): Bernoulli(keep) / keep.
    The GPU test feeds the reference the multipliers the library exports (ops.lstm_bidir_dropout_multipliers) instead."""
    if "dropout" not in case["extras"]:
        return None
    g = torch.Generator(device="cpu").manual_seed(77 + case["T"])
    T, B, H = case["T"], case["B"], case["H"]
    masks = {}
    for d in DIRS:
        for l in range(case["L"]):
            masks[(d, "in", l)] = (torch.rand(T, B, H if l == 0 else 2 * H, generator=g) < KEEP_IN).to(torch.float64) / KEEP_IN
            masks[(d, "out", l)] = (torch.rand(T, B, H, generator=g) < KEEP_OUT).to(torch.float64) / KEEP_OUT
    return masks


def reference(case, inp, masks=None, emulate=None):
    """Outputs and gradients of a case by the reference: dict of y, hT, cT, dK, db, dz0 (dK / db include the initial values of an
    "accumulate" case)."""
    f = call_forward(inp["z0"], inp["ks"], inp["bs"], inp["lengths"], inp["h0"], inp["c0"], masks, emulate)
    r = call_backward(f["cache"], inp["dytop_fw"], inp["dytop_bw"])
    out = {k: f[k] for k in OUTPUT_KINDS}
    out.update(r)
    if inp["dk0"] is not None:
        out["dK"] = [a + b.to(a.dtype) for a, b in zip(out["dK"], inp["dk0"])]
        out["db"] = [a + b.to(a.dtype) for a, b in zip(out["db"], inp["db0"])]
    return out


def emulation(case):
    return {0: "f32", 1: "bf16x3"}[case["precision"]]


def all_slice_errors(got, ref, info):
    return {kind: slice_errors(got[kind], ref[kind], kind, info) for kind in KINDS}


def is_cheap(case):
    """The cases the CPU test measures again (tests/test_cpu_bidir_layer_paths.py)."""
    return case["H"] <= 256 and case["B"] <= 33


# (precision, regime) -> {kind: largest per-slice error of the emulated arithmetic}: the run recorded above.  MEASURED: over every
# case of the family (what bound() uses); MEASURED_CHEAP: over its is_cheap() cases only, of the same run.
MEASURED = {
    (0, 'nominal'): {'y': 2.0e-06, 'hT': 1.2e-06, 'cT': 8.5e-07, 'dK': 2.5e-06, 'db': 2.5e-06, 'dz0': 1.2e-06},
    (0, 'saturating'): {'y': 3.4e-06, 'hT': 1.5e-06, 'cT': 9.5e-07, 'dK': 3.8e-06, 'db': 4.1e-06, 'dz0': 2.8e-06},
    (1, 'nominal'): {'y': 1.7e-05, 'hT': 1.3e-05, 'cT': 9.5e-06, 'dK': 2.2e-05, 'db': 2.9e-05, 'dz0': 1.4e-05},
    (1, 'saturating'): {'y': 5.1e-05, 'hT': 2.7e-05, 'cT': 1.3e-05, 'dK': 7.4e-05, 'db': 1.0e-04, 'dz0': 8.6e-05},
}
MEASURED_CHEAP = {
    (0, 'nominal'): {'y': 4.2e-07, 'hT': 3.3e-07, 'cT': 3.2e-07, 'dK': 1.0e-06, 'db': 1.2e-06, 'dz0': 1.2e-06},
    (0, 'saturating'): {'y': 3.4e-06, 'hT': 1.5e-06, 'cT': 9.5e-07, 'dK': 3.8e-06, 'db': 4.1e-06, 'dz0': 2.8e-06},
    (1, 'nominal'): {'y': 1.5e-05, 'hT': 1.1e-05, 'cT': 9.5e-06, 'dK': 1.4e-05, 'db': 1.5e-05, 'dz0': 1.4e-05},
    (1, 'saturating'): {'y': 5.1e-05, 'hT': 2.7e-05, 'cT': 1.3e-05, 'dK': 7.4e-05, 'db': 1.0e-04, 'dz0': 8.6e-05},
}


def bound(case, kind):
    """The tolerance of a slice of `kind` in `case`: min(cap, FACTOR x measured), see above."""
    cap = CAPS[case["precision"]][0 if kind in OUTPUT_KINDS else 1]
    return min(cap, FACTOR * MEASURED[family(case)][kind])


def measure(cases=None, verbose=False):
    """Runs the emulated arithmetic of every case against float64 and returns the MEASURED dict."""
    table = {}
    for case in (CASES if cases is None else cases):
        inp = make_inputs(case)
        masks = cpu_masks(case)
        ref, emu = reference(case, inp, masks), reference(case, inp, masks, emulate=emulation(case))
        errs = all_slice_errors(emu, ref, info_of(case, inp["lengths"]))
        row = table.setdefault(family(case), {k: 0.0 for k in KINDS})
        for kind, e in errs.items():
            row[kind] = max(row[kind], max(x[1] for x in e))
        if verbose:
            print("  %-24s " % case["name"] + " ".join("%s %.1e" % (k, max(x[1] for x in e)) for k, e in errs.items()), flush=True)
    return table


def _print_dict(name, table):
    print("%s = {" % name)
    for key in sorted(table):
        print("    %r: {%s}," % (key, ", ".join("%r: %.1e" % (k, table[key][k]) for k in KINDS)))
    print("}")


if __name__ == "__main__":
    import time
    t0 = time.time()
    # (two significant digits, as the dicts record them: the bounds are formed from the recorded figures)
    table, cheap = ({key: {k: float("%.1e" % v) for k, v in row.items()} for key, row in t.items()}
                    for t in (measure(verbose=True), measure([c for c in CASES if is_cheap(c)])))
    print()
    _print_dict("MEASURED", table)
    _print_dict("MEASURED_CHEAP", cheap)
    print("\npr %-10s | %s" % ("regime", " | ".join("%-15s" % k for k in KINDS)))
    for key in sorted(table):
        cells = []
        for k in KINDS:
            cap = CAPS[key[0]][0 if k in OUTPUT_KINDS else 1]
            cells.append("%.1e>%.1e%s" % (table[key][k], min(cap, FACTOR * table[key][k]), "c" if FACTOR * table[key][k] > cap else " "))
        print("%d  %-10s | %s" % (key[0], key[1], " | ".join(cells)))
    print("(measured>bound; c: the bound is the cap)   %.0f s" % (time.time() - t0))
