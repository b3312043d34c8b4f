"""float64 reference of the layer-wise bidirectional stack (tf.contrib.rnn.stack_bidirectional_dynamic_rnn over TF
BasicLSTMCell + DropoutWrapper), written as a short torch-autograd cell that takes explicit dropout masks.  Checker only."""
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
