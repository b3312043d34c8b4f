"""Float64 numpy reference of the strided time-frequency convolution in front of the input Linear (include/amdspeech.h,
"time-frequency convolution (front)"), the case table of its tests, the error bounds of the float32 kernels -- derived from the
arithmetic the header states, not tuned -- and the model-level oracle: oracle.model on the reference convolution's output with
model lengths (oracle/ itself is unchanged).

    x [T,B,G*F], w [K = G kt kf, C] (row k = (g kt + i) kf + j), bias [C];  pt = (kt-1)/2, pf = (kf-1)/2
    T' = ceil(T / st), F' = ceil(F / sf), Lb = min(max(lengths[b], 0), T), L'b = ceil(Lb / st)
    pre[t',b,f',c] = bias[c] + sum_{g,i,j} w[k,c] x[t' st + i - pt, b, g, f' sf + j - pf]     (frame in 0 .. Lb-1, bin in 0 .. F-1)
    y[t',b,f' C + c] = min(max(pre, 0), 20) for t' < L'b, 0 past it
    dw[k,c] = sum_{t' < L'b, b, f'} patch_k dy mask,  db[c] = sum dy mask,  mask = 0 < y < 20
"""
import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of float32
CLIP = 20.0


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for float32."""
    return n * U32 / (1.0 - n * U32)


def out_dims(T, F, st, sf):
    return -(-T // st), -(-F // sf)


def clip_lengths(lengths, T):
    return np.clip(np.asarray(lengths, np.int64), 0, T)


def model_lengths(lengths, T, st):
    return -(-clip_lengths(lengths, T) // st)


def patches(x, lengths, G, F, kt, kf, st, sf, absolute=False):
    """P [T',B,F',K] float64: the source value behind every (output position, k), 0 where the source frame lies outside the row or
    the source bin outside 0 .. F-1.  Frames at or past a row's length are replaced, not multiplied: they may hold NaN."""
    T, B, D = x.shape
    assert D == G * F
    To, Fo = out_dims(T, F, st, sf)
    pt, pf = (kt - 1) // 2, (kf - 1) // 2
    live = np.arange(T)[:, None] < clip_lengths(lengths, T)[None, :]
    xm = np.where(live[:, :, None], np.asarray(x, np.float64), 0.0).reshape(T, B, G, F)
    if absolute:
        xm = np.abs(xm)
    xp = np.zeros(((To - 1) * st + kt, B, G, (Fo - 1) * sf + kf))
    nt, nf = min(T, xp.shape[0] - pt), min(F, xp.shape[3] - pf)
    xp[pt:pt + nt, :, :, pf:pf + nf] = xm[:nt, :, :, :nf]
    P = np.zeros((To, B, Fo, G, kt, kf))
    for i in range(kt):
        for j in range(kf):
            P[:, :, :, :, i, j] = xp[i:i + (To - 1) * st + 1:st, :, :, j:j + (Fo - 1) * sf + 1:sf].transpose(0, 1, 3, 2)
    return P.reshape(To, B, Fo, G * kt * kf)


def forward(x, w, bias, lengths, G, F, kt, kf, st, sf, absolute=False):
    """(y [T',B,F'*C], pre [T',B,F',C]).  absolute: pre is sum |w x| + |bias|, what the forward bound multiplies (y is then
    meaningless and None)."""
    T, B, _ = x.shape
    w, bias = np.asarray(w, np.float64), np.asarray(bias, np.float64)
    P = patches(x, lengths, G, F, kt, kf, st, sf, absolute=absolute)
    if absolute:
        return None, P @ np.abs(w) + np.abs(bias)
    pre = P @ w + bias
    To, _, Fo, C = pre.shape
    live = np.arange(To)[:, None] < model_lengths(lengths, T, st)[None, :]
    y = np.where(live[:, :, None, None], np.clip(pre, 0.0, CLIP), 0.0)
    return y.reshape(To, B, Fo * C), pre


def mask_of(y):
    """The activation's mask as the kernel reads it from y (NaN past the lengths compares false)."""
    with np.errstate(invalid="ignore"):
        return (y > 0.0) & (y < CLIP)


def backward(x, y, dy, lengths, G, F, kt, kf, st, sf, absolute=False, mask=None):
    """(dw [K,C], db [C]) with the mask taken from y (or given as [T',B,F'*C] booleans).  absolute: the sums of |terms|."""
    T, B, _ = x.shape
    P = patches(x, lengths, G, F, kt, kf, st, sf, absolute=absolute)
    To, _, Fo, K = P.shape
    C = np.shape(dy)[2] // Fo
    live = np.arange(To)[:, None] < model_lengths(lengths, T, st)[None, :]
    m = (mask_of(np.asarray(y)) if mask is None else np.asarray(mask, bool)) & live[:, :, None]
    gm = np.where(m, np.asarray(dy, np.float64), 0.0).reshape(To, B, Fo, C)
    if absolute:
        gm = np.abs(gm)
    return P.reshape(-1, K).T @ gm.reshape(-1, C), gm.sum(axis=(0, 1, 2))


# ---- bounds.  Every pre is ONE float32 accumulation chain over the k_pad products (the matrix core's fused multiply-adds: one
# rounding per step, the padded steps and the steps outside the row add exact zeros) and one add of the bias: at most k_pad + 1
# roundings on the way of any term, so |err| <= gamma_{k_pad+1} (sum |w x| + |bias|) (Higham, Accuracy and Stability, 3.1).  The
# clip is 1-Lipschitz: the same bound holds for y.
def fwd_bound(abs_pre, k_pad):
    return gamma(k_pad + 1) * np.asarray(abs_pre, np.float64)


def dw_tree_depth(plan):
    """Roundings on the way of any one term of dw / db through the summation the plan describes: the partial's chain over dw_terms
    positions, the slice's sum of reduce_terms partials, the sum of reduce_slices slices, and the add into the pre-filled output."""
    return plan["dw_terms"] + plan["reduce_terms"] + plan["reduce_slices"] + 1


def dw_bound(abs_terms, dw0, plan, n_terms):
    """|dw - (dw0 + sum)| <= gamma_d (sum |terms| + |dw0|), d the smaller of the tree's depth and N + 1 -- the ceiling that ANY order
    of N terms and the pre-filled value meets."""
    d = min(dw_tree_depth(plan), int(n_terms) + 1)
    return gamma(d) * (np.asarray(abs_terms, np.float64) + np.abs(np.asarray(dw0, np.float64)))


# ---- cases (T, B, G, F, C, kt, kf, st, sf) of tests/test_gpu_conv_front.py; the tile-edge case is built from the plan there
CASES = [
    (1, 1, 1, 16, 16, 1, 1, 1, 1),             # pointwise
    (5, 2, 1, 13, 16, 11, 21, 1, 1),           # window larger than the input both ways
    (23, 3, 3, 40, 32, 11, 21, 2, 2),          # fbank groups, odd T, K = 693: K padding is live
    (17, 2, 1, 20, 48, 3, 5, 3, 1),            # T % st != 0, three channel blocks
    (16, 5, 1, 40, 64, 5, 3, 4, 4),            # stride 4 both ways
    (40, 33, 3, 40, 32, 11, 21, 2, 2),         # several tiles, odd B
]
# the key limits, for the plan table (no kernel runs at these)
LIMIT_CASES = [
    (1001, 32, 3, 40, 64, 11, 41, 1, 1),
    (1001, 32, 3, 40, 64, 11, 41, 4, 4),
    (998, 64, 3, 40, 32, 11, 21, 2, 2),
    (1001, 32, 3, 128, 32, 11, 41, 4, 1),
    (1001, 32, 1, 128, 16, 1, 1, 1, 1),
    (2000, 1, 1, 20, 64, 11, 41, 1, 1),
]


def length_sets(T, B, kt, st, rng, extra=()):
    """Lists of B lengths that together hold 0, 1, st, st + 1, pt, pt + 1, T (those that do not exceed T) and `extra`; the rest is
    random in 0 .. T.  As many sets as it takes at this B."""
    pt = (kt - 1) // 2
    must = []
    for v in [0, 1, st, st + 1, pt, pt + 1, T] + list(extra):
        if 0 <= v <= T and v not in must:
            must.append(int(v))
    sets = []
    while must:
        take, must = must[:B], must[B:]
        take = take + [int(v) for v in rng.randint(0, T + 1, size=B - len(take))]
        sets.append(np.asarray(take, np.int32))
    return sets


def case_data(case, rng):
    """Float32 (x, w, bias, dy, dw0, db0) of a case: pre-activations of unit scale, a bias that pushes a share of them past the
    clip at 20 and below 0, so both kinks are live."""
    T, B, G, F, C, kt, kf, st, sf = case
    K = G * kt * kf
    To, Fo = out_dims(T, F, st, sf)
    x = rng.randn(T, B, G * F).astype(np.float32)
    w = (rng.randn(K, C) * (4.0 / np.sqrt(K))).astype(np.float32)
    bias = (rng.randn(C) * 4.0 + 8.0).astype(np.float32)
    dy = rng.randn(To, B, Fo * C).astype(np.float32)
    return x, w, bias, dy, rng.randn(K, C).astype(np.float32), rng.randn(C).astype(np.float32)


# ---- the model-level oracle
CONV_MODEL = (32, 11, 21, 2, 2, 3)            # (C, kt, kf, st, sf, G): fbank-shaped input
# name, L, H, B, T_in, U, mode ("plain" | "lookahead" | "bidirectional"), dropout on, seed
MODEL_CONFIGS = [
    ("plain_128", 2, 128, 4, 40, 6, "plain", False, 11),
    ("plain_256", 2, 256, 5, 70, 8, "plain", False, 12),
    ("dropout_128", 2, 128, 5, 55, 6, "plain", True, 13),
    ("lookahead_128", 2, 128, 4, 47, 6, "lookahead", False, 14),
    ("bidirectional_128", 2, 128, 4, 41, 6, "bidirectional", False, 15),
]
LOOKAHEAD_CONTEXT = 3
NUM_LABELS = 30
UNDECIDED_SHARE = 1e-3


def model_batch(cfg):
    """(x [T_in,B,120] float32, source lengths, dense labels) of a model config: ragged lengths in T_in/2 .. T_in with one empty row,
    labels that fit the MODEL length."""
    _, L, H, B, T, U, mode, _, seed = cfg
    st = CONV_MODEL[3]
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, CONV_MODEL[5] * 40).astype(np.float32)
    lengths = rng.randint(T // 2, T + 1, size=B).astype(np.int32)
    lengths[0] = T
    lengths[1] = 0
    dense = np.zeros((B, U), np.int32)
    for b in range(B):
        n = rng.randint(1, max(2, min(U - 1, int(-(-lengths[b] // st)) // 3 + 1)))
        dense[b, :n] = rng.randint(1, NUM_LABELS - 1, size=n)
        dense[b, n] = NUM_LABELS - 1
    return x, lengths, dense


def conv_params(cfg):
    """Float32 (conv_w, conv_b) of a model config: Glorot-uniform over the receptive field, a small random bias."""
    C, kt, kf, _, _, G = CONV_MODEL
    rng = np.random.RandomState(cfg[-1] + 1000)
    K = G * kt * kf
    lim = np.sqrt(6.0 / (K + kt * kf * C))
    return ((rng.rand(K, C) * 2.0 - 1.0) * lim).astype(np.float32), (rng.randn(C) * 0.1).astype(np.float32)


def undecided(pre, abs_pre, k_pad):
    """Outputs whose float64 pre lies within the forward bound of a kink of the activation: a float32 forward may land on either
    side there, and only there."""
    b = fwd_bound(abs_pre, k_pad)
    return (np.abs(pre) <= b) | (np.abs(pre - CLIP) <= b)


def oracle_mask(pre, abs_pre, k_pad, y_dev, lengths, T, st):
    """The mask the oracle differentiates with: from the float64 pre where that is decided, from the device's y where it is not.
    Returns (mask [T',B,F'*C], undecided, live) and asserts what the issue sets: the two masks differ only on undecided elements,
    and those are at most UNDECIDED_SHARE of the live outputs."""
    To, B, Fo, C = pre.shape
    live = np.broadcast_to((np.arange(To)[:, None] < model_lengths(lengths, T, st)[None, :])[:, :, None, None], pre.shape)
    und = undecided(pre, abs_pre, k_pad) & live
    m64 = (pre > 0.0) & (pre < CLIP) & live
    mdev = mask_of(np.asarray(y_dev, np.float64)).reshape(pre.shape) & live
    assert not ((m64 != mdev) & ~und).any(), "the device's mask differs from the float64 one on a decided element"
    assert und.sum() <= UNDECIDED_SHARE * max(int(live.sum()), 1), (int(und.sum()), int(live.sum()))
    return np.where(und, mdev, m64).reshape(To, B, Fo * C), und, live


def model_oracle(run, p64, x, lengths, k_pad, y_dev):
    """The float64 oracle of the model with the convolution in front.  `run(p, x_model, model_lengths) -> (logits, loss, grads)` is
    an UNCHANGED oracle of the model behind it (oracle.model, or tests/lookahead_ref.model_oracle around it).  dZ_0 is recovered
    from that oracle's own input_w gradient: the model input is widened by the T'B x T'B identity and input_w by as many ZERO rows
    -- the forward pass is the same function, and the widened gradient's extra rows are I^T dZ_0 = dZ_0.
    p64 holds "conv_w" / "conv_b" beside the oracle's own tensors; y_dev is the device's y, read only where the float64 pre is
    undecided (oracle_mask).  Returns (logits, loss, gradients by name with conv_w / conv_b, y, model lengths)."""
    C, kt, kf, st, sf, G = CONV_MODEL
    T, B, D = x.shape
    F = D // G
    y, pre = forward(x, p64["conv_w"], p64["conv_b"], lengths, G, F, kt, kf, st, sf)
    _, abs_pre = forward(x, p64["conv_w"], p64["conv_b"], lengths, G, F, kt, kf, st, sf, absolute=True)
    Lo = model_lengths(lengths, T, st).astype(np.int32)
    To, _, W = y.shape
    base = {k: v for k, v in p64.items() if k not in ("conv_w", "conv_b")}
    wide = dict(base, input_w=np.concatenate([base["input_w"], np.zeros((To * B, base["input_w"].shape[1]))]))
    x_wide = np.concatenate([y, np.eye(To * B).reshape(To, B, To * B)], axis=2)
    logits, loss, g = run(wide, x_wide, Lo)
    dz0 = g["input_w"][W:]
    g = dict(g, input_w=g["input_w"][:W])
    dy = (dz0 @ base["input_w"].T).reshape(To, B, W)
    mask, _, _ = oracle_mask(pre, abs_pre, k_pad, y_dev, lengths, T, st)
    g["conv_w"], g["conv_b"] = backward(x, None, dy, lengths, G, F, kt, kf, st, sf, mask=mask)
    return logits, loss, g, y, Lo
