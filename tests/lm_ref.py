"""Checker for the language-model kernels (csrc/lm.hip): float64 numpy references, the rounding bounds as formulas, and the
case tables.  Never imported by the product.

Conventions (include/amdspeech.h, "language model"): tokens int32 [B][ld], position (t, b) reads tok[b, t]; a position is inside
its row when t < lengths[b]; time-major activations [T][B][.].

Rounding bounds, u = 2**-24 (float32 unit round-off), M = max |logit| of the row, C classes.

embed_fwd   exact: one correctly rounded float32 addition w + bias (the float32 rounding of the float64 sum is that number).

embed_bwd   an element of dw is dw0 + t_1 + ... + t_k summed in SOME order in float32: n = k + 1 terms, n - 1 additions.  Any
            order of n - 1 additions satisfies |computed - exact| <= gamma_(n-1) * sum|terms| <= n u / (1 - n u) * sum|terms|
            (Higham, Accuracy and Stability, 4.2), the form noise_reverb_ref.py uses for its L-term sums.

xent nll    d_i = fl(x_i - m) is off by at most u |x_i - m| <= 2 M u, so e_i = fl(exp(d_i)) = exp(x_i - m) (1 + a), |a| <= (2 M + E) u
            with E u the relative error of the exp implementation (E = 4: two ulp; the device's and numpy's float32 exp are
            within one).  s = fl(sum e_i), C - 1 additions in any order of non-negative terms: relative error <= (2 M + E + C) u.
            fl(log s) = log S + b, |b| <= (2 M + E + C) u + E u ln C  (1 <= S <= C, the log implementation within E u relative).
            lse = fl(m + log s): + u |lse| <= u (M + ln C).   nll = fl(lse - x_t): + u |nll| <= u (2 M + ln C).
            Sum: u (5 M + C + (E + 2) ln C + E), first order; the second-order terms are covered by dividing by 1 - (2 M + C + E) u.

xent dlogits  p_i = fl(e_i / s) = P_i (1 + c), |c| <= (2 M + E) u + (2 M + E + C) u + u.  g = fl(p_i - onehot): + u |g|;
            fl(scale g): + u |scale g|.  With P_i <= 1 and |P_i - onehot| <= 1:  |error| <= |scale| u (4 M + C + 2 E + 3) per element,
            and summed over a row (sum P_i = 1, sum |P_i - onehot| <= 2):  |sum_c dlogits| <= |scale| u (4 M + C + 2 E + 5), the exact
            sum being 0.  An e_i or p_i below the smallest normal float32 may be flushed to 0: + |scale| 2**-126 per element.
"""
import numpy as np

from oracle import model as om

U = 2.0 ** -24
E_LIBM = 4.0
TINY = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------------------- embed
def live_positions(lengths, T):
    """bool [T, B]: t < lengths[b]."""
    return np.arange(T)[:, None] < np.asarray(lengths)[None, :]


def embed_fwd_ref(tok, lengths, T, w, bias):
    """float64 out [T, B, H]; its float32 rounding is what the kernel must return, bit for bit."""
    tok = np.asarray(tok)
    B, (V, H) = tok.shape[0], w.shape
    ids = tok[:, :T].T                                              # [T, B]
    hit = live_positions(lengths, T) & (ids >= 0) & (ids < V)
    out = np.zeros((T, B, H), np.float64)
    out[hit] = w.astype(np.float64)[ids[hit]]
    if bias is not None:
        out += bias.astype(np.float64)
    return out


def embed_bwd_ref(tok, lengths, T, dz, V):
    """The sums embed_bwd ADDS: (dw [V, H], dbias [H]) in float64, the sums of |terms| (same shapes) and the term counts
    (n_dw [V], n_db scalar) for the bound."""
    tok = np.asarray(tok)
    H = dz.shape[2]
    ids = tok[:, :T].T
    live = live_positions(lengths, T)
    d = dz.astype(np.float64)
    dw = np.zeros((V, H)); aw = np.zeros((V, H)); n_dw = np.zeros(V, np.int64)
    for v in range(V):
        sel = live & (ids == v)
        dw[v] = d[sel].sum(0); aw[v] = np.abs(d[sel]).sum(0); n_dw[v] = sel.sum()
    return dw, d[live].sum(0), aw, np.abs(d[live]).sum(0), n_dw, int(live.sum())


def sum_bound(n_terms, abs_sum):
    """n-term float32 sum in any order: n u / (1 - n u) * sum|terms| (module docstring); n_terms and abs_sum broadcast."""
    n = np.asarray(n_terms, np.float64)
    return n * U / (1.0 - n * U) * abs_sum


# ----------------------------------------------------------------------------------------------------------------- xent
def xent_live(targets, lengths, T, C):
    tg = np.asarray(targets)[:, :T].T
    return live_positions(lengths, T) & (tg >= 0) & (tg < C)


def xent_ref(logits, targets, lengths, scale):
    """float64 (nll [T, B], dlogits [T, B, C], live [T, B]); dead positions are zero."""
    T, B, C = logits.shape
    x = logits.astype(np.float64)
    tg = np.asarray(targets)[:, :T].T
    live = xent_live(targets, lengths, T, C)
    m = x.max(axis=2, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=2, keepdims=True)
    lse = (m + np.log(s))[..., 0]
    safe = np.where(live, tg, 0)
    xt = np.take_along_axis(x, safe[..., None], axis=2)[..., 0]
    nll = np.where(live, lse - xt, 0.0)
    g = e / s
    np.put_along_axis(g, safe[..., None], np.take_along_axis(g, safe[..., None], axis=2) - 1.0, axis=2)
    return nll, np.where(live[..., None], float(scale) * g, 0.0), live


def xent_f32(logits, targets, lengths, scale, variant="right"):
    """The same formulas evaluated in float32 numpy, operation by operation as the kernel does them (the bounds must hold for it),
    and two deliberately WRONG variants the bounds must reject:
      "no_max":    softmax without the maximum subtracted, nll = -log(p[target]) -- exp(-80) / exp(80) is 0 in float32
      "c_minus_1": the softmax taken over the first C - 1 classes only."""
    T, B, C = logits.shape
    f = np.float32
    x = logits.astype(f)
    tg = np.asarray(targets)[:, :T].T
    live = xent_live(targets, lengths, T, C)
    safe = np.where(live, tg, 0)[..., None]
    onehot = np.zeros((T, B, C), f)
    np.put_along_axis(onehot, safe, f(1), axis=2)
    with np.errstate(all="ignore"):
        if variant == "no_max":
            e = np.exp(x)
            p = e / e.sum(axis=2, keepdims=True, dtype=f)
            nll = -np.log(np.take_along_axis(p, safe, axis=2))[..., 0]
        else:
            xs = x[..., :C - 1] if variant == "c_minus_1" else x
            m = xs.max(axis=2, keepdims=True)
            e = np.exp(x - m)
            if variant == "c_minus_1":
                e[..., C - 1] = 0
            s = e.sum(axis=2, keepdims=True, dtype=f)
            p = e / s
            nll = ((m + np.log(s)) - np.take_along_axis(x, safe, axis=2))[..., 0]
        g = f(scale) * (p - onehot)
    return np.where(live, nll, f(0)).astype(f), np.where(live[..., None], g, f(0)).astype(f)


def _second_order(C, M):
    return 1.0 - (2.0 * M + C + E_LIBM) * U


def nll_bound(C, M):
    """|nll_f32 - nll_exact| for a row of C logits with max |logit| M (module docstring)."""
    return U * (5.0 * M + C + (E_LIBM + 2.0) * np.log(C) + E_LIBM) / _second_order(C, M)


def dlogits_bound(C, M, scale):
    """... for one element of dlogits."""
    return abs(scale) * (U * (4.0 * M + C + 2.0 * E_LIBM + 3.0) / _second_order(C, M) + TINY)


def dlogits_rowsum_bound(C, M, scale):
    """... for the sum of a live row of dlogits (exactly 0 in exact arithmetic), the sum itself taken in float64."""
    return abs(scale) * (U * (4.0 * M + C + 2.0 * E_LIBM + 5.0) / _second_order(C, M) + C * TINY)


def loss_rule(nll32):
    """loss[b]: the float32 rounding of the float64 sum, in increasing t, of the float32 nll[t][b] -- exactly."""
    acc = np.zeros(nll32.shape[1], np.float64)
    for t in range(nll32.shape[0]):
        acc = acc + nll32[t].astype(np.float64)
    return acc.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- case tables
XENT_T, XENT_B = 5, 3
XENT_C_FIXED = (2, 63, 64, 65, 80, 128, 129)
XENT_C_MAX = 4096


def xent_class_counts(plan):
    """The fixed C of the table plus one C on each side of every boundary the plan query reports up to 4096.  `plan(T, B, C)`
    returns a dict with c_min / c_max (ops.xent_plan): the range of C that takes the same kernel instantiation."""
    cs = set(XENT_C_FIXED)
    c = 2
    while c <= XENT_C_MAX:
        hi = plan(XENT_T, XENT_B, c)["c_max"]
        assert hi >= c, (c, hi)
        cs.add(min(hi, XENT_C_MAX))
        if hi + 1 <= XENT_C_MAX:
            cs.add(hi + 1)
        c = hi + 1
    cs.add(XENT_C_MAX)
    return sorted(cs)


def xent_case(C, ld, kind, seed=0):
    """One case at T 5, B 3: rows of lengths {T, 1, 0}; `kind` is "normal" (logits ~ N(0, 1)), "pm80" (entries at +-80, the
    target of position (0, 0) at -80 beside a +80) or "equal" (position (1, 0) a row of all-equal values).  Row 0 carries a
    target of -1 at t = 2 and a target of C at t = 3: dead positions inside a live row."""
    T, B = XENT_T, XENT_B
    rng = np.random.RandomState(1000 * C + 10 * ld + seed)
    logits = rng.randn(T, B, C).astype(np.float32)
    targets = rng.randint(0, C, size=(B, ld)).astype(np.int32)
    if kind == "pm80":
        sign = np.where(rng.rand(T, B, C) < 0.5, -1.0, 1.0)
        where = rng.rand(T, B, C) < 0.5
        logits = np.where(where, 80.0 * sign, logits).astype(np.float32)
        logits[0, 0, :] = rng.randn(C)
        logits[0, 0, 0] = -80.0
        logits[0, 0, C - 1] = 80.0
        targets[0, 0] = 0
    elif kind == "equal":
        logits[1, 0, :] = 0.75
    else:
        assert kind == "normal"
    targets[0, 2] = -1
    targets[0, 3] = C
    lengths = np.array([T, 1, 0], np.int32)
    return dict(C=C, ld=ld, kind=kind, logits=logits, targets=targets, lengths=lengths)


def xent_cases(plan):
    out = []
    for C in xent_class_counts(plan):
        for ld in (XENT_T + 1, XENT_T + 4):
            for kind in ("normal", "pm80", "equal"):
                out.append(xent_case(C, ld, kind))
    return out


EMBED_SHAPES = ((1, 16), (80, 16), (80, 48), (80, 528), (300, 128))      # (V, H)


def embed_case(V, H, T=7, B=3, skew=False, seed=0):
    """tokens, lengths, w, bias, dz for one case.  Regular cases: lengths {T, 0, T - 2}, ids drawn from the lower half of the
    alphabet (the upper half never occurs), one id of -1 and one of V inside live rows.  skew: EVERY id equal, every row full."""
    rng = np.random.RandomState(7919 * V + 31 * H + T + seed)
    ld = T + 1
    if skew:
        tok = np.full((B, ld), min(3, V - 1), np.int32)
        lengths = np.full(B, T, np.int32)
    else:
        tok = rng.randint(0, max(V // 2, 1), size=(B, ld)).astype(np.int32)
        tok[0, 1] = -1
        tok[2, 2] = V
        lengths = np.array([T, 0, T - 2], np.int32)[:B]
    w = rng.randn(V, H).astype(np.float32)
    bias = rng.randn(H).astype(np.float32)
    dz = rng.randn(T, B, H).astype(np.float32)
    return dict(V=V, H=H, T=T, B=B, tok=tok, lengths=lengths, w=w, bias=bias, dz=dz, skew=skew)


def embed_cases():
    return [embed_case(V, H) for V, H in EMBED_SHAPES] + [embed_case(80, 48, T=40, B=16, skew=True)]


# ------------------------------------------------------------------------------------------------------- the LM oracle
def lm_oracle_loss_and_grads(p, tok, lengths, L, in_masks=None, out_masks=None):
    """The language-model step restated with the acoustic oracle: one-hot rows (zero past a row's length) through
    oracle.model.forward, lm_ref's cross-entropy against tok[:, 1:], oracle.model.backward.  Returns (loss [B], logits, grads)."""
    V = p["input_w"].shape[0]
    T = int(np.max(lengths))
    B = tok.shape[0]
    x = np.zeros((T, B, V), p["input_w"].dtype)
    for b in range(B):
        for t in range(int(lengths[b])):
            x[t, b, tok[b, t]] = 1.0
    logits, _, cache = om.forward(p, x, lengths, L, keep_cache=True, in_masks=in_masks, out_masks=out_masks)
    nll, dlogits, _ = xent_ref(logits, tok[:, 1:], lengths, 1.0)
    grads = om.backward(p, cache, dlogits, lengths, L, in_masks=in_masks, out_masks=out_masks)
    return nll.sum(axis=0), logits, grads
