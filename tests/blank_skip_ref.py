"""Checker for blank-frame skipping (csrc/ctc_blank_skip.hip): the float64 numpy reference of the semantics in include/amdspeech.h
("blank-frame skipping"), the rounding bound as a formula, a float32 emulation of the kernels' arithmetic with planted faults, the case
table, and seeded "peaky" posteriors for the decoder-invariance tests.  Never imported by the product.

Semantics.  Blank is class C-1; n_b = min(max(lengths[b], 0), T);
    lpb[t]  = (x[C-1] - max_c x[c]) - log(sum_c exp(x[c] - max))        x = logits[t][b]
    skip[t] = t < n_b and lpb[t] >= log(theta)       (a NaN compares false: the frame is kept)
    keep[t] = t < n_b and not (skip[t] and t > 0 and skip[t-1])         of every run of skippable frames the FIRST stays
and the kept frames move to the front of out_logits in order, zeros behind them; src_frame holds their source frames, -1 behind.

Rounding bound, u = 2**-24 (float32 unit round-off), M = max |logit| of the frame, C classes, in the manner of lm_ref's nll bound.
    d_i = fl(x_i - m) is off by at most u |x_i - m| <= 2 M u, so e_i = fl(exp(d_i)) = exp(x_i - m) (1 + a), |a| <= (2 M + E) u with
    E u the relative error of the exp implementation (E = 4: two ulp).  s = fl(sum e_i): C - 1 additions in ANY order of
    non-negative terms, each in (0, 1] or flushed to 0, the largest exactly 1: relative error <= (2 M + E + C) u.
    fl(log s) = log S + b, |b| <= (2 M + E + C) u + E u ln C   (1 <= S <= C, the log implementation within E u relative).
    fl(x_blank - m): + u |x_blank - m| <= 2 M u.   lpb = fl(that - log s): + u |lpb| <= u (2 M + ln C).
    Sum: u (6 M + C + (E + 1) ln C + E), first order; the second-order terms are covered by dividing by 1 - (2 M + C + E) u.

Decided frames.  Every frame of the table with t < n_b is DECIDED: whichever kernel stays inside the bound takes the same skip
decision as float64.  A frame is decided when
    (a) its float64 lpb lies at least MARGIN = 100 bounds away from log(theta), or it holds a NaN (lpb is NaN in any arithmetic: kept), or
    (b) its blank logit is at least 80 above every other logit.  Then x_blank - m is exactly 0, every other exp is below 2**-115, the sum
        is exactly 1 in float32 and in float64 whatever the order, its log exactly 0 and lpb exactly 0 >= log(theta) for every
        theta <= 1: skippable in any arithmetic.  This is how a table can hold theta = 1 (log(theta) = 0, reached only by equality).
The share of undecided frames allowed is zero (undecided()).
"""
import numpy as np

U = 2.0 ** -24
E_LIBM = 4.0
MARGIN = 100.0
EXACT_DOMINANCE = 80.0


def lpb_bound(C, M):
    """|lpb_f32 - lpb_f64| for a frame of C logits with max |logit| M (module docstring)."""
    return U * (6.0 * M + C + (E_LIBM + 1.0) * np.log(C) + E_LIBM) / (1.0 - (2.0 * M + C + E_LIBM) * U)


def clip_lengths(lengths, T):
    return np.clip(np.asarray(lengths, np.int64), 0, T)


# ------------------------------------------------------------------------------------------------------------ reference
def blank_logp_ref(logits, lengths):
    """float64 lpb [T][B]; 0 at t >= n_b (the call's blank_logp output)."""
    x = np.asarray(logits, np.float64)
    T, B, C = x.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax.reduce(x, axis=2)                                     # (the maximum ignores a NaN, as fmaxf does)
        lpb = (x[:, :, C - 1] - m) - np.log(np.sum(np.exp(x - m[:, :, None]), axis=2))
    live = np.arange(T)[:, None] < clip_lengths(lengths, T)[None, :]
    return np.where(live, lpb, 0.0)


def keep_from_skip(skip, n):
    """The run rule on one utterance: skip bool [T], n frames -> keep bool [T]."""
    T = len(skip)
    keep = np.zeros(T, bool)
    for t in range(min(n, T)):
        keep[t] = not (skip[t] and t > 0 and skip[t - 1])
    return keep


def compact(logits, keep):
    """logits [T,B,C] and keep bool [T,B] -> (out_logits, out_lengths int32 [B], src_frame int32 [B,T]); bit copies."""
    T, B, C = logits.shape
    out = np.zeros_like(logits)
    src = np.full((B, T), -1, np.int32)
    n_out = np.zeros(B, np.int32)
    for b in range(B):
        ts = np.flatnonzero(keep[:, b])
        out[:len(ts), b] = logits[ts, b]
        src[b, :len(ts)] = ts
        n_out[b] = len(ts)
    return out, n_out, src


def blank_skip_ref(logits, lengths, theta):
    """The whole call in float64 decisions: dict(blank_logp float64 [T,B], skip, keep bool [T,B], out_logits, out_lengths, src_frame)."""
    logits = np.asarray(logits, np.float32)
    T, B, C = logits.shape
    n = clip_lengths(lengths, T)
    lpb = blank_logp_ref(logits, lengths)
    live = np.arange(T)[:, None] < n[None, :]
    with np.errstate(invalid="ignore"):
        skip = live & (lpb >= np.log(np.float64(theta)))
    keep = np.stack([keep_from_skip(skip[:, b], int(n[b])) for b in range(B)], axis=1)
    out, n_out, src = compact(logits, keep)
    return dict(blank_logp=lpb, skip=skip, keep=keep, out_logits=out, out_lengths=n_out, src_frame=src)


def undecided(logits, lengths, theta):
    """Frames with t < n_b that are NOT decided (module docstring): bool [T,B].  The table must hold none."""
    x = np.asarray(logits, np.float64)
    T, B, C = x.shape
    lpb = blank_logp_ref(logits, lengths)
    live = np.arange(T)[:, None] < clip_lengths(lengths, T)[None, :]
    with np.errstate(invalid="ignore"):
        M = np.nanmax(np.abs(x), axis=2)
        far = np.abs(lpb - np.log(np.float64(theta))) >= MARGIN * lpb_bound(C, M)
        others = np.max(x[:, :, :C - 1], axis=2)
        exact = (x[:, :, C - 1] - others >= EXACT_DOMINANCE) & (lpb == 0.0)
    return live & ~(far | exact | np.isnan(lpb))


# ------------------------------------------------------------------------------------- float32 emulation of the kernels
FAULTS = ("keep_last", "seam_reset", "count_past_length", "gt_not_ge", "tail_not_zeroed")


def _butterfly(v, op):
    """v float32 [R, waves, 64]: the 32-16-8-4-2-1 xor butterfly of every wave; every lane ends with the wave's value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[:, :, lane ^ o]).astype(np.float32)
    return v


def blank_logp_f32(logits, lengths, words_per_lane, threads_per_row, vec):
    """lpb in float32 numpy, operation by operation and in the kernels' order (ctc_blank_skip.hip: bs_rows_kernel): lane l of the
    threads_per_row lanes holds the units l, l + TPR, ... (a unit: `vec` consecutive words), takes its maximum and adds its
    exponentials in increasing c, the lanes of a wave meet in the butterfly, the waves in wave order."""
    f = np.float32
    x = np.asarray(logits, f)
    T, B, C = x.shape
    R, tpr, wpl = T * B, threads_per_row, words_per_lane
    assert wpl * tpr >= C and (vec == 1 or C % 4 == 0)
    pad = np.full((R, wpl * tpr), -np.inf, f)
    pad[:, :C] = x.reshape(R, C)
    c = np.arange(wpl * tpr)
    unit = c // vec
    lane, slot = unit % tpr, (unit // tpr) * vec + c % vec
    held = np.empty((R, tpr, wpl), f)
    held[:, lane, slot] = pad
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.full((R, tpr), -np.inf, f)
        for i in range(wpl):
            m = np.fmax(m, held[:, :, i])
        m = _butterfly(m.reshape(R, tpr // 64, 64), np.fmax)[:, :, 0]
        mm = m[:, 0]
        for k in range(1, tpr // 64):
            mm = np.fmax(mm, m[:, k])
        s = np.zeros((R, tpr), f)
        for i in range(wpl):
            e = np.exp((held[:, :, i] - mm[:, None]).astype(f)).astype(f)
            s = (s + np.where(held[:, :, i] == -np.inf, f(0), e)).astype(f)
        s = _butterfly(s.reshape(R, tpr // 64, 64), np.add)[:, :, 0]
        ss = s[:, 0]
        for k in range(1, tpr // 64):
            ss = (ss + s[:, k]).astype(f)
        lpb = ((pad[:, C - 1] - mm).astype(f) - np.log(ss).astype(f)).astype(f)
    live = np.arange(T)[:, None] < clip_lengths(lengths, T)[None, :]
    return np.where(live, lpb.reshape(T, B), f(0)).astype(f)


def blank_skip_f32(logits, lengths, theta, plan, fault=None):
    """The whole call as the kernels do it (rows in float32, the scan in chunks of plan["t_chunk"] frames with a carried count, the
    gather), or with one of FAULTS planted.  Returns what blank_skip_ref returns, blank_logp in float32."""
    assert fault is None or fault in FAULTS
    logits = np.asarray(logits, np.float32)
    T, B, C = logits.shape
    tpr = 64 if plan["kernel"] == "wave" else plan["rows_threads"]
    lpb = blank_logp_f32(logits, lengths, plan["words_per_lane"], tpr, plan["vec"])
    thr = np.float32(np.log(np.float64(theta)))
    n = clip_lengths(lengths, T)
    with np.errstate(invalid="ignore"):
        flags = (lpb > thr) if fault == "gt_not_ge" else (lpb >= thr)
    flags = flags & (np.arange(T)[:, None] < n[None, :])                 # (a row past its length writes flag 0)
    chunk = plan["t_chunk"]
    src = np.full((B, T), -1, np.int32)
    n_out = np.zeros(B, np.int32)
    keep = np.zeros((T, B), bool)
    for b in range(B):
        nb = T if fault == "count_past_length" else int(n[b])
        f = flags[:, b]
        base = 0
        for t0 in range(0, nb, chunk):
            for t in range(t0, min(t0 + chunk, nb)):
                if fault == "keep_last":
                    k = not (f[t] and t + 1 < nb and f[t + 1])
                else:
                    prev = t > 0 and f[t - 1] and not (fault == "seam_reset" and t == t0)
                    k = not (f[t] and prev)
                if k:
                    keep[t, b] = True
                    src[b, base] = t
                    base += 1
        n_out[b] = base
    out = np.full_like(logits, 7.0) if fault == "tail_not_zeroed" else np.zeros_like(logits)
    for b in range(B):
        out[:n_out[b], b] = logits[src[b, :n_out[b]], b]
    return dict(blank_logp=lpb, skip=flags, keep=keep, out_logits=out, out_lengths=n_out, src_frame=src)


def same_outputs(got, want):
    """out_lengths, src_frame and out_logits bit for bit (tail words included)."""
    return (np.array_equal(got["out_lengths"], want["out_lengths"]) and np.array_equal(got["src_frame"], want["src_frame"])
            and np.asarray(got["out_logits"], np.float32).tobytes() == np.asarray(want["out_logits"], np.float32).tobytes())


# ----------------------------------------------------------------------------------------------------------- case table
C_FIXED = (2, 5, 80, 81)
T_FIXED = (1, 2, 3)
B_ALL = (1, 3, 33)
C_MAX = 4096
PATTERNS = ("none", "all", "alternating", "run_at_start", "run_at_end", "seam", "past_length", "nan", "theta_one", "mixed")


def class_counts(plan):
    """The fixed C of the table plus the C on either side of every c_min / c_max boundary the plan reports up to 4096."""
    cs = set(C_FIXED)
    c = 2
    while c <= C_MAX:
        p = plan(3, 3, c)
        assert p["c_min"] <= c <= p["c_max"], (c, p)
        for v in (p["c_min"], p["c_max"], p["c_max"] + 1):
            if 2 <= v <= C_MAX:
                cs.add(v)
        c = p["c_max"] + 1
    return sorted(cs)


def frame_counts(plan):
    ch = plan(3, 3, 5)["t_chunk"]
    return sorted(set(T_FIXED) | {ch - 1, ch, ch + 1, 2 * ch + 1})


def lengths_for(T, B):
    """0, 1, T, T + 5 and a negative one, cycled over the rows; row 0 is always the full length."""
    menu = (T, T + 5, 1, 0, -3, max(T - 1, 0), (T + 1) // 2)
    return np.array([menu[b % len(menu)] for b in range(B)], np.int32)


def make_frames(blank, C, seed, dominance=20.0, noise=0.5):
    """Logits [T,B,C] from a wish bool [T,B]: True makes the blank logit `dominance` above seeded noise (lpb about -C exp(-dominance):
    skippable at every theta of the table), False gives a seeded non-blank label that lead (lpb about -dominance: never skippable)."""
    rng = np.random.RandomState(seed)
    T, B = blank.shape
    x = (noise * rng.randn(T, B, C)).astype(np.float32)
    if dominance >= EXACT_DOMINANCE:
        x = np.clip(x, -1.0, 1.0)
    label = rng.randint(0, C - 1, size=(T, B))
    tt, bb = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    x[tt, bb, np.where(blank, C - 1, label)] = np.float32(dominance)
    return x


def make_case(T, B, C, pattern, chunk, seed=0):
    """One case of the table: dict(name, T, B, C, theta, logits, lengths, pattern)."""
    rng = np.random.RandomState(7919 * seed + 31 * T + 7 * B + C)
    lengths = lengths_for(T, B)
    theta, dominance = 0.9, 20.0
    t = np.arange(T)[:, None] * np.ones((1, B), np.int64)
    if pattern == "none":
        blank = np.zeros((T, B), bool)
    elif pattern == "all":
        blank = np.ones((T, B), bool)
    elif pattern == "alternating":
        blank = t % 2 == 1
    elif pattern == "run_at_start":
        blank = t < max(2, T // 3)
    elif pattern == "run_at_end":                                         # ... of the FULL rows: up to n - 1 = T - 1
        blank = t >= T - max(2, T // 3)
    elif pattern == "seam":                                               # a run of two across every chunk seam, one frame on each side
        blank = (t % chunk == 0) & (t > 0) | (t % chunk == chunk - 1) & (t + 1 < T)
    elif pattern == "past_length":                                        # blank from two frames before the row's end to the buffer's
        n = clip_lengths(lengths, T)
        blank = t >= np.maximum(n - 2, 0)[None, :]
    elif pattern in ("nan", "mixed", "theta_one"):
        blank = rng.rand(T, B) < 0.6
        if pattern == "theta_one":
            theta, dominance = 1.0, 90.0
    else:
        raise ValueError(pattern)
    logits = make_frames(blank, C, seed + 1000 * T + C, dominance)
    if pattern == "theta_one":                                            # the non-blank frames keep a lead of 20 (lpb about -20)
        lead = make_frames(np.zeros((T, B), bool), C, seed + 5, 20.0)
        logits = np.where(blank[:, :, None], logits, lead)
    if pattern == "nan":                                                  # a NaN in a blank-looking frame INSIDE a run: it is kept
        for b in range(B):
            tn = min(T - 1, 1 + b % 3)
            logits[max(tn - 1, 0):tn + 2, b] = make_frames(np.ones((len(logits[max(tn - 1, 0):tn + 2]), 1), bool), C, seed + b)[:, 0]
            logits[tn, b, (3 * b) % C] = np.nan
    return dict(name="T%d_B%d_C%d_%s" % (T, B, C, pattern), T=T, B=B, C=C, theta=theta, logits=logits, lengths=lengths, pattern=pattern)


def cases(plan):
    """The table (module docstring of tests/test_gpu_blank_skip.py): every C at a small T, every T at a scalar and a vector C,
    every B, and every pattern at a T of two chunks and one frame (and at a small one)."""
    ch = plan(3, 3, 5)["t_chunk"]
    out, seen = [], set()

    def add(T, B, C, pattern):
        key = (T, B, C, pattern)
        if key not in seen:
            seen.add(key)
            out.append(make_case(T, B, C, pattern, ch))

    for C in class_counts(plan):
        add(7, 3, C, "mixed")
    for T in frame_counts(plan):
        for C in (5, 80):
            add(T, 3, C, "mixed")
    for B in B_ALL:
        add(9, B, 80, "mixed")
        add(ch + 1, B, 5, "seam")
    for pattern in PATTERNS:
        add(2 * ch + 1, 3, 5, pattern)
        add(9, 3, 80, pattern)
    add(5, 3, C_MAX, "theta_one")
    add(5, 3, 1025, "nan")
    return out


# --------------------------------------------------------------------------------- peaky posteriors for the decoders
MEAN_RUN = 4.0


def peaky_posteriors(T, B, C, blank_share, seed, soft=True):
    """Seeded CTC-like posteriors [T,B,C] and lengths: isolated label frames between runs of blank frames whose blank logit is
    EXACT_DOMINANCE above all others (lpb exactly 0.0 in float32: skippable at every theta), about blank_share of the frames inside
    such runs.  A label frame leads by about 6 with a runner-up (soft: the decoders' n-best lists then hold real alternatives, far
    above the e^-80 a path through a run frame costs)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(T, B, C).astype(np.float32)
    in_run = np.zeros((T, B), bool)
    start = blank_share / (MEAN_RUN - (MEAN_RUN - 1.0) * blank_share)     # runs of 1 + Poisson(MEAN_RUN - 1) frames cover blank_share
    for b in range(B):
        t = 0
        while t < T:
            if rng.rand() < start:
                run = 1 + rng.poisson(MEAN_RUN - 1.0)
                in_run[t:t + run, b] = True
                t += run
            else:
                t += 1
    lab = rng.randint(0, C - 1, size=(T, B))
    tt, bb = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    x[tt, bb, lab] += np.float32(6.0)
    if soft:
        x[tt, bb, (lab + 1 + rng.randint(0, max(C - 2, 1), size=(T, B))) % (C - 1)] += np.float32(3.0)
    run = np.clip(rng.randn(T, B, C), -1.0, 1.0).astype(np.float32)
    run[:, :, C - 1] = np.float32(EXACT_DOMINANCE + 1.0)
    x = np.where(in_run[:, :, None], run, x)
    lengths = np.array([T - (3 * b) % max(T // 2, 1) for b in range(B)], np.int32)
    return x, lengths, in_run
