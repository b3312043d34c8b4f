"""CHECKER ONLY (never imported by the product): the float64 reference, the bound, the case table and the inputs of the feature
normalisation kernels (csrc/feature_norm.hip, ops.feature_norm / ops.feature_moments), restated in numpy from the semantics the
C ABI documents (include/amdspeech.h, "feature normalisation"), not from the kernels.

    n = min(n_b, t_in);  mean = (1/n) sum_{t<n} x[t,b,d];  var = (1/n) sum_{t<n} (x[t,b,d] - mean)^2      (population variance)
    y[t,b,d] = (x[t,b,d] - mean) * scale  for t < n,   scale = 1 / sqrt(max(var, 1e-10))  (1 without variance normalisation)

The reference is TWO-PASS in float64: the mean first, then the squared deviations from it.

The bound (derived, not measured).  The library accumulates in float64 and rounds the result to float32 once, so
    |y - y_ref| <= 1 ulp_f32(|y_ref|) + 2^-40 * max_t |x[t,b,d]| * scale
the first term for the one rounding (half an ulp, a whole one where y and y_ref straddle a power of two), the second for what the
float64 sums can lose: a relative 2^-40 of the largest input is thousands of times the 2^-53 of one float64 operation, room for the
n <= 2^20 additions of a row and for the cancellation in Q'/n - (S'/n)^2 as long as the shift K is within a few deviations of the mean.

The case table is the smallest set of shapes at which the kernels can go wrong; every case names the plan fields it was written
for, `expected_plan` restates the plan's arithmetic independently, and the tests assert the fields against ops.feature_norm_plan so
that no case silently runs another variant.  Inputs: every frame at or past its row's length holds a NaN (POISON) that must still
be there afterwards; dim 0 has mean -1131 and deviation 3 (c0 of an MFCC on speech), dim 1 is constant within a row, dim 2 moves by
one float32 ulp around 5 (a variance of 5.7e-14, below the floor), the others draw their offsets from +-1200 and their scales from
1e-3 .. 1e2.

A MISALIGNED BASE (x off by one word with D % 4 == 0) is REFUSED by the library (amdspeech.h), not run with single-word accesses;
tests/test_gpu_feature_norm.py::test_misaligned_base_is_refused holds it to that."""
import numpy as np

THREADS, MAX_WGS, TARGET_WGS, MIN_PASSES, META_MAX, MAX_WIDTH = 256, 2048, 512, 4, 256, 4096
VAR_FLOOR = 1e-10
MODES = ("none", "utterance", "global")
POISON = np.uint32(0x7FC0DEAD)          # a quiet NaN no valid element holds
PAD_FINITE = np.float32(12345.0).view(np.uint32)

# name: (D, t_in, B, lengths, plan fields the case was written for).  lengths: "edges" = 0, 1, 2, t_in, t_in + 7 cycling over the
# rows; "full" = t_in, t_in + 7, 0.7 t_in cycling; or an explicit list
CASES = {
    "vec4_d40":      (40, 70, 5, "edges", dict(vec=4, split=1, meta_by_copy=0)),
    "vec4_d120":     (120, 70, 5, "edges", dict(vec=4, split=2, meta_by_copy=0)),            # fbank's width; two slices of 35
    "vec1_d13":      (13, 70, 5, "edges", dict(vec=1, split=1, meta_by_copy=0)),
    "mid_slice":     (120, 70, 3, [36, 35, 69], dict(vec=4, split=2)),                       # lengths one frame into / at the end of slice 0
    "offset_split":  (40, 1001, 3, "full", dict(vec=4, split=15, workgroups=45)),            # |mean| >> std over 1001 frames, 15 slices
    "constant_dim":  (8, 33, 2, "full", dict(vec=4, split=1)),
    "tiny_variance": (8, 33, 2, [33, 17], dict(vec=4, split=1)),
    "wide_batch":    (4, 3, 257, "edges", dict(vec=4, split=1, meta_by_copy=1, workgroups=257)),
    "widest_frame":  (4096, 2, 1, [2], dict(vec=4, split=1, workgroups=1)),                    # 1024 vector columns on 256 lanes
    "vec1_columns":  (301, 5, 2, [5, 3], dict(vec=1, split=1)),                                # 301 columns on 256 lanes, one slot
    "row_stride":    (4, 2, 2050, "edges", dict(vec=4, split=1, meta_by_copy=1, workgroups=MAX_WGS)),   # rows beyond the grid's cap
    "headline_rows": (40, 1001, 32, "full", dict(vec=4, split=15, workgroups=480)),          # the headline shape itself
}
GPU_CASES = sorted(CASES)


def ceil_div(a, b):
    return -(-int(a) // int(b))


def lanes_for(cols):
    lanes = 1
    while lanes < cols and lanes < THREADS:
        lanes *= 2
    return lanes


def slots_for(D):
    vec = 4 if D % 4 == 0 else 1
    return THREADS // lanes_for(D // vec)


def expected_plan(B, D, t_in, mode="utterance"):
    """The whole plan struct as a dict, or None where the call is refused."""
    if B <= 0 or D <= 0 or t_in <= 0 or t_in * B >= 2 ** 31 or D > MAX_WIDTH or mode not in MODES:
        return None
    vec = 4 if D % 4 == 0 else 1
    rows = min(B, MAX_WGS)
    split = max(1, min(ceil_div(TARGET_WGS, rows), t_in // (MIN_PASSES * slots_for(D))))
    split = ceil_div(t_in, ceil_div(t_in, split))
    ws = B * (2 * split + 1) * D * 8 if mode == "utterance" else 0
    if ws >= 2 ** 31:
        return None
    return dict(vec=vec, split=split, workgroups=0 if mode == "none" else split * rows, lds_bytes=THREADS * 2 * vec * 8,
                meta_by_copy=1 if B > META_MAX else 0, workspace_bytes=ws)


# ------------------------------------------------------------------------------------------------ the float64 reference
def clipped(n_frames, t_in):
    return np.minimum(np.asarray(n_frames, np.int64), t_in)


def statistics(x, n_frames):
    """(mean, var) float64 [B, D] of each row's first min(n, t_in) frames, two-pass; zeros for an empty row."""
    x = np.asarray(x, np.float64)
    t_in, B, D = x.shape
    mean, var = np.zeros((B, D)), np.zeros((B, D))
    for b, n in enumerate(clipped(n_frames, t_in)):
        if n > 0:
            mean[b] = x[:n, b].sum(axis=0) / n
            var[b] = ((x[:n, b] - mean[b]) ** 2).sum(axis=0) / n
    return mean, var


def moments(x, n_frames):
    """float64 [B, 2, D]: mean and M2 = sum (x - mean)^2 per row (what ops.feature_moments returns)."""
    mean, var = statistics(x, n_frames)
    n = clipped(n_frames, np.asarray(x).shape[0]).astype(np.float64)
    return np.stack([mean, var * n[:, None]], axis=1)


def scales(var, norm_vars=True, var_floor=VAR_FLOOR):
    return 1.0 / np.sqrt(np.maximum(var, var_floor)) if norm_vars else np.ones_like(var)


def normalise(x, n_frames, norm_vars=True, var_floor=VAR_FLOOR):
    """float64 [t_in, B, D]: the formula above; frames at or past a row's length keep what x holds there."""
    x = np.asarray(x, np.float64)
    y = x.copy()
    mean, var = statistics(x, n_frames)
    scale = scales(var, norm_vars, var_floor)
    for b, n in enumerate(clipped(n_frames, x.shape[0])):
        y[:n, b] = (x[:n, b] - mean[b]) * scale[b]
    return y


def normalise_global(x, n_frames, table):
    """float32, bit for bit what global mode stores: float32((float64(x) - mean) * scale) on the valid frames."""
    x = np.asarray(x, np.float32)
    y = x.copy()
    for b, n in enumerate(clipped(n_frames, x.shape[0])):
        y[:n, b] = ((x[:n, b].astype(np.float64) - table[0]) * table[1]).astype(np.float32)
    return y


def bound(x, n_frames, norm_vars=True, var_floor=VAR_FLOOR):
    """float64 [t_in, B, D]: the bound of the module docstring at every element (meaningless past a row's length)."""
    x64 = np.asarray(x, np.float64)
    y = normalise(x64, n_frames, norm_vars, var_floor)
    _, var = statistics(x64, n_frames)
    scale = scales(var, norm_vars, var_floor)
    out = np.zeros_like(y)
    for b, n in enumerate(clipped(n_frames, x64.shape[0])):
        if n > 0:
            ulp = np.spacing(np.abs(y[:n, b]).astype(np.float32)).astype(np.float64)
            out[:n, b] = ulp + 2.0 ** -40 * np.abs(x64[:n, b]).max(axis=0) * scale[b]
    return out


def judge(got, x, n_frames, const_dims=(), norm_vars=True, var_floor=VAR_FLOOR):
    """What the edge test asserts about a result `got` (float32 [t_in, B, D]) for the input x: dict(ratio = the worst
    |got - y_ref| / bound over the valid frames (inf for a NaN), pad_intact = every word at or past a row's length unchanged bit
    for bit, const_zero = the constant dims exactly 0.0)."""
    x = np.asarray(x, np.float32)
    got = np.asarray(got, np.float32)
    y, lim = normalise(x, n_frames, norm_vars, var_floor), bound(x, n_frames, norm_vars, var_floor)
    ratio, pad_intact, const_zero = 0.0, True, True
    for b, n in enumerate(clipped(n_frames, x.shape[0])):
        pad_intact &= np.array_equal(got[n:, b].view(np.uint32), x[n:, b].view(np.uint32))
        if n > 0:
            err = np.abs(got[:n, b].astype(np.float64) - y[:n, b]) / lim[:n, b]
            ratio = max(ratio, float(np.where(np.isnan(err), np.inf, err).max()))
            for d in const_dims:
                const_zero &= bool(np.all(got[:n, b, d].view(np.uint32) << 1 == 0))      # (+0.0 or -0.0)
    return dict(ratio=ratio, pad_intact=bool(pad_intact), const_zero=bool(const_zero))


def passes(verdict):
    return verdict["ratio"] <= 1.0 and verdict["pad_intact"] and verdict["const_zero"]


# ------------------------------------------------------------------------------------------------ inputs
def case_lengths(name):
    D, t_in, B, kind, _ = CASES[name]
    if kind == "edges":
        values = [0, 1, 2, t_in, t_in + 7]
    elif kind == "full":
        values = [t_in, t_in + 7, max(1, int(0.7 * t_in))]
    else:
        values = list(kind)
    return np.array([values[b % len(values)] for b in range(B)], np.int32)


def const_dims(name):
    """Dims of a case that are constant within every row: they must come out as exact zeros."""
    D = CASES[name][0]
    if name == "constant_dim":
        return (1, 3, 6)
    return (1,) if D >= 4 else ()


def case_inputs(name, pad=POISON):
    """(x float32 [t_in, B, D], lengths int32 [B]); every word of a frame at or past its row's length holds the bit pattern `pad`:
    POISON, or PAD_FINITE where a check must see a padded word that was recomputed (arithmetic on a NaN can return its very bits)."""
    D, t_in, B, _, _ = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    offsets = rng.uniform(-1200, 1200, size=D)
    spreads = 10.0 ** rng.uniform(-3, 2, size=D)
    x = (offsets + spreads * rng.randn(t_in, B, D)).astype(np.float32)
    if D >= 4:
        x[:, :, 0] = (-1131.0 + 3.0 * rng.randn(t_in, B)).astype(np.float32)
        x[:, :, 2] = np.float32(5.0) + np.spacing(np.float32(5.0)) * rng.randint(0, 2, size=(t_in, B)).astype(np.float32)
    for d in const_dims(name):
        x[:, :, d] = (-1131.0 + 0.37 * d + np.arange(B)).astype(np.float32)[None, :]
    if name == "tiny_variance":             # every dim but the constant one: a few ulps around its offset
        for d in range(D):
            if d not in const_dims(name) and d != 2:
                base = np.float32(offsets[d] if d else -1131.0)
                x[:, :, d] = base + np.spacing(np.abs(base)) * rng.randint(-2, 3, size=(t_in, B)).astype(np.float32)
    lengths = case_lengths(name)
    bits = x.view(np.uint32)
    for b, n in enumerate(clipped(lengths, t_in)):
        bits[n:, b] = pad
    return x, lengths


# ------------------------------------------------------------------------------------------------ the kernels' scheme, emulated
FAULTS = {                                   # a planted fault -> the case whose check it must miss
    "float32_no_shift": "offset_split",      # float32 accumulation of x and x^2 without the shift
    "shift_from_row_0": "vec4_d40",          # K taken from row 0 (there: an empty row, its frame 0 a NaN) instead of row b
    "sample_variance": "offset_split",       # divides by n - 1
    "unclipped_count": "vec4_d40",           # n_frames[b] used unclipped (a row of t_in + 7)
    "padding_summed": "vec4_d40",            # frames at or past n included in the sums
    "padding_written": "vec4_d40",           # frames at or past n written
    "last_slice_dropped": "offset_split",    # the last time slice's partial left out
    "delta_dims_skipped": "vec4_d120",       # only the 40 static dims of fbank normalised
    "scale_before_subtraction": "offset_split",      # x * scale - mean
}


def emulate(x, n_frames, split, slots, norm_vars=True, var_floor=VAR_FLOOR, fault=None):
    """The scheme amdspeech.h documents, in numpy: per time slice and frame slot a float64 chain of (x - K) and (x - K)^2 with
    K = x[0, b], the slots summed in slot order, the slices in slice order, mean = K + S'/n, var = max(Q'/n - (S'/n)^2, 0), scale
    in float64, one rounding.  fault: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS, fault
    x = np.asarray(x, np.float32)
    t_in, B, D = x.shape
    out = x.copy()
    slice_len = ceil_div(t_in, split)
    acc = np.float32 if fault == "float32_no_shift" else np.float64
    for b in range(B):
        n_raw = int(n_frames[b])
        n = n_raw if fault == "unclipped_count" else min(n_raw, t_in)
        last = t_in if fault == "padding_summed" else min(n, t_in)          # frames that enter the sums
        if n <= 0:
            continue
        K = x[0, 0 if fault == "shift_from_row_0" else b].astype(np.float64)
        if fault == "float32_no_shift":
            K = np.zeros(D)
        S, Q = np.zeros(D, acc), np.zeros(D, acc)
        for s in range(split - 1 if fault == "last_slice_dropped" else split):
            t0, t1 = s * slice_len, min((s + 1) * slice_len, last)
            Ss, Qs = np.zeros(D, acc), np.zeros(D, acc)
            for q in range(slots):
                d = (x[t0 + q:t1:slots, b].astype(np.float64) - K).astype(acc)
                if len(d):
                    Ss = Ss + np.cumsum(d, axis=0, dtype=acc)[-1]
                    Qs = Qs + np.cumsum(d * d, axis=0, dtype=acc)[-1]
            S, Q = S + Ss, Q + Qs
        with np.errstate(all="ignore"):
            m = (S / acc(n)).astype(acc)
            mean = K + m.astype(np.float64)
            var = np.maximum((Q / acc(n) - m * m).astype(np.float64), 0.0)
            if fault == "sample_variance":
                var = var * n / (n - 1)
            scale = 1.0 / np.sqrt(np.maximum(var, var_floor)) if norm_vars else np.ones(D)
            dims = slice(0, 40) if fault == "delta_dims_skipped" else slice(None)
            stop = t_in if fault == "padding_written" else min(n, t_in)
            v = x[:stop, b, dims].astype(np.float64)
            if fault == "scale_before_subtraction":
                out[:stop, b, dims] = (v * scale[dims] - mean[dims]).astype(np.float32)
            else:
                out[:stop, b, dims] = ((v - mean[dims]) * scale[dims]).astype(np.float32)
    return out
