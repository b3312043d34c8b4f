"""CHECKER ONLY (never imported by the product): SpecAugment's frequency and time masks restated in numpy from the semantics the
C ABI documents (include/amdspeech.h, "SpecAugment"), not from the kernel (csrc/spec_augment.hip, ops.spec_augment).

    r(stream, idx) = mix32(mix32(idx ^ lo32(seed)) + stream * 0x9e3779b9 + hi32(seed)) >> 8             24 bits
    mask m of a kind of row b:   idx = b * 64 + m,   stream = 0x5A000000 + 2 * kind + which     (kind 0 frequency, 1 time;
                                                                                                 which 0 width, 1 start)
    wmax   = kind == 0 ? min(Fw, P) : min(Tw, n_b * permille // 1000)         extent = kind == 0 ? P : n_b
    width  = (r(width stream, idx) * (wmax + 1)) >> 24
    start  = (r(start stream, idx) * (extent - width + 1)) >> 24
    x[t, b, c] = +0.0 for t < n_b = min(len_b, T) when c % P lies in a frequency span of row b or t in a time span of row b

Integers only, so the comparison with the kernel is np.array_equal on uint32 bit patterns: masked words are 0x00000000, every other
word -- the frames at or past n_b included -- keeps its pattern.

CASES: the smallest shapes at which the kernel can go wrong; each names what it can catch.  `expected_plan` restates the plan's
arithmetic independently, and the tests assert the fields against ops.spec_augment_plan so that no case silently runs the other
variant.  "stride" has more (frame, row) items than one pass of the capped grid."""
import numpy as np

THREADS, MAX_WGS, STORES_PER_LANE, MAX_WIDTH, MAX_FREQ_MASKS, MAX_TIME_MASKS = 256, 2048, 4, 4096, 8, 16
SEED = (7 << 32) | 12345
POISON = np.uint32(0x7FC0DEAD)          # a quiet NaN no live element holds: every frame at or past a row's length
SPECIALS = np.array([0x80000000,        # -0.0
                     0x00000001,        # the smallest denormal
                     0x7F800000,        # +inf
                     0xFF800000,        # -inf
                     0x7FA12345],       # a signalling NaN with a payload
                    np.uint32)
M32 = 0xFFFFFFFF


def policy(P, F, Fw, M, Tw, permille):
    return dict(period=P, freq_masks=F, freq_width=Fw, time_masks=M, time_width=Tw, time_permille=permille)


def _stride_lengths(B):
    return [270 + b % 40 for b in range(B)]          # 270 .. 309


# name: (T, B, W, P, F, Fw, M, Tw, permille, lengths)
CASES = {
    "scalar_w13":    (9, 3, 13, 13, 2, 5, 2, 4, 1000, [9, 4, 0]),            # the scalar variant; an empty row
    "vec4_p40":      (12, 4, 40, 40, 2, 7, 2, 5, 1000, [12, 20, 1, 7]),      # 16-byte time rows, frequency spans across vector
                                                                             # boundaries; a length above T; a one-frame row
    "stacked_p13x4": (10, 3, 52, 13, 2, 6, 1, 3, 500, [10, 6, 3]),           # W % 4 == 0 while P % 4 != 0; four repetitions
    "fbank_p40x3":   (8, 2, 120, 40, 2, 8, 2, 3, 1000, [8, 5]),              # static / delta / delta-delta masked together
    "stack3_fbank":  (7, 2, 360, 40, 1, 8, 1, 2, 400, [7, 3]),               # nine repetitions
    "cap_zero":      (6, 3, 16, 16, 1, 4, 2, 10, 100, [6, 9, 2]),            # the ratio cap rounds every time mask to width 0
    "full_width":    (5, 2, 8, 8, 3, 8, 0, 0, 0, [5, 5]),                    # Fw == P; M == 0
    "stride":        (310, 1700, 16, 16, 2, 4, 2, 20, 200, _stride_lengths(1700)),    # 527,000 items on 2048 x 256 per pass
}


def case_policy(name):
    return policy(*CASES[name][3:9])


def mix32(v):
    v &= M32
    v ^= v >> 16
    v = (v * 0x7feb352d) & M32
    v ^= v >> 15
    v = (v * 0x846ca68b) & M32
    v ^= v >> 16
    return v


def r(seed, stream, idx):
    """The 24-bit draw; python ints, 32-bit wrap-around."""
    a = mix32((idx & M32) ^ (seed & M32))
    return mix32((a + stream * 0x9e3779b9 + ((seed >> 32) & M32)) & M32) >> 8


def spans(pol, seed, b, n):
    """[(start, width)] of row b with n = min(len_b, T) frames: the F frequency masks first, then the M time masks."""
    out = []
    for kind, count in ((0, pol["freq_masks"]), (1, pol["time_masks"])):
        for m in range(count):
            idx = b * 64 + m
            if kind == 0:
                wmax, extent = min(pol["freq_width"], pol["period"]), pol["period"]
            else:
                wmax, extent = min(pol["time_width"], n * pol["time_permille"] // 1000), n
            width = (r(seed, 0x5A000000 + 2 * kind, idx) * (wmax + 1)) >> 24
            start = (r(seed, 0x5A000000 + 2 * kind + 1, idx) * (extent - width + 1)) >> 24
            out.append((start, width))
    return out


def masks(pol, seed, T, W, b, length):
    """(n_b, time mask bool [T], channel mask bool [W]) of one row."""
    n = min(int(length), T)
    t_mask, c_mask = np.zeros(T, bool), np.zeros(W, bool)
    if n <= 0:
        return n, t_mask, c_mask
    sp = spans(pol, seed, b, n)
    bins = np.arange(W) % pol["period"]
    for start, width in sp[:pol["freq_masks"]]:
        c_mask |= (bins >= start) & (bins < start + width)
    for start, width in sp[pol["freq_masks"]:]:
        t_mask[start:start + width] = True
    t_mask[n:] = False
    return n, t_mask, c_mask


def apply(x, lengths, pol, seed):
    """A masked COPY of x [T, B, W] (any dtype: uint32 bit patterns for the exact comparison, float64 for the oracle)."""
    x = np.array(x, copy=True)
    T, B, W = x.shape
    for b in range(B):
        n, t_mask, c_mask = masks(pol, seed, T, W, b, lengths[b])
        if n <= 0:
            continue
        live = np.zeros(T, bool)
        live[:n] = True
        x[:, b][(live[:, None] & (t_mask[:, None] | c_mask[None, :]))] = 0
    return x


def lanes_per_item(units):
    lanes = 1
    while lanes * STORES_PER_LANE < units and lanes < THREADS:
        lanes *= 2
    return lanes


def expected_plan(T, B, W, pol):
    """The whole plan struct as a dict (for a 16-byte aligned x), or None where the call is refused."""
    P, F, Fw, M, Tw, pm = (pol[k] for k in ("period", "freq_masks", "freq_width", "time_masks", "time_width", "time_permille"))
    if T <= 0 or B <= 0 or T * B >= 2 ** 31 or not 1 <= W <= MAX_WIDTH or not 1 <= P <= W or W % P:
        return None
    if not 0 <= F <= MAX_FREQ_MASKS or not 0 <= M <= MAX_TIME_MASKS or not 0 <= Fw <= P or Tw < 0 or not 0 <= pm <= 1000:
        return None
    vec = 4 if W % 4 == 0 else 1
    lanes = lanes_per_item(W // vec)
    per_wg = THREADS // lanes
    on = (F > 0 and Fw > 0) or (M > 0 and Tw > 0 and pm > 0)        # a kind with no mask or no width masks nothing
    return dict(vec=vec, lanes=lanes, items_per_workgroup=per_wg, workgroups=min(-(-T * B // per_wg), MAX_WGS) if on else 0,
                reps=W // P)


def case_inputs(name):
    """(x uint32 [T, B, W], lengths int32 [B]): random finite floats (none of them zero), the special patterns from the start of
    every row's live region and a payload in its last live word, POISON at every frame at or past the row's length."""
    T, B, W = CASES[name][:3]
    lengths = np.asarray(CASES[name][9], np.int32)
    rng = np.random.RandomState(sum(map(ord, name)))
    x = (rng.rand(T, B, W) + 0.5).astype(np.float32).view(np.uint32).copy()
    for b in range(B):
        n = min(int(lengths[b]), T)
        if n > 0:
            flat = x[:n, b].reshape(-1)             # (a copy: the row's frames are not contiguous)
            m = min(len(SPECIALS), flat.size)
            flat[:m] = SPECIALS[:m]
            if flat.size > len(SPECIALS):
                flat[-1] = SPECIALS[-1]
            x[:n, b] = flat.reshape(n, W)
        x[n:, b] = POISON
    return x, lengths
