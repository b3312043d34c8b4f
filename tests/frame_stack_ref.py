"""CHECKER ONLY (never imported by the product): the numpy reference, the case table and the inputs of the low frame rate input
kernel (csrc/frame_stack.hip, ops.frame_stack).

    out[j][b][i * D + d] = x[j * s + i][b][d]   if j * s + i < min(n_b, t_in),   0 otherwise        n_out[b] = ceil(n_b / s)

The kernel is a copy, so everything here works on uint32 bit patterns and the comparison is np.array_equal: no tolerance.

The table is the smallest set of shapes at which the kernel can go wrong.  Every value of every axis appears -- (k, s) in
{(1,1), (3,3), (2,3), (3,1), (8,3), (1,4), (16,16)}, D in {1, 6, 13, 20, 40, 120}, t_in in {1, 2, 7, 9, 10} (windows that run past
the end, t_in below k), B in {1, 3, 33, 257} -- each (k, s) meets both `vec` values, and B = 257 brings `meta_by_copy`.  One case
beyond those sets ("grid_stride") has more items than the capped grid takes in one pass.  Every case names the plan fields it was
written for; `expected_plan` restates the arithmetic of plan_frame_stack independently, and the GPU test asserts the fields
against ops.frame_stack_plan so that a case cannot silently run the other variant.

Lengths within one batch cycle through 0, 1, t_in - 1, t_in, t_in + 5 (the front end's counts are not clipped to t_in), starting at
the case's `first`.  The source is poisoned with a NaN at every frame at or past its row's length, and the valid region carries
-0.0, a denormal, +inf, -inf and a NaN with a payload."""
import numpy as np

THREADS, MAX_WGS, META_MAX, MAX_FACTOR, MAX_WIDTH = 256, 2048, 256, 16, 4096
POISON = np.uint32(0x7FC0DEAD)          # a quiet NaN no valid element holds
SENTINEL = np.uint32(0xCDCDCDCD)        # what `out` holds before the call
SPECIALS = np.array([0x80000000,        # -0.0
                     0x00000001,        # the smallest denormal
                     0x7F800000,        # +inf
                     0xFF800000,        # -inf
                     0x7FA12345],       # a signalling NaN with a payload
                    np.uint32)

# name: (k, s, D, t_in, B, first, plan fields the case was written for)
CASES = {
    "k1s1_vec4":        (1, 1, 40, 7, 3, 2, dict(vec=4, meta_by_copy=0)),
    "k1s1_vec1":        (1, 1, 13, 10, 1, 4, dict(vec=1, meta_by_copy=0)),
    "k3s3_vec4":        (3, 3, 40, 10, 33, 0, dict(vec=4, meta_by_copy=0, t_out=4, d_out=120)),
    "k3s3_vec1":        (3, 3, 13, 7, 3, 2, dict(vec=1, meta_by_copy=0, t_out=3)),
    "k3s3_by_copy":     (3, 3, 40, 9, 257, 0, dict(vec=4, meta_by_copy=1, t_out=3)),
    "k2s3_vec4":        (2, 3, 20, 9, 3, 1, dict(vec=4, meta_by_copy=0)),
    "k2s3_vec1":        (2, 3, 6, 2, 1, 3, dict(vec=1, meta_by_copy=0, t_out=1)),
    "k3s1_vec4":        (3, 1, 120, 7, 3, 2, dict(vec=4, meta_by_copy=0, t_out=7, d_out=360)),
    "k3s1_vec1":        (3, 1, 1, 10, 33, 0, dict(vec=1, meta_by_copy=0, d_out=3)),
    "k8s3_short":       (8, 3, 20, 2, 3, 2, dict(vec=4, meta_by_copy=0, t_out=1)),           # t_in below k
    "k8s3_vec1":        (8, 3, 13, 9, 33, 0, dict(vec=1, meta_by_copy=0)),
    "k1s4_one_frame":   (1, 4, 40, 1, 1, 4, dict(vec=4, meta_by_copy=0, t_out=1)),
    "k1s4_vec1":        (1, 4, 6, 10, 3, 2, dict(vec=1, meta_by_copy=0, t_out=3)),
    "k16s16_vec4":      (16, 16, 120, 10, 3, 2, dict(vec=4, meta_by_copy=0, t_out=1, d_out=1920)),   # 480 words on 256 lanes
    "k16s16_vec1":      (16, 16, 1, 7, 33, 0, dict(vec=1, meta_by_copy=0, t_out=1)),
    "k16s16_one_frame": (16, 16, 6, 1, 1, 3, dict(vec=1, meta_by_copy=0)),
    "grid_stride":      (3, 1, 120, 125, 33, 0, dict(vec=4, meta_by_copy=0, workgroups=MAX_WGS)),   # 2063 passes' worth of items
}


def ceil_div(a, b):
    return -(-int(a) // int(b))


def lanes_per_item(units):
    lanes = 1
    while lanes < units and lanes < THREADS:
        lanes *= 2
    return lanes


def expected_plan(B, D, t_in, k, s):
    """The whole plan struct as a dict, or None where the call is refused."""
    if B <= 0 or D <= 0 or t_in <= 0 or not 1 <= k <= MAX_FACTOR or not 1 <= s <= MAX_FACTOR or k * D > MAX_WIDTH:
        return None
    vec = 4 if D % 4 == 0 else 1
    t_out = ceil_div(t_in, s)
    per_wg = THREADS // lanes_per_item(k * D // vec)
    return dict(t_out=t_out, d_out=k * D, vec=vec, workgroups=min(ceil_div(t_out * B, per_wg), MAX_WGS),
                meta_by_copy=1 if B > META_MAX else 0)


def stack(x, n_frames, k, s):
    """The formula above on an array [t_in, B, D] of any dtype: (out [ceil(t_in / s), B, k * D], n_out)."""
    x = np.asarray(x)
    t_in, B, D = x.shape
    t_out = ceil_div(t_in, s)
    out = np.zeros((t_out, B, k * D), x.dtype)
    for b in range(B):
        n = min(int(n_frames[b]), t_in)
        for i in range(k):
            j = np.arange(t_out)
            j = j[j * s + i < n]
            out[j, b, i * D:(i + 1) * D] = x[j * s + i, b]
    return out, np.array([ceil_div(n, s) for n in n_frames], np.int32)


def stack_brute_force(x, n_frames, k, s):
    """... and as the formula is written: three loops, one source frame at a time."""
    x = np.asarray(x)
    t_in, B, D = x.shape
    t_out = ceil_div(t_in, s)
    out = np.zeros((t_out, B, k * D), x.dtype)
    for j in range(t_out):
        for b in range(B):
            for i in range(k):
                if j * s + i < min(int(n_frames[b]), t_in):
                    out[j, b, i * D:(i + 1) * D] = x[j * s + i, b, :]
    return out


def case_lengths(t_in, B, first):
    values = [0, 1, t_in - 1, t_in, t_in + 5]
    return np.array([values[(first + b) % 5] for b in range(B)], np.int32)


def case_inputs(name):
    """(x uint32 [t_in, B, D], lengths int32 [B]) of a case: random finite floats, the special patterns from the start of every
    row's valid region, POISON at every frame at or past the row's length."""
    k, s, D, t_in, B, first, _ = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    x = rng.randn(t_in, B, D).astype(np.float32).view(np.uint32).copy()
    lengths = case_lengths(t_in, B, first)
    for b in range(B):
        n = min(int(lengths[b]), t_in)
        flat = x[:n, b].reshape(-1)                 # (a copy: the row's frames are not contiguous)
        m = min(len(SPECIALS), flat.size)
        flat[:m] = SPECIALS[:m]
        if flat.size > len(SPECIALS):
            flat[-1] = SPECIALS[-1]                 # ... and a payload in the last valid word
        x[:n, b] = flat.reshape(n, D)
        x[n:, b] = POISON
    return x, lengths
