"""The small kernels around the planned ones -- clip + Adam, batch norm (fused and data parallel), reverse_sequences, greedy decode,
merge_repeated, edit_distance, axpy and fill: the case tables, references and placement of tests/test_cpu_small_ref.py and
tests/test_gpu_small_kernels.py.  numpy only; a checker: the product never imports it.

Data kinds and what each owes:
  ints    (clip_adam, reverse_sequences with accumulate, the adjoint, axpy) small integers stored as f32: every sum stays below 2^24
          and is exact in f32 in ANY order, so the result is owed BIT FOR BIT.  clip_adam: gradients in {-1, 0, 1}, nonzero at
          index 0, n - 1, the scalar tail and both sides of every grid-stride boundary of either kernel (adam_geometry()), sparse
          enough that S = sum g^2 < 2^18: one dropped or doubled term moves sqrt(S) by >= 16 ulp, and the norm is asserted within
          1 ulp of float32(sqrt(S)).  With clip = 1e9 the scale is exactly 1; with m = v = 0, m = (1 - b1) g and v = (1 - b2) g^2 are
          single f32 products, owed bit for bit; a zero gradient leaves p as it was, bit for bit: every element updated exactly once.
  atclip  (clip_adam) 65536 gradients of +-2^-8, the rest 0: S = 1 exactly in any order, norm = 1.0 = clip.  The run with clip = 1
          must equal the run with clip = 1e9 bit for bit (m and v nonzero).
  zero    (clip_adam) all gradients 0: norm 0; with m = 0: p and m as they were, v = b2 v, bit for bit; with m != 0: m = b1 m and
          v = b2 v bit for bit, p against float64, nothing non-finite.
  normal  randn against float64 (the oracle's functions); tiny (clip_adam): |g| ~ 1e-12, sqrt(v) far below eps.
  planned (greedy decode) logits = 10 * one-hot of a planned best path + noise of 0.1: the expected ids follow from the plan alone
          (collapse()); exact ties are planted as equal floats and planned as the LOWEST index.
  Everything about integers (decode, merge, distance) and every copy (reverse_sequences, fill) is owed exactly.

Bounds of the float cases: no new constants.  adam_f32() and bn_f32() / bn_dp_f32() restate the kernels' formulas in f32 numpy -- batch
sums sequentially over b in the kernels' order, the sum of squares in the kernels' thread / wave / block order; the error of that
restatement against float64 ON THE CASE'S OWN INPUTS, times 4 (FMA contraction, the 1-2 ulp of rsqrtf / sqrtf that numpy does not
share), is the bound per case and output, computed when asked for and stored nowhere.  Errors are max|got - ref| / max|ref| (p of
clip_adam: max|got - ref|), and the clip_adam bounds never exceed those of tests/test_gpu_kernels.py::test_clip_adam (ADAM_CAPS).
One floor, from the number format and not from any kernel: no f32 result is owed closer to float64 than half an ulp, yet the
restatement's error on a SINGLE number (the norm; inv_std of the 1 x 1 x 1 shape) falls anywhere between 0 and half an ulp by chance
(measured: 2e-9 for the norm of normal-1023-unclipped), where a kernel that contracts one product into an FMA is a whole ulp away.
So a measured error enters as at least HALF_ULP = 2^-24 of the reference's largest magnitude: no bound is below 2 ulp of that.
bn_one_pass_f32() is the E[x^2] - mean^2 rewrite the offset data must catch.

Placement (Placed): every output and every input is a contiguous view inside a larger buffer, GUARD elements before and after,
the view's offset a multiple of 4 elements (16 bytes: clip_adam requires it) plus `off`.  Around outputs: 7.0 (int32: 0x7a7a7a7a),
owed bit-identical afterwards; around inputs: NaN (int32: the same sentinel).  ops.ctc_greedy_decode and ops.edit_distance allocate
their own outputs: those are compared whole, padding included.

Left out: NaN logits (the argmax of a row with NaN is unpinned), and lengths beyond the row width for merge_repeated and
edit_distance (the ABI does not pin them)."""
import functools

import numpy as np

GUARD = 64
PAD_OUT = 7.0
PAD_IN = float("nan")
SENTINEL = 0x7A7A7A7A
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 3e-4
BN_EPS = 1e-3
MARGIN = 4.0
HALF_ULP = 2.0 ** -24


def _rng(name, salt=0):
    return np.random.RandomState((sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 7919 * salt) % (2 ** 31))


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def same_bits(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    return got.shape == ref.shape and got.dtype == ref.dtype and bool(np.array_equal(bits(got), bits(ref)))


def ulps(a, b):
    """Distance of two positive finite f32 in units of the last place."""
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


class Placed:
    """A contiguous device view of arr's shape inside a larger buffer: [GUARD | off | data | GUARD]."""

    def __init__(self, arr, out, off=0):
        import torch
        arr = np.ascontiguousarray(arr)
        assert arr.dtype in (np.float32, np.int32)
        self.dtype = arr.dtype
        if arr.dtype == np.int32:
            self.pad = np.int32(SENTINEL)
        else:
            self.pad = np.float32(PAD_OUT if out else PAD_IN)
        n = arr.size
        host = np.full(GUARD + off + (n + 3) // 4 * 4 + GUARD, self.pad, arr.dtype)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        host[self.lo:self.hi] = arr.reshape(-1)
        self.before = host.copy()
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.hi].view(arr.shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 4 * off % 16

    def result(self):
        return self.view.cpu().numpy()

    def surroundings_intact(self):
        host = self.buf.cpu().numpy()
        return same_bits(host[:self.lo], self.before[:self.lo]) and same_bits(host[self.hi:], self.before[self.hi:])

    def untouched(self):
        """The whole buffer as it was placed (a refused call)."""
        return same_bits(self.buf.cpu().numpy(), self.before)


# ---- clip + Adam ----------------------------------------------------------------------------------------------------------------
SUMSQ_CAP, ADAM_CAP = 1024, 2048      # csrc/optim.hip: the grid caps of sumsq_kernel and clip_adam_kernel
ADAM_SIZES = (1, 3, 4, 5, 1023, 1048575, 1048579, 1048583, 2097159, 4200003)      # (1048583: the first n at which sumsq strides twice)
ADAM_CAPS = dict(norm=1e-4, p=2e-6, m=1e-4, v=1e-4)      # tests/test_gpu_kernels.py::test_clip_adam
BIG_CLIP = 1e9


def adam_geometry(n):
    """blocks and trips (of the busiest thread) of the two grid-stride loops over n // 4 float4s."""
    n4, want = n // 4, (n // 4 + 1 + 255) // 256
    g = {}
    for key, cap in (("sumsq", SUMSQ_CAP), ("adam", ADAM_CAP)):
        blocks = min(want, cap)
        g[key] = dict(blocks=blocks, capped=want > cap, stride4=blocks * 256, trips=max(1, -(-n4 // (blocks * 256))))
    g["tail"] = n % 4
    return g


def adam_case(name, n, kind, clip=BIG_CLIP, steps=1):
    return dict(name=name, n=n, kind=kind, clip=clip, steps=steps)


ADAM_CASES = [adam_case("ints-%d" % n, n, "ints") for n in ADAM_SIZES] + [
    # norm ~ 0.1 sqrt(n): below and above the clip
    adam_case("normal-5-unclipped", 5, "normal", clip=10.0, steps=3),
    adam_case("normal-5-clipped", 5, "normal", clip=0.05, steps=3),
    adam_case("normal-1023-unclipped", 1023, "normal", clip=100.0, steps=3),
    adam_case("normal-1023-clipped", 1023, "normal", clip=1.0, steps=3),
    adam_case("normal-2097159-unclipped", 2097159, "normal", clip=1000.0, steps=3),
    adam_case("normal-2097159-clipped", 2097159, "normal", clip=1.0, steps=3),
    adam_case("atclip-1048583", 1048583, "atclip", clip=1.0),
    adam_case("zero-5", 5, "zero", clip=1.0),
    adam_case("zero-1048583", 1048583, "zero", clip=1.0),
    adam_case("tiny-1023", 1023, "tiny", clip=1.0, steps=3),
    adam_case("tiny-1048583", 1048583, "tiny", clip=1.0, steps=3),
]
ADAM_REFUSED = ("unaligned-p", "unaligned-g", "unaligned-m", "unaligned-v", "clip-zero", "clip-negative")


def adam_case_by_name(name):
    return next(c for c in ADAM_CASES if c["name"] == name)


def adam_planted(n):
    """Indices that must carry a nonzero gradient: 0, n - 1, the scalar tail, both sides of every stride boundary of either loop."""
    idx = {0, n - 1} | set(range(n // 4 * 4, n))
    geo = adam_geometry(n)
    for key in ("sumsq", "adam"):
        for k in range(1, geo[key]["trips"] + 1):
            e = 4 * k * geo[key]["stride4"]
            idx |= {i for i in (e - 1, e, n // 4 * 4 - 1) if 0 <= i < n}
    return np.array(sorted(idx), np.int64)


def adam_operands(c, with_m=False):
    """p, g, m, v (f32).  g is the gradient of EVERY step (the engine re-accumulates; the optimiser does not care).
    with_m: the second run of the `zero` kind, m nonzero."""
    n, kind = c["n"], c["kind"]
    rng = _rng(c["name"])
    p = rng.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if kind == "ints":
        g = np.zeros(n, np.float32)
        k = min(n, 100000)
        where = rng.choice(n, size=k, replace=False) if n > 8 else np.arange(n)
        g[where] = rng.randint(-1, 2, size=len(where))
        planted = adam_planted(n)
        g[planted] = rng.choice([-1.0, 1.0], size=len(planted))
    elif kind == "atclip":
        g = np.zeros(n, np.float32)
        planted = adam_planted(n)
        rest = np.setdiff1d(rng.choice(n, size=70000, replace=False), planted)[:65536 - len(planted)]
        where = np.concatenate([planted, rest])
        assert len(where) == 65536
        g[where] = rng.choice([-1.0, 1.0], size=len(where)) * np.float32(2.0 ** -8)
        m = (rng.randn(n) * 0.1).astype(np.float32)
        v = (rng.randn(n) ** 2 * 0.01 + 1e-6).astype(np.float32)
    elif kind == "zero":
        g = np.zeros(n, np.float32)
        v = (rng.randn(n) ** 2 * 0.01 + 1e-6).astype(np.float32)
        if with_m:
            m = (rng.randn(n) * 0.1).astype(np.float32)
    elif kind == "tiny":
        g = (rng.randn(n) * 1e-12).astype(np.float32)
    else:
        g = (rng.randn(n) * 0.1).astype(np.float32)
        m = (rng.randn(n) * 0.1).astype(np.float32)
        v = (rng.randn(n) ** 2 * 0.01 + 1e-6).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v)


def lr_t(step, lr=LR):
    return lr * np.sqrt(1.0 - B2 ** step) / (1.0 - B1 ** step)


def adam_f64(o, clip, steps):
    """oracle.model.clip_and_adam in float64, `steps` steps with the same gradient -> per step (norm, p, m, v)."""
    from oracle import model as om
    p, g, m, v = ({"w": o[k].astype(np.float64)} for k in ("p", "g", "m", "v"))
    out = []
    for step in range(1, steps + 1):
        gn = om.clip_and_adam(p, g, m, v, step, LR, clip)
        out.append(dict(norm=gn, p=p["w"].copy(), m=m["w"].copy(), v=v["w"].copy()))
    return out


def _butterfly(acc):
    """The xor-shuffle sum of a wave: acc [waves, 64] -> [waves] (every lane ends with the same value; f32 + is commutative)."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


def sumsq_f32(g):
    """sqrtf of the sum of squares in the order of sumsq_kernel and the head of clip_adam_kernel, without FMA contraction."""
    g = np.ascontiguousarray(g, np.float32)
    n, n4 = g.size, g.size // 4
    geo = adam_geometry(n)["sumsq"]
    blocks, threads = geo["blocks"], geo["blocks"] * 256
    q = g[:n4 * 4].reshape(n4, 4)
    q = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    trips = -(-n4 // threads) if n4 else 0
    padded = np.zeros(max(trips, 1) * threads, np.float32)
    padded[:n4] = q
    acc = np.zeros(threads, np.float32)
    for row in padded.reshape(-1, threads)[:trips]:
        acc = acc + row      # (a thread past n4 adds nothing; adding +0 changes no sum)
    tail = g[n4 * 4:]
    acc[:len(tail)] = acc[:len(tail)] + tail * tail
    waves = _butterfly(acc.reshape(-1, 64)).reshape(blocks, 4)
    partial = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    padded = np.zeros(SUMSQ_CAP, np.float32)
    padded[:blocks] = partial
    acc = np.zeros(256, np.float32)
    for row in padded.reshape(4, 256)[:-(-blocks // 256)]:
        acc = acc + row
    red = _butterfly(acc.reshape(4, 64))
    return np.sqrt(((red[0] + red[1]) + red[2]) + red[3])


def adam_f32(o, clip, steps):
    """clip_adam_kernel restated in f32 numpy."""
    f = np.float32
    p, g, m, v = (o[k].astype(f) for k in ("p", "g", "m", "v"))
    b1, b2, eps, clip = f(B1), f(B2), f(EPS), f(clip)
    out = []
    for step in range(1, steps + 1):
        gn = f(sumsq_f32(g))
        scale = clip / max(gn, clip)
        gc = g * scale
        m = b1 * m + (f(1) - b1) * gc
        v = b2 * v + (f(1) - b2) * gc * gc
        p = p - f(lr_t(step)) * m / (np.sqrt(v) + eps)
        assert p.dtype == m.dtype == v.dtype == np.float32
        out.append(dict(norm=gn, p=p.copy(), m=m.copy(), v=v.copy()))
    return out


def adam_errors(got, ref):
    """One step's errors in the measures of test_clip_adam."""
    return dict(norm=abs(float(got["norm"]) - ref["norm"]) / (ref["norm"] if ref["norm"] > 0 else 1.0),
                p=float(np.abs(got["p"].astype(np.float64) - ref["p"]).max()), m=rel_err(got["m"], ref["m"]), v=rel_err(got["v"], ref["v"]))


@functools.lru_cache(maxsize=None)
def adam_measured(name):
    """The restatement's error against float64 per output: the worst over the case's steps."""
    c = adam_case_by_name(name)
    o = adam_operands(c, with_m=True)
    ref, f32 = adam_f64(o, c["clip"], c["steps"]), adam_f32(o, c["clip"], c["steps"])
    errs = [adam_errors(a, b) for a, b in zip(f32, ref)]
    floor = dict(norm=HALF_ULP, m=HALF_ULP, v=HALF_ULP, p=HALF_ULP * float(np.abs(ref[-1]["p"]).max()))
    return {k: max(floor[k], max(e[k] for e in errs)) for k in ADAM_CAPS}


def adam_bounds(name):
    return {k: min(MARGIN * e, ADAM_CAPS[k]) for k, e in adam_measured(name).items()}


# ---- batch norm -----------------------------------------------------------------------------------------------------------------
BN_SHAPES = ((1, 1, 1), (3, 2, 5), (2, 64, 128), (7, 5, 37), (5, 32, 512))
BN_DATA = ("randn", "offset", "constcol")
BN_MODES = ("xhat", "noxhat", "inplace")      # out of place with xhat; xhat=None; y aliasing x and dx aliasing dy
BN_SHARDS = {5: (3, 2), 32: (1, 4, 27)}       # batch size -> the unequal split of the data-parallel form
BN_OUTPUTS = ("y", "xhat", "inv_std", "dx_own", "dx")


def bn_case(shape, data):
    T, B, H = shape
    return dict(name="bn-%dx%dx%d-%s" % (T, B, H, data), T=T, B=B, H=H, data=data, shards=BN_SHARDS.get(B))


BN_CASES = [bn_case(s, d) for s in BN_SHAPES for d in BN_DATA]


def bn_case_by_name(name):
    return next(c for c in BN_CASES if c["name"] == name)


def bn_operands(c):
    rng = _rng(c["name"])
    T, B, H = c["T"], c["B"], c["H"]
    x = rng.randn(T, B, H).astype(np.float32)
    if c["data"] == "offset":
        x = (x + np.float32(100.0)).astype(np.float32)
    if c["data"] == "constcol":
        x[T // 2, :, H // 2] = np.float32(1.75)     # var exactly 0: y = 0, inv_std = rsqrt(eps)
    return dict(x=x, dy=rng.randn(T, B, H).astype(np.float32))


def bn_f64(o, xhat=None, inv=None):
    """oracle.model.batch_norm / batch_norm_backward in float64: y (= xhat), inv_std [T, H], dx; dx_own = the float64 backward of
    the given (the kernel's own) xhat and inv_std."""
    from oracle import model as om
    assert om.BN_EPS == BN_EPS
    y, i = om.batch_norm(o["x"].astype(np.float64))
    dy = o["dy"].astype(np.float64)
    r = dict(y=y, xhat=y, inv_std=i[:, 0, :], dx=om.batch_norm_backward(dy, y, i))
    if xhat is not None:
        r["dx_own"] = om.batch_norm_backward(dy, xhat.astype(np.float64), inv.astype(np.float64)[:, None, :])
    return r


def _seq_sum(a):
    """sum over axis 1 (b), sequentially from 0 in f32: the kernels' loops."""
    acc = np.zeros((a.shape[0], a.shape[2]), np.float32)
    for b in range(a.shape[1]):
        acc = acc + a[:, b, :]
    return acc


def _bn_bwd_f32(dy, xhat, inv, s1, s2):
    return inv[:, None, :] * (dy - s1[:, None, :] - xhat * s2[:, None, :])


def bn_f32(o):
    """bn_fwd_kernel / bn_bwd_kernel restated: two-pass variance, divisions by B, 1 / sqrt for rsqrtf."""
    f = np.float32
    x, dy = o["x"], o["dy"]
    B = f(x.shape[1])
    mean = _seq_sum(x) / B
    d = x - mean[:, None, :]
    var = _seq_sum(d * d) / B
    inv = (f(1) / np.sqrt(var + f(BN_EPS))).astype(f)
    y = d * inv[:, None, :]
    dx = _bn_bwd_f32(dy, y, inv, _seq_sum(dy) / B, _seq_sum(dy * y) / B)
    assert y.dtype == dx.dtype == inv.dtype == np.float32
    return dict(y=y, xhat=y, inv_std=inv, dx=dx, dx_own=dx)


def bn_one_pass_f32(o):
    """inv_std of the rewrite the suite must catch: var = E[x^2] - mean^2 in f32."""
    f = np.float32
    x = o["x"]
    B = f(x.shape[1])
    mean = _seq_sum(x) / B
    var = np.maximum(_seq_sum(x * x) / B - mean * mean, f(0))
    return (f(1) / np.sqrt(var + f(BN_EPS))).astype(f)


def bn_dp_f32(o, shards):
    """The data-parallel kernels restated: local sums per shard, added in shard order, times f32(1 / n)."""
    f = np.float32
    x, dy = o["x"], o["dy"]
    inv_n = f(1.0) / f(x.shape[1])
    cuts = np.cumsum((0,) + tuple(shards))
    parts = lambda a: [a[:, lo:hi, :] for lo, hi in zip(cuts[:-1], cuts[1:])]
    total = lambda xs: functools.reduce(lambda a, b: a + b, xs)
    gsum = total([_seq_sum(s) for s in parts(x)])
    mean = gsum * inv_n
    gsq = total([_seq_sum((s - mean[:, None, :]) * (s - mean[:, None, :])) for s in parts(x)])
    inv = (f(1) / np.sqrt(gsq * inv_n + f(BN_EPS))).astype(f)
    y = (x - mean[:, None, :]) * inv[:, None, :]
    s1 = total([_seq_sum(s) for s in parts(dy)]) * inv_n
    s2 = total([_seq_sum(a * b) for a, b in zip(parts(dy), parts(y))]) * inv_n
    dx = _bn_bwd_f32(dy, y, inv, s1, s2)
    assert y.dtype == dx.dtype == inv.dtype == np.float32
    return dict(y=y, xhat=y, inv_std=inv, dx=dx, dx_own=dx)


def bn_errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in BN_OUTPUTS if k in got and k in ref}


@functools.lru_cache(maxsize=None)
def bn_measured(name, shards=None):
    """The restatement's error against float64 per output (shards: of the data-parallel restatement)."""
    o = bn_operands(bn_case_by_name(name))
    f32 = bn_f32(o) if shards is None else bn_dp_f32(o, shards)
    return {k: max(e, HALF_ULP) for k, e in bn_errors(f32, bn_f64(o, f32["xhat"], f32["inv_std"])).items()}


def bn_bounds(name, shards=None):
    return {k: MARGIN * e for k, e in bn_measured(name, shards).items()}


# ---- reverse_sequences ----------------------------------------------------------------------------------------------------------
REV_SHAPES = ((1, 1, 4), (5, 3, 12), (17, 7, 132), (64, 2, 512))      # (17, 7, 132): T B H / 4 = 3927, no multiple of 256
REV_REFUSED = ("h-not-multiple-of-4", "in-place")


def rev_lengths(T, B):
    """Length vectors of B entries that together cover {-3, 0, 1, 2, T - 1, T, T + 5}."""
    want = [-3, 0, 1, 2, T - 1, T, T + 5]
    return [np.array([want[(i + j) % 7] for j in range(B)], np.int32) for i in range(0, 7, B)]


REV_CASES = [dict(name="rev-%dx%dx%d" % s, T=s[0], B=s[1], H=s[2], lengths=rev_lengths(s[0], s[1])) for s in REV_SHAPES]


def rev_case_by_name(name):
    return next(c for c in REV_CASES if c["name"] == name)


def rev_operands(c):
    rng = _rng(c["name"])
    s = (c["T"], c["B"], c["H"])
    return dict(x=rng.randn(*s).astype(np.float32), xi=rng.randint(-8, 9, size=s).astype(np.float32),
                yi=rng.randint(-8, 9, size=s).astype(np.float32), prior=rng.randint(-8, 9, size=s).astype(np.float32))


def rev_ref(x, lengths):
    from oracle import model as om
    return om.reverse_sequences(x, np.clip(lengths, 0, x.shape[0]))


def rev_masked(x, lengths):
    """x with zeros at and past each clamped length: what reversing twice gives."""
    t = np.arange(x.shape[0])[:, None, None]
    return np.where(t < np.clip(lengths, 0, x.shape[0])[None, :, None], x, np.zeros_like(x))


# ---- greedy decode --------------------------------------------------------------------------------------------------------------
SEAMS = (64, 256)      # the first frame of the next wave of a ballot, of the next 256-thread chunk


def collapse(path, length, blank):
    """The ids a planned best path decodes to: drop repeats of the previous FRAME, then blanks."""
    out, prev = [], -1
    for k in list(path)[:max(0, min(int(length), len(path)))]:
        if k != prev and k != blank:
            out.append(int(k))
        prev = k
    return out


def greedy_row(kind, T, C, rng, **kw):
    """-> dict(path [T], ties {t: (classes tied at the top)}, ninf [frames of all -inf], length, kind, ...)."""
    blank = C - 1
    lab = lambda: int(rng.randint(0, C - 1))
    path, ties, ninf = np.full(T, blank, np.int64), {}, []
    length = kw.get("length", T)
    if kind == "blank":
        pass
    elif kind == "random":
        path = rng.randint(0, C, size=T)
        path[rng.rand(T) < 0.3] = blank
        rep = rng.rand(T) < 0.3
        for t in range(1, T):
            if rep[t]:
                path[t] = path[t - 1]
    elif kind == "alternating":      # no blank, no repeat: every frame kept (C = 2 has one label: label, blank, label ...)
        a, b = (0, 1) if C > 2 else (0, blank)
        path = np.where(np.arange(T) % 2 == 0, a, b)
    elif kind in ("same", "lbl", "diff"):
        k = kw["seam"]
        a = lab()
        b = (a + 1) % (C - 1) if C > 2 else blank
        if kind == "same":
            path[k - 2:k + 2] = a
        elif kind == "lbl":
            path[k - 1], path[k + 1] = a, a
        else:
            path[k - 1], path[k] = a, b
    elif kind == "ties":
        for t, pair in kw["pairs"].items():
            path[t] = min(pair)
            ties[t] = tuple(pair)
    elif kind == "ninf":
        path[:] = 0
        ninf = list(range(T))
    else:
        raise ValueError(kind)
    return dict(kind=kind, seam=kw.get("seam"), path=np.asarray(path, np.int64), ties=ties, ninf=ninf, length=int(length))


def greedy_case(name, T, C, rows):
    rng = _rng(name)
    return dict(name=name, T=T, C=C, B=len(rows), rows=[greedy_row(k, T, C, rng, **kw) for k, kw in rows])


def _tie_rows(C):
    pairs = {0: (3, 9) if C > 9 else (0, 1)}                 # two classes in different lanes
    pairs[2] = (1, C - 1)                                    # a label and the blank
    if C > 64:
        pairs[4] = (C - 65, C - 1)                           # c and c + 64 in one lane (here: against the blank)
    if C > 66:
        pairs[6] = (1, 65)                                   # c and c + 64 in one lane, two labels
    if C > 129:
        pairs[8] = (1, 129)                                  # ... and c + 128 (the blank of C = 130)
    return ("ties", dict(pairs=pairs))


GREEDY_CASES = [
    greedy_case("greedy-t1-c2", 1, 2, [("alternating", {}), ("blank", {}), ("ninf", {})]),
    greedy_case("greedy-t63-c29", 63, 29, [("random", {}), ("alternating", dict(length=72)), ("blank", {})]),
    greedy_case("greedy-t64-c64", 64, 64, [("random", {}), ("alternating", {}), ("random", dict(length=1)), _tie_rows(64)]),
    greedy_case("greedy-t65-c65", 65, 65, [("same", dict(seam=64)), ("diff", dict(seam=64)), ("alternating", {}), _tie_rows(65),
                                           ("random", dict(length=0))]),
    greedy_case("greedy-t255-c80", 255, 80, [("alternating", {}), ("random", dict(length=0)), ("random", dict(length=264))]),
    greedy_case("greedy-t256-c80", 256, 80, [("alternating", {}), ("random", dict(length=265)), _tie_rows(80)]),
    greedy_case("greedy-t257-c130", 257, 130, [("same", dict(seam=256)), ("diff", dict(seam=256)), ("alternating", {}), _tie_rows(130),
                                               ("ninf", dict(length=70))]),
    greedy_case("greedy-t513-c29", 513, 29, [(k, dict(seam=s)) for s in SEAMS for k in ("same", "lbl", "diff")] +
                [("alternating", {}), ("alternating", dict(length=300)), ("random", dict(length=1)), ("blank", {})]),
    greedy_case("greedy-t513-c2", 513, 2, [("alternating", {}), ("lbl", dict(seam=64)), ("lbl", dict(seam=256)), ("random", dict(length=522))]),
]
GREEDY_WS_CASE = "greedy-t513-c29"      # run once more with the scratch of a CtcWorkspace


def greedy_case_by_name(name):
    return next(c for c in GREEDY_CASES + [CHAIN_CASE] if c["name"] == name)


def greedy_operands(c):
    """logits [T, B, C] f32, lengths, and the expected (ids [B, T] padded with C, out_len [B]) from the plan alone."""
    T, B, C = c["T"], c["B"], c["C"]
    rng = _rng(c["name"], 1)
    logits = (rng.randn(T, B, C) * 0.1).astype(np.float32)
    ids, out_len = np.full((B, T), C, np.int32), np.zeros(B, np.int32)
    for b, r in enumerate(c["rows"]):
        logits[np.arange(T), b, r["path"]] += np.float32(10.0)
        for t, tied in r["ties"].items():
            logits[t, b, list(tied)] = logits[t, b, tied[0]]
        for t in r["ninf"]:
            logits[t, b, :] = -np.inf
        n = max(0, min(r["length"], T))
        if n < T:      # frames past the length: strong non-blank logits that must be ignored
            logits[np.arange(n, T), b, (np.arange(n, T) * 7 + b) % (C - 1)] += np.float32(30.0)
        got = collapse(r["path"], r["length"], C - 1)
        ids[b, :len(got)] = got
        out_len[b] = len(got)
    return dict(logits=logits, lengths=np.array([r["length"] for r in c["rows"]], np.int32), ids=ids, out_len=out_len)


# ---- merge_repeated -------------------------------------------------------------------------------------------------------------
MERGE_T = 300
MERGE_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, MERGE_T)
MERGE_CONTENTS = ("equal", "distinct", "seamrun", "alternating", "pairs")
MERGE_MAX_T = 15360      # csrc/ctc.hip: T * 4 <= 60 KiB of LDS
MERGE_PAD = 99


def merge_row(content, n, T, rng):
    """A row of T ints: the first n are the sequence, the rest junk that must stay."""
    row = (1000 + rng.randint(0, 5, size=T)).astype(np.int32)
    i = np.arange(n)
    if content == "equal":
        row[:n] = 5
    elif content == "distinct":
        row[:n] = i % 7 + 7 * (i % 2)      # neighbours differ, values recur
    elif content == "seamrun":             # runs across 63 | 64 and 255 | 256, everything else distinct
        seq = i % 7 + 7 * (i % 2)
        for k in SEAMS:
            seq[max(0, k - 2):k + 2] = 40 + k
        row[:n] = seq[:n]
    elif content == "alternating":
        row[:n] = 3 + (i % 2)
    elif content == "pairs":               # a a b b a a ...: kept values recur two apart
        row[:n] = 3 + (i // 2) % 2
    elif content == "random":
        row[:n] = rng.randint(0, 3, size=n)
    else:
        raise ValueError(content)
    return row


def merge_ref(ids, lens, pad):
    """-> (ids, lens) after the merge: positions [kept, n) hold pad, positions >= n are as they were."""
    ids, out = ids.copy(), np.zeros(len(lens), np.int32)
    for r, n in enumerate(lens):
        seq = ids[r, :n]
        keep = np.ones(n, bool)
        keep[1:] = seq[1:] != seq[:-1]
        kept = seq[keep]
        ids[r, :n] = pad
        ids[r, :len(kept)] = kept
        out[r] = len(kept)
    return ids, out


def merge_operands(name):
    rng = _rng(name)
    if name == "merge-table":
        rows = [(c, n) for n in MERGE_LENGTHS for c in MERGE_CONTENTS]
        T = MERGE_T
    else:      # "merge-largest": one row of the largest accepted width, full
        rows, T = [("random", MERGE_MAX_T)], MERGE_MAX_T
    ids = np.stack([merge_row(c, n, T, rng) for c, n in rows])
    lens = np.array([n for _, n in rows], np.int32)
    want_ids, want_lens = merge_ref(ids, lens, MERGE_PAD)
    return dict(rows=rows, ids=ids, lens=lens, want_ids=want_ids, want_lens=want_lens)


MERGE_CASES = ("merge-table", "merge-largest")


# ---- edit_distance --------------------------------------------------------------------------------------------------------------
ED_M = (0, 1, 63, 64, 65, 127, 128, 129, 200)      # lengths of the SECOND sequence: the kernel's 64-column chunks
ED_N = (0, 1, 64, 300)
ED_LDA, ED_LDB = 303, 205
ED_MAX_LDB = 15359      # csrc/ctc.hip: (ldb + 1) * 4 <= 60 KiB of LDS
ED_GROUP = 70


def levenshtein(a, b):
    """Row-vectorised DP: cur[j] = min(cand[j], cur[j - 1] + 1) is a running minimum of cand[k] - k."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(len(b) + 1)
    prev = j.copy()
    for i, ai in enumerate(a, 1):
        cand = np.empty(len(b) + 1, np.int64)
        cand[0] = i
        cand[1:] = np.minimum(prev[:-1] + (b != ai), prev[1:] + 1)
        prev = np.minimum.accumulate(cand - j) + j
    return int(prev[-1])


@functools.lru_cache(maxsize=None)
def ed_pairs():
    """-> list of (kind, a, b, distance known by construction or None)."""
    rng = _rng("edit-distance")
    seq = lambda n, lo, hi: rng.randint(lo, hi, size=n).astype(np.int32)
    pairs = []
    for m in ED_M:
        b = seq(m, 0, 80)
        pairs.append(("identical", b.copy(), b, 0))
        if m >= 1:
            pairs.append(("drop-first", b[1:].copy(), b, 1))      # the insertion chain crosses every chunk boundary
            pairs.append(("drop-last", b[:-1].copy(), b, 1))
        for col in (64, 128):
            if m > col:
                pairs.append(("deletion-at-%d" % col, np.delete(b, col - 1), b, 1))
        for n in ED_N:
            pairs.append(("disjoint", seq(n, 0, 10), seq(m, 10, 20), max(n, m)))
            pairs.append(("random-2", seq(n, 0, 2), seq(m, 0, 2), None))
            pairs.append(("random-80", seq(n, 0, 80), seq(m, 0, 80), None))
    return pairs


def ed_pack(pairs, lda, ldb):
    """int32 [n, lda], [n], [n, ldb], [n]: sentinel garbage beyond both lengths."""
    n = len(pairs)
    a, b = np.full((n, lda), SENTINEL, np.int32), np.full((n, ldb), SENTINEL, np.int32)
    for i, (_, x, y, _) in enumerate(pairs):
        a[i, :len(x)], b[i, :len(y)] = x, y
    return a, np.array([len(p[1]) for p in pairs], np.int32), b, np.array([len(p[2]) for p in pairs], np.int32)


@functools.lru_cache(maxsize=None)
def ed_expected():
    out = []
    for kind, a, b, known in ed_pairs():
        d = levenshtein(a, b)
        assert known is None or d == known, (kind, len(a), len(b), d, known)
        out.append(d)
    return np.array(out, np.int32)


def ed_largest():
    """One pair with ldb = m = ED_MAX_LDB and n = 3."""
    rng = _rng("edit-distance-largest")
    b = rng.randint(0, 80, size=ED_MAX_LDB).astype(np.int32)
    a = np.array([b[5], 81, b[9000]], np.int32)
    return [("largest", a, b, None)]


ED_CASES = ("ed-table", "ed-single", "ed-largest")

# ---- the chain of AcousticModel: greedy -> merge_repeated (pad = C) -> edit_distance against the truths ---------------------------
CHAIN_CASE = greedy_case("chain-t70-c29", 70, 29, [("random", {}), ("random", dict(length=41)), ("alternating", {}), ("blank", {}),
                                                   ("same", dict(seam=64)), ("random", dict(length=0))])


def chain_operands():
    c = CHAIN_CASE
    o = greedy_operands(c)
    rng = _rng(c["name"], 2)
    U = 24
    truth, tlen = np.zeros((c["B"], U), np.int32), rng.randint(1, U + 1, size=c["B"]).astype(np.int32)
    for b in range(c["B"]):
        truth[b, :tlen[b]] = rng.randint(1, c["C"], size=tlen[b])
    return dict(o, truth=truth, tlen=tlen)


def chain_ref(o, C):
    """The oracle's decode, the merge in plain Python, the oracle's distance."""
    from oracle import model as om
    dec = om.greedy_decode(o["logits"], o["lengths"])
    merged = [[k for i, k in enumerate(r) if i == 0 or k != r[i - 1]] for r in dec]
    dist = [om.edit_distance(r, o["truth"][b, :o["tlen"][b]]) for b, r in enumerate(merged)]
    return merged, np.array(dist, np.int32)


# ---- axpy / fill ----------------------------------------------------------------------------------------------------------------
VEC_SIZES = (1, 255, 257, 524293)      # 2048 blocks of 256 = 524288: the last size takes a second trip
VEC_CAP = 2048
AXPY_A = 3.0
FILL_VALUE = float(np.float32(np.pi))      # a full mantissa


def vec_operands(n):
    rng = _rng("vec-%d" % n)
    x, y = rng.randint(-8, 9, size=n).astype(np.float32), rng.randint(-8, 9, size=n).astype(np.float32)
    return dict(x=x, y=y, axpy=(y.astype(np.int64) + 3 * x.astype(np.int64)).astype(np.float32))


# ---- coverage: every edge the tables were written for ----------------------------------------------------------------------------
def _geo(c):
    return adam_geometry(c["n"])


def _rows(kind, seam=None):
    return [(c, r) for c in GREEDY_CASES for r in c["rows"] if r["kind"] == kind and (seam is None or r["seam"] == seam)]


def _tie(pred):
    return any(pred(pair, c["C"]) for c, r in _rows("ties") for pair in r["ties"].values())


COVERAGE = {
    "adam: n below one float4": lambda: any(c["n"] < 4 for c in ADAM_CASES),
    "adam: sumsq at its cap, not beyond": lambda: any(c["kind"] == "ints" and _geo(c)["sumsq"]["blocks"] == SUMSQ_CAP and not _geo(c)["sumsq"]["capped"]
                                                      for c in ADAM_CASES),
    "adam: sumsq capped, one trip": lambda: any(c["kind"] == "ints" and _geo(c)["sumsq"]["capped"] and _geo(c)["sumsq"]["trips"] == 1 for c in ADAM_CASES),
    "adam: sumsq capped, two trips, tail 3": lambda: any(c["kind"] == "ints" and _geo(c)["sumsq"]["trips"] == 2 and _geo(c)["tail"] == 3 for c in ADAM_CASES),
    "adam: update grid uncapped beside it": lambda: any(c["kind"] == "ints" and not _geo(c)["adam"]["capped"] and _geo(c)["sumsq"]["capped"]
                                                        for c in ADAM_CASES),
    "adam: update grid capped, two trips, tail 3": lambda: any(c["kind"] == "ints" and _geo(c)["adam"]["capped"] and _geo(c)["adam"]["trips"] == 2 and
                                                               _geo(c)["tail"] == 3 for c in ADAM_CASES),
    "adam: three trips of the update": lambda: any(c["kind"] == "ints" and _geo(c)["adam"]["trips"] == 3 for c in ADAM_CASES),
    "adam: normal below and above the clip, at a capped size": lambda: {"normal-2097159-unclipped", "normal-2097159-clipped"} <= {c["name"] for c in ADAM_CASES},
    "adam: norm == clip": lambda: any(c["kind"] == "atclip" for c in ADAM_CASES),
    "adam: zero gradients": lambda: any(c["kind"] == "zero" for c in ADAM_CASES),
    "adam: sqrt(v) below eps": lambda: any(c["kind"] == "tiny" for c in ADAM_CASES),
    "bn: B = 1": lambda: any(c["B"] == 1 for c in BN_CASES),
    "bn: exactly one block": lambda: any(c["T"] * c["H"] == 256 for c in BN_CASES),
    "bn: a partial second block": lambda: any(256 < c["T"] * c["H"] < 512 for c in BN_CASES),
    "bn: offset data at B = 32": lambda: any(c["data"] == "offset" and c["B"] == 32 for c in BN_CASES),
    "bn: a constant column": lambda: any(c["data"] == "constcol" and c["B"] > 1 for c in BN_CASES),
    "bn: every aliasing form": lambda: set(BN_MODES) == {"xhat", "noxhat", "inplace"},
    "bn: shards (3, 2)": lambda: any(c["shards"] == (3, 2) for c in BN_CASES),
    "bn: shards (1, 4, 27)": lambda: any(c["shards"] == (1, 4, 27) for c in BN_CASES),
    "rev: float4 count no multiple of 256": lambda: any((c["T"] * c["B"] * c["H"] // 4) % 256 and c["T"] * c["B"] * c["H"] // 4 > 256 for c in REV_CASES),
    "rev: every length of the list in every shape": lambda: all({int(v) for ls in c["lengths"] for v in ls} ==
                                                                {-3, 0, 1, 2, c["T"] - 1, c["T"], c["T"] + 5} for c in REV_CASES),
    "greedy: every C": lambda: {2, 29, 64, 65, 80, 130} <= {c["C"] for c in GREEDY_CASES},
    "greedy: every T": lambda: {1, 63, 64, 65, 255, 256, 257, 513} <= {c["T"] for c in GREEDY_CASES},
    "greedy: T B no multiple of 4": lambda: any(c["T"] * c["B"] % 4 for c in GREEDY_CASES),
    "greedy: all blank": lambda: bool(_rows("blank")),
    "greedy: every frame kept across waves and chunks": lambda: any(c["T"] > 256 and r["length"] >= c["T"] and c["C"] > 2 for c, r in _rows("alternating")),
    "greedy: a row of -inf": lambda: bool(_rows("ninf")),
    "greedy: lengths 0, 1, T, T + 9": lambda: all(any(r["length"] == f(c["T"]) for c in GREEDY_CASES for r in c["rows"])
                                                  for f in (lambda T: 0, lambda T: 1, lambda T: T, lambda T: T + 9)),
    "greedy: tie in different lanes": lambda: _tie(lambda p, C: p[0] % 64 != p[1] % 64 and max(p) != C - 1),
    "greedy: tie of c and c + 64": lambda: _tie(lambda p, C: p[1] - p[0] == 64 and max(p) != C - 1),
    "greedy: tie of a label and the blank": lambda: _tie(lambda p, C: max(p) == C - 1),
    "merge: every length": lambda: set(MERGE_LENGTHS) == {0, 1, 2, 63, 64, 65, 255, 256, 257, MERGE_T},
    "merge: the largest accepted row": lambda: MERGE_MAX_T * 4 == 60 * 1024,
    "ed: every chunk boundary of m": lambda: {63, 64, 65, 127, 128, 129} <= {len(p[2]) for p in ed_pairs()},
    "ed: every (n, m) at random": lambda: {(n, m) for n in ED_N for m in ED_M} <= {(len(p[1]), len(p[2])) for p in ed_pairs() if p[0] == "random-80"},
    "ed: deletion at columns 64 and 128": lambda: {"deletion-at-64", "deletion-at-128"} <= {p[0] for p in ed_pairs()},
    "ed: groups of 70": lambda: len(ed_pairs()) >= 2 * ED_GROUP,
    "ed: lda != ldb": lambda: ED_LDA != ED_LDB and ED_LDA > max(ED_N) and ED_LDB > max(ED_M),
    "ed: the largest accepted second sequence": lambda: (ED_MAX_LDB + 1) * 4 == 60 * 1024,
    "vec: the grid cap on both sides": lambda: any(n <= VEC_CAP * 256 for n in VEC_SIZES) and any(VEC_CAP * 256 < n < VEC_CAP * 256 + 256 for n in VEC_SIZES),
}
for _k in ("same", "lbl", "diff"):
    for _s in SEAMS:
        COVERAGE["greedy: %s across %d | %d" % (_k, _s - 1, _s)] = (lambda k=_k, s=_s: bool(_rows(k, s)))
