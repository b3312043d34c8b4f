"""Cases, reference, metric and bounds for the CTC recursion kernels (csrc/ctc.hip, the head of csrc/ctc_flow.h).  Checker only:
numpy, no GPU, nothing of the product is imported.

The reference is oracle.model.ctc_loss_and_grad in float64 on the float32 logits (tests/test_cpu_ctc_ref.py holds it against
torch.nn.functional.ctc_loss autograd in float64).  What is here:

  build(case)        logits, dense labels, lengths of a case of CASES.  A case fixes what chance used to decide: the number of live
                     extended states S = 2 n + 1 of every row (up to smax = 2 U + 1: all U label slots used, no EOS), the rows'
                     lengths, where repeated labels sit (`rep`: the odd states s with ext[s] == ext[s - 2]), the alphabet, the kind
                     of logits and the seed; `plan` names the recursion kernel it must run under each setting of the switches
                     ("default"; "shift0": AMDSPEECH_CTC_SHIFT=0; "pair0": AMDSPEECH_CTC_SHIFT=0 AMDSPEECH_CTC_PAIR=0).
  slice_errors       the metric: per utterance and block of frames (the first and the last 16 valid frames on their own -- both
                     recursions start there -- and blocks of 64 between) the largest absolute error of dlogits; per utterance the
                     relative error of the loss.
  invariants         what needs no reference: over a valid frame t < len the row of dlogits sums to 0 (softmax sums to 1, the
                     occupancies sum to 1; to 1 where the loss is inf and the gradient is the softmax); rows of ignored utterances
                     and frames t >= len are exactly 0.
  emulate            the arithmetic of a kernel family on the CPU: log2 domain, the state in float64 (every kernel and the fused head;
                     family + "-f32": the float32 state three of them had) with float32 exp2 / log2 on the differences to the maximum, alpha / beta
                     rounded to float32 when stored, alpha + beta - ll in double, the posterior and the occupancies in float32.
                     `fault` plants one of three mistakes (FAULTS) for the proof that the metric has teeth.
  reach / closure    which (kernel, R), waves, repeat positions and final-lse splits a set of rows reaches, from a few lines restating
                     the thread layouts; REQUIRED is what the matrix must reach.

Bounds.  No bound comes from a GPU.  The bound of a slice is 8 x the error of the emulated arithmetic of the case's kernel family
against the float64 oracle ON THAT SLICE of that case (the factor the LSTM matrix uses: the emulation has numpy's exp2 / log2 where
the device has the 1-ulp v_exp_f32 / v_log_f32, no fused multiply-adds and another order of summation), not below a floor of a
few float32 roundings of a number of magnitude 1 (D_FLOOR: softmax and occupancy are each rounded once, so an emulation that
happens to land on the float64 value says nothing about the device's last bit), and never looser than the suite's figures: 2e-5
relative on the loss, 2e-3 absolute on dlogits, for the float64-state recursion 1e-3 of the tensor's maximum if that is less.

EMULATED (largest slice error of dlogits, relative error of the loss and row-sum defect of the emulated arithmetic against float64;
`PYTHONPATH=. python tests/ctc_ref.py` prints every case).  The last two columns are the same with the state in float32, which the
"wave", "pair" and "edge" kernels carried until this matrix was written: over the 2e-3 cap wherever long meets wide, which is why
they now carry float64 (csrc/ctc.hip) and why the bounds below are those of the float64 state.  What remains in the first columns
is the float32 STORAGE of alpha / beta in the workspace (|alpha| ~ 5 T natural-log units with random x 2 logits: one rounding of
2.4e-4 .. 9.8e-4), which the workspace layout fixes.

family  case           logits      T     S  | dlogits  loss     row sum | f32 state: dlogits  loss
wave    wave-full      random     67   127  | 2.1e-05  6.1e-08  2.2e-05 | 7.4e-05  1.3e-07
wave    large-wave     large      90    81  | 1.2e-04  5.5e-08  1.2e-04 | 3.0e-04  1.4e-07
shift   shift-full     random    203   383  | 8.0e-05  4.5e-08  8.0e-05 | (float64 since round 4)
shift   shift-long     random   1003   383  | 4.1e-04  4.2e-08  4.3e-04 |
pair    pair-full-255  random    263   511  | 1.0e-04  4.0e-08  1.0e-04 | 7.9e-04  3.7e-07
pair    pair-long      random   1001   511  | 4.2e-04  3.7e-08  4.3e-04 | 3.3e-03  8.0e-07
edge4   edge4-full     random    519  1023  | 1.8e-04  4.5e-08  1.9e-04 | 1.6e-03  3.7e-07
edge4   edge4-long     random   1001  1023  | 4.0e-04  5.7e-08  4.1e-04 | 4.4e-03  6.5e-07
edge4   large-edge4    large     310   601  | 4.9e-04  1.2e-08  4.9e-04 | 5.4e-03  4.8e-07
edge8   edge8-full     random   1031  2047  | 4.1e-04  4.9e-08  4.1e-04 | 7.8e-03  1.0e-06
edge20  edge20-long    random   1300  2201  | 4.5e-04  4.0e-08  4.6e-04 | 7.1e-03  9.6e-07
edge20  exact-U1100    random   1093  2181  | 4.3e-04  2.7e-08  4.3e-04 | 7.3e-03  3.1e-07
edge20  edge20-R       random   2563  5119  | 9.8e-04  5.1e-08  9.9e-04 | 2.5e-02  2.0e-06
(edge2 -- AMDSPEECH_CTC_PAIR=0 -- shares the pair rows: same cases, same arithmetic.)  8 x these is over the cap from T ~ 600 on, so
the long cases are bound by the cap itself; tests/test_cpu_ctc_ref.py asserts that the emulation stays under the cap on every slice.
"""
import functools

import numpy as np

from oracle import model as om

F32, F64 = np.float32, np.float64
LOG2E, LN2 = F32(1.4426950408889634), F32(0.6931471805599453)
FACTOR = 8.0
LOSS_CAP, D_CAP, D_CAP_REL64 = 2e-5, 2e-3, 1e-3
D_FLOOR = 2.0 ** -21          # softmax, occupancy, their difference and log p: four float32 roundings of magnitude <= 1 (2^-23 each)
LOSS_FLOOR = 2.0 ** -22       # the loss is stored as a float32 after two float32 multiplications (LOG2E, LN2) of its terms
MODES = {"default": {}, "shift0": {"AMDSPEECH_CTC_SHIFT": "0"}, "pair0": {"AMDSPEECH_CTC_SHIFT": "0", "AMDSPEECH_CTC_PAIR": "0"}}
FAULTS = ("skip_first", "late_halo", "final_one")


# ------------------------------------------------------------------------------------------------ the ladder, restated
def expected_plan(U, mode="default"):
    """(kernel, rmax, threads) of csrc/ctc.hip's ladder for a label width: restated here ONLY for the closure arithmetic; every case
    also names its plan literally, and the GPU test asserts the library's answer against that."""
    smax = 2 * U + 1
    if smax <= 128:
        return ("wave", 2, 64)
    if smax <= 384 and mode == "default":
        return ("shift", 2, 256)
    if smax <= 512:
        return ("pair", 2, 256) if mode != "pair0" else ("edge", 2, 256)
    return ("edge", 4 if smax <= 1024 else 8 if smax <= 2048 else 20, 256)


def family(plan):
    return plan[0] if plan[0] != "edge" else "edge%d" % plan[1]


def state_dtype(fam):
    """The type the family's recursion carries its state in.  Every kernel carries float64 now; the float32 state the "wave", "pair"
    and "edge" kernels had is kept as an emulation (fam + "-f32") because it is the finding that moved them: see EMULATED."""
    return F32 if fam.endswith("-f32") else F64


# ------------------------------------------------------------------------------------------------ cases
def row(n, length=None, eos=None, rep=(), kind="valid"):
    """One utterance: n target labels (S = 2 n + 1), `length` frames (None: T), eos: an EOS after the labels (None: where it fits),
    rep: odd states s >= 3 with ext[s] == ext[s - 2].  kind: "valid", "len0", "empty" (all-zero label row -> the all-blank target),
    "toolong" (more labels than frames: ignored), "impossible" (fits by count, but its repeats need more frames: loss inf)."""
    return dict(n=n, length=length, eos=eos, rep=tuple(rep), kind=kind)


def case(name, T, C, U, rows, plan, logits="random", seed=0, tags=()):
    return dict(name=name, T=T, C=C, U=U, rows=rows, plan=plan, logits=logits, seed=seed, tags=tuple(tags), B=len(rows))


WAVE, SHIFT, PAIR = ("wave", 2), ("shift", 2), ("pair", 2)
E2, E4, E8, E20 = ("edge", 2), ("edge", 4), ("edge", 8), ("edge", 20)
ALL_WAVE = {"default": WAVE, "shift0": WAVE, "pair0": WAVE}
MID = {"default": SHIFT, "shift0": PAIR, "pair0": E2}            # 129 .. 384 extended states
UPPER = {"default": PAIR, "shift0": PAIR, "pair0": E2}           # 385 .. 512


def _cases():
    c = []
    # ---- every kernel of the ladder at full width (S == smax), a shorter row beside it, T not a multiple of 16
    c.append(case("wave-full", 67, 80, 63, [row(63, eos=False), row(31, 50), row(32, 61, rep=(5,)), row(1, 3)], ALL_WAVE, seed=1))
    c.append(case("shift-full", 203, 80, 191, [row(191, eos=False, rep=(97, 193, 289, 95, 191, 287, 381)), row(95, 150), row(96, 203), row(143, 190), row(144, 201)],
                  MID, seed=2))
    c.append(case("pair-full-255", 263, 80, 255, [row(255, eos=False, rep=(509,)), row(127, 200), row(128, 262, rep=(3, 255)), row(254, 263)], UPPER, seed=3))
    c.append(case("pair-full-192", 198, 29, 192, [row(192, eos=False), row(96, 101), row(191, 197)], UPPER, seed=4))
    c.append(case("edge4-full", 519, 80, 511, [row(511, eos=False, rep=(1021,)), row(127, 140), row(128, 300), row(255, 270), row(256, 519, rep=(3, 513, 515)),
                                               row(383, 400), row(384, 500)], {"default": E4}, seed=5))
    c.append(case("edge8-full", 1031, 80, 1023, [row(1023, eos=False), row(127, 131), row(128, 133), row(255, 300), row(256, 1031), row(383, 390), row(384, 401, rep=(3, 7, 11, 767)),
                                                 row(511, 520), row(512, 530), row(639, 650), row(640, 700), row(767, 800), row(768, 801), row(895, 900),
                                                 row(896, 1000)], {"default": E8}, seed=6))
    c.append(case("edge20-R", 2563, 29, 2559, [row(2559, eos=False), row(127, 300), row(255, 263), row(256, 261, rep=(3, 513)), row(383, 777), row(895, 903), row(1663, 1669),
                                               row(2431, 2437), row(2432, 2563)], {"default": E20}, seed=7))
    # ---- the DPP-shift kernel: the last owned state of a wave and the first of the next; the 16-frame refresh
    for T in (15, 16, 17, 31, 33):
        n = min(T, 191)
        c.append(case("shift-T%d" % T, T, 80, 191, [row(n - 1, T), row(n // 2, T - 1), row(n, T, eos=False)], MID, seed=10 + T))
    c.append(case("shift-waves", 211, 80, 191, [row(95), row(96, 210), row(143, 200), row(144), row(191, eos=False)], MID, seed=20))
    c.append(case("shift-long", 1003, 80, 191, [row(191, eos=False), row(191, 1001, eos=False, rep=(97, 193, 289)), row(100, 999)], MID, seed=21, tags=("long",)))
    c.append(case("shift-161", 257, 80, 161, [row(161, eos=False), row(8, 200), row(91, 250)], MID, seed=22))
    # ---- two frames per exchange, default mode: T odd and even
    c.append(case("pair-T-even", 256, 80, 192, [row(192, eos=False), row(100, 255)], UPPER, seed=30))
    c.append(case("pair-T-odd", 257, 80, 255, [row(255, eos=False), row(254, 256), row(64, 129)], UPPER, seed=31))
    # ---- one-wave kernel: R = 1 and 2, S around the thread count
    c.append(case("wave-R", 70, 29, 40, [row(31), row(32), row(15, 33), row(40, eos=False), row(39)], ALL_WAVE, seed=32))
    # ---- dispatch edges (each asserts its plan; U = 2560 is refused: the GPU test and test_cpu_ctc_ref check that)
    for U, plan in ((63, ALL_WAVE), (64, MID), (191, MID), (192, UPPER), (255, UPPER), (256, {"default": E4}), (511, {"default": E4}),
                    (512, {"default": E8}), (1023, {"default": E8}), (1024, {"default": E20}), (2559, {"default": E20})):
        c.append(case("edge-U%d" % U, 45, 80, U, [row(min(U, 40), 45, eos=U > 40), row(7, 19), row(min(U, 21), 44, eos=True if U > 21 else None)], plan, seed=40 + U % 7))
    # ---- repeats on the first / second / third state of a thread (R = 3: 513 .. 768 live states), and on the last two states
    c.append(case("edge-R3-repeats", 420, 80, 600, [row(300, 420, rep=(3, 9, 13, 17, 301, 599)), row(383, 419, rep=(767, 765)), row(256, 300)],
                  {"default": E8}, seed=50))
    c.append(case("edge4-R1-repeats", 150, 80, 300, [row(100, 150, rep=(3, 5, 7, 129, 131, 199)), row(127, 149, rep=(255,))], {"default": E4}, seed=51))
    # ---- T at the edges
    for U, plan in ((12, ALL_WAVE), (100, MID), (200, UPPER), (300, {"default": E4})):
        for T in (1, 2, 7, 8, 9):
            c.append(case("T%d-U%d" % (T, U), T, 80, U, [row(min(T, 3), T, eos=False), row(max(T // 2, 1) if T > 1 else 1, T, eos=T > 1), row(T, T, eos=False)],
                          plan, seed=60 + T))
    for U, plan in ((60, ALL_WAVE), (150, MID), (250, UPPER), (400, {"default": E4}), (1100, {"default": E20})):
        # T == required time exactly (one alignment: the posterior is 0 or 1); T == required - 1 (ignored); repeats that make the
        # target impossible although required <= T (loss inf, gradient = softmax)
        n = U - 10
        c.append(case("exact-U%d" % U, n + 3, 80, U, [row(n, n, eos=False), row(n, n - 1, eos=False, kind="toolong"), row(n - 1, n, eos=True),
                                                      row(n, n + 3, eos=False, rep=(3, 7, 11, 2 * n - 1), kind="impossible"), row(20, n + 3),
                                                      row(n, n + 1, eos=False)],      # (one spare frame: every path runs at full speed but for one step)
                      plan, seed=70, tags=("inf",)))
    # ---- rows of every kind in one batch of a wide kernel; B = 1
    for U, plan in ((150, MID), (250, UPPER), (500, {"default": E4})):
        c.append(case("mixed-U%d" % U, 77, 80, U, [row(30, 77), row(5, 0, kind="len0"), row(0, 50, kind="empty"), row(70, 40, kind="toolong"),
                                                   row(60, 500, eos=True)], plan, seed=80))
        c.append(case("single-U%d" % U, 53, 80, U, [row(50, 53)], plan, seed=81))
    # ---- alphabets (C = 3: every label is 1 -- one LDS address in the gradient kernel; 4096: the ABI's maximum)
    for C in (3, 29, 64, 65, 80, 1000, 4096):
        c.append(case("C%d-wave" % C, 21, C, 10, [row(5, 21), row(3, 9), row(10, 20, eos=False)], ALL_WAVE, seed=90))
        c.append(case("C%d-wide" % C, 23, C, 300, [row(9, 23), row(4, 11)], {"default": E4}, seed=91))
    # ---- logits other than random
    for kind in ("peaky", "large"):
        c.append(case("%s-wave" % kind, 90, 80, 40, [row(40, eos=False), row(20, 70)], ALL_WAVE, logits=kind, seed=100))
        c.append(case("%s-mid" % kind, 230, 80, 170, [row(170, eos=False, rep=(97, 193)), row(90, 199)], MID, logits=kind, seed=101))
        c.append(case("%s-edge4" % kind, 310, 80, 300, [row(300, eos=False), row(150, 309)], {"default": E4}, logits=kind, seed=102))
    # ---- long and wide together: where the float32 state costs most
    c.append(case("edge20-long", 1300, 80, 1100, [row(1100, eos=False), row(1099, 1299), row(500, 1001)], {"default": E20}, seed=110, tags=("long",)))
    c.append(case("edge4-long", 1001, 80, 511, [row(511, eos=False), row(510, 1000)], {"default": E4}, seed=111, tags=("long",)))
    c.append(case("pair-long", 1001, 80, 255, [row(255, eos=False), row(254, 999), row(128, 1001)], UPPER, seed=112, tags=("long",)))
    c.append(case("mid-long", 1001, 80, 191, [row(191, eos=False), row(190, 1000)], MID, seed=113, tags=("long",)))
    return c


CASES = _cases()
# the suite's older parametrised cases (tests/test_gpu_kernels.py): (T, B, C, U), seed T + B -- the closure check must FAIL on these
OLD_CASES = [(30, 4, 80, 12), (101, 7, 80, 40), (257, 3, 80, 161), (64, 2, 29, 70), (300, 2, 80, 600), (600, 2, 80, 1100)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def runs():
    """(case, mode) pairs: a case runs under every setting of the switches its `plan` names."""
    return [(c, m) for c in CASES for m in MODES if m in c["plan"]]


def _labels(rng, n, C, rep):
    """n labels in 1 .. C-2, adjacent ones different except at the repeats (label u == label u-1 for every state s = 2u+1 in rep)."""
    lab = np.zeros(n, np.int64)
    repu = {(s - 1) // 2 for s in rep}
    for u in range(n):
        if u in repu and u > 0:
            lab[u] = lab[u - 1]
        elif C <= 3:
            lab[u] = 1
        else:
            v = rng.randint(1, C - 1)
            while u > 0 and v == lab[u - 1]:
                v = rng.randint(1, C - 1)
            lab[u] = v
    return lab


def build(c):
    """-> logits [T,B,C] float32, dense [B,U] int32, lengths [B] int32, info: per row dict(S, ext, valid, inf, Tb)."""
    T, B, C, U = c["T"], c["B"], c["C"], c["U"]
    rng = np.random.RandomState(1000 + c["seed"])
    dense = np.zeros((B, U), np.int32)
    lengths = np.zeros(B, np.int32)
    info = []
    for b, r in enumerate(c["rows"]):
        n = r["n"]
        assert n <= U
        lab = _labels(rng, n, C, r["rep"])
        dense[b, :n] = lab
        eos = r["eos"] if r["eos"] is not None else n < U
        if eos:
            assert n < U
            dense[b, n] = C - 1
        lengths[b] = T if r["length"] is None else r["length"]
        Tb = min(int(lengths[b]), T)
        kept = max(n + (1 if eos else 0), 1)
        valid = lengths[b] > 0 and kept <= lengths[b]
        nrep = int(sum(1 for u in range(1, n) if lab[u] == lab[u - 1]))
        inf = valid and n + nrep > Tb
        assert valid == (r["kind"] in ("valid", "empty", "impossible")), (c["name"], b)
        assert inf == (r["kind"] == "impossible"), (c["name"], b, n, nrep, Tb)
        ext = np.full(2 * n + 1, C - 1, np.int64)
        ext[1::2] = lab
        if C > 3:       # the builder put repeats exactly where the row says (C = 3: every label is 1)
            assert {s for s in range(3, 2 * n + 1, 2) if ext[s] == ext[s - 2]} == {s for s in r["rep"] if 3 <= s <= 2 * n}, (c["name"], b)
        info.append(dict(S=2 * n + 1, ext=ext, valid=bool(valid), inf=bool(inf), Tb=Tb, n=n, nrep=nrep))
    if c["logits"] == "random":
        logits = rng.randn(T, B, C).astype(F32) * F32(2.0)
    elif c["logits"] == "large":
        logits = rng.uniform(-40.0, 40.0, size=(T, B, C)).astype(F32)
    else:       # "peaky": a trained network's output -- one class stands out per frame, along a valid alignment of the target
        logits = rng.randn(T, B, C).astype(F32)
        for b, i in enumerate(info):
            if not i["valid"] or i["inf"]:
                continue
            path = _alignment(rng, i["ext"], i["Tb"])
            logits[np.arange(i["Tb"]), b, path] += F32(8.0)
    return logits, dense, lengths, info


def _alignment(rng, ext, Tb):
    """A valid alignment: every label state once or more, a blank between repeated labels, the other frames spread at random."""
    S = len(ext)
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    for s in range(3, S, 2):
        if ext[s] == ext[s - 2]:
            need[s - 1] = 1
    extra = Tb - int(need.sum())
    assert extra >= 0
    need += rng.multinomial(extra, np.ones(S) / S)
    return np.repeat(ext, need)


# ------------------------------------------------------------------------------------------------ the reference
def reference(logits, dense, lengths):
    """float64 loss [B] and dlogits [T,B,C] of the repository's oracle on the float32 logits."""
    with np.errstate(all="ignore"):
        return om.ctc_loss_and_grad(np.asarray(logits).astype(F64), om.sparsify_labels(dense, logits.shape[2]), np.asarray(lengths))


# ------------------------------------------------------------------------------------------------ the metric
def frame_blocks(Tb):
    """The valid frames of an utterance in blocks: the first 16 and the last 16 on their own, 64 at a time between."""
    if Tb <= 16:
        return [(0, Tb)] if Tb > 0 else []
    if Tb <= 32:
        return [(0, 16), (16, Tb)]
    mid = [(a, min(a + 64, Tb - 16)) for a in range(16, Tb - 16, 64)]
    return [(0, 16)] + mid + [(Tb - 16, Tb)]


def slice_errors(got_loss, got_d, ref_loss, ref_d, lengths):
    """-> {("loss", b): relative error, ("d", b, t0, t1): max abs error}; every utterance and every frame t < len is in one slice.
    An inf loss matches only inf (error 0), anything else there is an error of inf."""
    T, B, _ = ref_d.shape
    out = {}
    got_loss, ref_loss = np.asarray(got_loss, F64), np.asarray(ref_loss, F64)
    got_d, ref_d = np.asarray(got_d, F64), np.asarray(ref_d, F64)
    for b in range(B):
        if np.isinf(ref_loss[b]) or np.isnan(got_loss[b]) or np.isinf(got_loss[b]):
            out[("loss", b)] = 0.0 if got_loss[b] == ref_loss[b] else np.inf
        else:
            out[("loss", b)] = abs(got_loss[b] - ref_loss[b]) / max(abs(ref_loss[b]), 1e-30) if ref_loss[b] != 0 else abs(got_loss[b])
        for t0, t1 in frame_blocks(min(int(lengths[b]), T)):
            e = np.abs(got_d[t0:t1, b] - ref_d[t0:t1, b])
            out[("d", b, t0, t1)] = float(np.inf if np.isnan(e).any() else e.max())
    return out


def invariants(loss, d, lengths, valid, inf):
    """-> (largest |row sum - target| over the valid frames, count of non-zero values where exact zeros belong).  The target of a
    row sum is 0, and 1 where the loss is inf (gradient = softmax)."""
    T, B, C = d.shape
    d64 = np.asarray(d, F64)
    worst, dirty = 0.0, 0
    for b in range(B):
        Tb = min(int(lengths[b]), T) if valid[b] else 0
        dirty += int(np.count_nonzero(d[Tb:, b])) + int(np.isnan(d64[Tb:, b]).sum())
        if not valid[b]:
            dirty += int(loss[b] != 0)
            continue
        s = np.abs(d64[:Tb, b].sum(axis=1) - (1.0 if inf[b] else 0.0))
        worst = max(worst, float(np.inf if np.isnan(s).any() else s.max()))
    return worst, dirty


def rowsum_bound(emu_worst, C):
    """The row sum adds C float32 values of magnitude <= 1 (2^-24 each) to the slice's floor; else 8 x the emulation's, capped."""
    return min(D_CAP, FACTOR * max(emu_worst, D_FLOOR + C * 2.0 ** -24))


def bounds(emu_errors, fam, ref_d):
    """Per-slice bounds from the emulation's per-slice errors (same keys as slice_errors)."""
    cap_d = D_CAP
    if state_dtype(fam) is F64:
        cap_d = min(D_CAP, D_CAP_REL64 * float(np.abs(ref_d).max()))
    out = {}
    for k, e in emu_errors.items():
        if k[0] == "loss":
            out[k] = min(LOSS_CAP, FACTOR * max(e, LOSS_FLOOR))
        else:
            out[k] = min(cap_d, FACTOR * max(e, D_FLOOR))
    return out


# ------------------------------------------------------------------------------------------------ thread layouts, restated
def edge_R(S, threads):
    return -(-S // threads)


def reach(plan, S, rep, Tb):
    """What one valid row of S live states reaches in the kernel `plan` = (kernel, rmax, threads): a set of tags.
      ("R", family, R)            states per thread actually used (wave / edge kernels)
      ("wave", family, w)         the highest wave that holds a live state (256-thread kernels)
      ("rep", family, pos)        a repeat (skip flag off) on the thread's state `pos` (0 first, 1 second, ...) -- in the coordinates
                                  of the alpha recursion, and ("rep-b", ...) in those of the beta recursion
      ("rep-wave", "shift", w)    a repeat on the first owned label state of wave w of the DPP kernel (either direction)
      ("rep-last", family)        ext[S-2] == ext[S-4]
      ("fin", family, how)        the last two states sit in one thread / in two threads of a wave / in two waves
      ("S", family, k)            S = k mod threads for k in (1, threads - 1)  (S is odd: a multiple itself cannot occur)"""
    kernel, rmax, threads = plan
    fam = family(plan)
    out = set()
    if Tb < 1:
        return out
    if kernel in ("wave", "edge"):
        R = edge_R(S, threads)
        assert R <= rmax
        out.add(("R", fam, R))
        owner = lambda s: s // R
        for s in rep:
            out.add(("rep", fam, s % R))                  # alpha: skip[r] of state s
            out.add(("rep-b", fam, (s - 2) % R))          # beta: the flag sits on state s - 2
        if S % threads in (1, threads - 1):
            out.add(("S", fam, S % threads))
    elif kernel == "pair":
        owner = lambda s: s // 2
        for s in rep:
            out.add(("rep", fam, s % 2))
            out.add(("rep-b", fam, (S - 1 - (s - 2)) % 2))
    else:
        owner = lambda s: 64 * (s // 96) + 16 + (s % 96) // 2      # wave w owns 96 w .. 96 w + 95, two states per lane from lane 16
        for s in rep:
            if s % 96 == 1:
                out.add(("rep-wave", "shift", s // 96))
            k = S - 1 - (s - 2)                                     # the beta recursion's coordinate of the flagged state
            if k % 96 == 1:
                out.add(("rep-wave-b", "shift", k // 96))
    if threads == 256:
        out.add(("wave", fam, owner(S - 1) // 64))
    if S >= 2:
        a, b = owner(S - 2), owner(S - 1)
        out.add(("fin", fam, "thread" if a == b else "wave" if a // 64 == b // 64 else "waves"))
    if S - 2 in rep:
        out.add(("rep-last", fam))
    if Tb % 2 == 0:
        out.add(("T-even", fam))
    else:
        out.add(("T-odd", fam))
    return out


def reached(rows_by_plan):
    """Union of reach() over (plan, S, rep, Tb) tuples."""
    out = set()
    for plan, S, rep, Tb in rows_by_plan:
        out |= reach(plan, S, rep, Tb)
    return out


def matrix_rows(cases=None):
    """(plan, S, rep, Tb) of every valid, possible row of the matrix under every mode it runs in."""
    out = []
    for c in (CASES if cases is None else cases):
        _, _, _, info = build(c)
        for mode, kr in c["plan"].items():
            plan = expected_plan(c["U"], mode)
            assert plan[:2] == tuple(kr), (c["name"], mode, plan, kr)
            for i, r in zip(info, c["rows"]):
                if i["valid"] and not i["inf"]:
                    rep = tuple(s for s in range(3, i["S"], 2) if i["ext"][s] == i["ext"][s - 2])
                    out.append((plan + (), i["S"], rep, i["Tb"]))
    return out


def old_rows():
    """The same for the six older cases of tests/test_gpu_kernels.py (its make_ctc_case, restated draw for draw), all three modes."""
    out = []
    for T, B, C, U in OLD_CASES:
        rng = np.random.RandomState(T + B)
        rng.randn(T, B, C)
        lengths = rng.randint(max(1, T // 2), T + 1, size=B)
        for b in range(B):
            n = rng.randint(1, max(2, min(U - 1, int(lengths[b]) // 2 + 1)))
            lab = rng.randint(1, C - 1, size=n)
            if n > 2 and b % 2 == 0:
                lab[1] = lab[0]
            rep = tuple(2 * u + 1 for u in range(1, n) if lab[u] == lab[u - 1])
            for mode in MODES:
                out.append((expected_plan(U, mode), 2 * n + 1, rep, int(lengths[b])))
    return out


def _required():
    req = set()
    req |= {("R", "wave", 1), ("R", "wave", 2), ("S", "wave", 63), ("S", "wave", 1)}
    for rmax, rs in ((2, (1, 2)), (4, (1, 2, 3, 4)), (8, range(1, 9)), (20, (1, 2, 3, 7, 13, 19, 20))):
        fam = "edge%d" % rmax
        req |= {("R", fam, R) for R in rs}
        req |= {("S", fam, 255), ("S", fam, 1)}
        req |= {("wave", fam, w) for w in range(4)}
        req |= {("fin", fam, "wave")} | ({("fin", fam, "thread")} if rmax > 2 else set())      # (two states per thread: S - 2 and S - 1 never share one)
    for fam in ("shift", "pair"):
        req |= {("wave", fam, w) for w in range(4)}
        req |= {("T-even", fam), ("T-odd", fam), ("rep-last", fam)}
    req |= {("rep-wave", "shift", w) for w in (1, 2, 3)} | {("rep-wave-b", "shift", w) for w in (1, 2, 3)}
    req |= {("fin", "shift", "wave"), ("fin", "shift", "waves"), ("fin", "pair", "wave"), ("fin", "pair", "waves"), ("fin", "edge4", "waves"),
            ("fin", "wave", "wave")}
    # a repeat on the first (R = 1, 3), the second and the third state of a thread, in both recursions; on the target's last label
    req |= {("rep", "edge4", 0), ("rep", "edge8", 0), ("rep", "edge8", 1), ("rep", "edge8", 2), ("rep-b", "edge8", 0), ("rep-b", "edge8", 1),
            ("rep", "edge2", 1), ("rep", "pair", 1), ("rep", "wave", 0), ("rep-last", "edge4"), ("rep-last", "edge8"), ("rep-last", "edge2")}
    return req


REQUIRED = _required()
# states the DPP kernel's waves begin and end at, frames around its 16-frame refresh: (kernel, S) and (kernel, T) that must occur
REQUIRED_S = {("shift", S) for S in (191, 193, 287, 289, 383)} | {("pair", 385), ("pair", 511)}
REQUIRED_T = {("shift", T) for T in (15, 16, 17, 31, 33)}


def closure_missing(rows):
    """What REQUIRED / REQUIRED_S / REQUIRED_T name and `rows` ((plan, S, rep, Tb) tuples) do not reach."""
    got = reached(rows)
    miss = set(REQUIRED) - got
    miss |= {("S=",) + k for k in REQUIRED_S if not any(p[0] == k[0] and S == k[1] for p, S, _, _ in rows)}
    miss |= {("T=",) + k for k in REQUIRED_T if not any(p[0] == k[0] and Tb == k[1] for p, _, _, Tb in rows)}
    if not any(p[0] == "shift" and S == 383 and Tb >= 1001 for p, S, _, Tb in rows):
        miss.add(("long", "shift"))
    return miss


# ------------------------------------------------------------------------------------------------ the emulation
def _lse3(a, b, c, dt):
    """lse3_2 / lse3_2d of csrc/ctc_core.h: the maximum in the state's type, exp2 / log2 in float32 on the differences."""
    mm = np.maximum(np.maximum(a, np.maximum(b, c)), dt(-1e30))
    with np.errstate(divide="ignore"):
        e = np.exp2((a - mm).astype(F32)) + np.exp2((b - mm).astype(F32)) + np.exp2((c - mm).astype(F32))
        return mm + np.log2(e).astype(dt)


def _shift(x, k, dt):
    out = np.full_like(x, -np.inf)
    out[k:] = x[:len(x) - k]
    return out


def _chain(em, skip, dt, skip_fault=None):
    """The alpha recursion over em [Tb,S] (float32 emissions, log2 units) in the state type dt.  Returns n [Tb,S] (with the frame's
    emission: alpha) and v [Tb,S] (before it: beta, when run in the reversed coordinates) as float32 natural logs, and the last state."""
    Tb, S = em.shape
    NEG = dt(-np.inf)
    cur = np.full(S, NEG, dt)
    cur[:2] = em[0, :2].astype(dt)
    n_out = np.empty((Tb, S), F32)
    v_out = np.empty((Tb, S), F32)
    ln2 = dt(LN2)
    n_out[0] = cur.astype(F32) * LN2                            # (step 0: a float32 product in every kernel)
    v_out[0] = np.where(np.arange(S) < 2, F32(0), F32(-np.inf))
    sk = skip if skip_fault is None else skip & ~skip_fault
    for i in range(1, Tb):
        p1 = _shift(cur, 1, dt)
        p2 = np.where(sk, _shift(cur, 2, dt), NEG)
        v = _lse3(cur, p1, p2, dt)
        cur = v + em[i].astype(dt)
        n_out[i] = (cur * ln2).astype(F32)
        v_out[i] = (v * ln2).astype(F32)
    return n_out, v_out, cur


def _chain_shift_waves(em, skip, late_wave=None):
    """ctc_alpha_beta3_kernel as it is laid out: four waves of 128 consecutive states, the lowest 32 of a wave copies of the previous
    wave's highest 32, recomputed with everything else (the lane below lane 0 is -inf, so the copies go stale from the bottom, two
    states per frame) and refreshed through LDS every 16 frames.  late_wave: that wave takes every second refresh one frame late, after 17 frames
    (a planted fault).  Same returns as _chain."""
    Tb, S = em.shape
    dt = F64
    idx = np.arange(4)[:, None] * 96 - 32 + np.arange(128)[None, :]           # the state a (wave, slot) holds
    act = (idx >= 0) & (idx < S)
    safe = np.clip(idx, 0, S - 1)
    cur = np.where(act & (idx < 2), em[0][safe].astype(dt), -np.inf)
    skw = np.where(act, skip[safe], False)
    own = act & (np.arange(128)[None, :] >= 32)
    n_out = np.full((Tb, S), -np.inf, F32)
    v_out = np.full((Tb, S), -np.inf, F32)
    n_out[0][idx[own]] = cur[own].astype(F32) * LN2
    v_out[0] = np.where(np.arange(S) < 2, F32(0), F32(-np.inf))
    ln2 = dt(LN2)

    def refresh(w):
        cur[w, :32] = cur[w - 1, 96:]

    for i in range(1, Tb):
        for w in (1, 2, 3):
            on_time = i > 1 and (i - 1) % 16 == 0
            if (on_time and w != late_wave) or (w == late_wave and ((i - 1) % 32 == 16 or (i > 2 and (i - 2) % 32 == 0))):
                refresh(w)
        p1 = np.full_like(cur, -np.inf)
        p1[:, 1:] = cur[:, :-1]
        p2 = np.full_like(cur, -np.inf)
        p2[:, 2:] = cur[:, :-2]
        p2 = np.where(skw, p2, -np.inf)
        v = _lse3(cur, p1, p2, dt)
        cur = np.where(act, v + em[i][safe].astype(dt), -np.inf)
        n_out[i][idx[own]] = (cur[own] * ln2).astype(F32)
        v_out[i][idx[own]] = (v[own] * ln2).astype(F32)
    last = np.full(S, -np.inf, dt)
    last[idx[own]] = cur[own]
    return n_out, v_out, last


def log_softmax32(logits):
    """log_softmax_kernel in float32 (the order of the sum over C is numpy's)."""
    x = np.asarray(logits, F32)
    m = x.max(axis=2, keepdims=True)
    s = np.exp(x - m).sum(axis=2, keepdims=True, dtype=F32)
    return x - (m + np.log(s))


def emulate(logits, dense, lengths, plan, fault=None, fam=None):
    """Loss [B] and dlogits [T,B,C] (float32) by the arithmetic of the kernel `plan` = (kernel, rmax, threads) takes.
    fault: None or one of FAULTS --
      "skip_first"  the skip flag of every thread's FIRST state is dropped (wave / edge layout: state s with s % R == 0)
      "late_halo"   wave 2 of the DPP kernel takes every second halo refresh one frame late
      "final_one"   the final log-sum-exp takes only state S - 1"""
    T, B, C = logits.shape
    kernel, rmax, threads = plan
    fam = fam or family(plan)
    dt = state_dtype(fam)
    blank = C - 1
    logp = log_softmax32(logits)
    loss = np.zeros(B, F32)
    d = np.zeros((T, B, C), F32)
    rows = om.sparsify_labels(dense, C)
    for b in range(B):
        tgt, required = om.ctc_targets(rows[b], C)
        Tb = min(int(lengths[b]), T)
        if lengths[b] <= 0 or required > lengths[b]:
            continue
        ext = np.full(2 * len(tgt) + 1, blank, np.int64)
        ext[1::2] = tgt
        S = len(ext)
        skip = np.zeros(S, bool)
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        lp = logp[:Tb, b, :]
        em = lp[:, ext] * LOG2E                                    # float32
        rext = ext[::-1]
        rskip = np.zeros(S, bool)
        rskip[2:] = (rext[2:] != blank) & (rext[2:] != rext[:-2])
        rem = em[::-1, ::-1]
        fa = fb = None
        if fault == "skip_first":
            R = edge_R(S, threads)
            first = np.arange(S) % R == 0
            fa = first                                             # alpha: the flag of state s
            fb = first[::-1].copy()                                # beta: the flag of the transition s -> s + 2 sits on state s = S - 1 - k
        if kernel == "shift" and (fault == "late_halo" or fam == "shift-waves"):
            late = 2 if fault == "late_halo" else None
            alpha, _, last = _chain_shift_waves(em, skip, late)
            _, beta_r, _ = _chain_shift_waves(np.ascontiguousarray(rem), rskip, late)
        else:
            alpha, _, last = _chain(em, skip, dt, fa)
            _, beta_r, _ = _chain(np.ascontiguousarray(rem), rskip, dt, fb)
        beta = beta_r[::-1, ::-1]
        NEG = dt(-np.inf)
        a1 = last[S - 1]
        a2 = last[S - 2] if S > 1 and fault != "final_one" else NEG
        ll2 = _lse3(np.array([a1], dt), np.array([a2], dt), np.array([NEG], dt), dt)[0]
        ll = F32(ll2 * dt(LN2)) if dt is F64 else F32(ll2) * LN2
        loss[b] = -ll
        y = np.exp(lp)
        if np.isneginf(ll):
            d[:Tb, b] = y
            continue
        post = np.exp((alpha.astype(F64) + beta.astype(F64) - F64(ll)).astype(F32))      # [Tb,S] float32
        occ = np.zeros((Tb, C), F32)
        np.add.at(occ, (np.arange(Tb)[:, None], ext[None, :]), post)
        d[:Tb, b] = y - occ
    return loss, d


@functools.lru_cache(maxsize=None)
def evaluated(name, mode="default", fam=None):
    """(inputs, reference, emulation, bounds, info) of a case under a mode, computed once per process."""
    c = by_name(name)
    logits, dense, lengths, info = build(c)
    ref_loss, ref_d = reference(logits, dense, lengths)
    plan = expected_plan(c["U"], mode)
    fam = fam or family(plan)
    with np.errstate(all="ignore"):
        emu_loss, emu_d = emulate(logits, dense, lengths, plan, fam=fam)
    emu_err = slice_errors(emu_loss, emu_d, ref_loss, ref_d, lengths)
    valid = [i["valid"] for i in info]
    inf = [i["inf"] for i in info]
    emu_inv = invariants(emu_loss, emu_d, lengths, valid, inf)
    return dict(case=c, logits=logits, dense=dense, lengths=lengths, info=info, ref_loss=ref_loss, ref_d=ref_d, emu_loss=emu_loss, emu_d=emu_d,
                emu_err=emu_err, bounds=bounds(emu_err, fam, ref_d), valid=valid, inf=inf, emu_rowsum=emu_inv[0], fam=fam, plan=plan)


def judge(ev, got_loss, got_d):
    """-> (failures, worst ratio of error to bound): every slice of a result against its bound, then the invariants."""
    errs = slice_errors(got_loss, got_d, ev["ref_loss"], ev["ref_d"], ev["lengths"])
    assert set(errs) == set(ev["bounds"])
    fails, worst = [], 0.0
    for k, e in sorted(errs.items(), key=str):
        ratio = e / ev["bounds"][k] if e > 0 else 0.0
        worst = max(worst, ratio)
        if not e <= ev["bounds"][k]:
            fails.append("%s: error %.3g > bound %.3g (emulated %.3g)" % (k, e, ev["bounds"][k], ev["emu_err"][k]))
    rs, dirty = invariants(np.asarray(got_loss), np.asarray(got_d), ev["lengths"], ev["valid"], ev["inf"])
    rb = rowsum_bound(ev["emu_rowsum"], ev["case"]["C"])
    worst = max(worst, rs / rb)
    if not rs <= rb:
        fails.append("row sums: %.3g > bound %.3g (emulated %.3g)" % (rs, rb, ev["emu_rowsum"]))
    if dirty:
        fails.append("%d values that must be exactly 0 are not" % dirty)
    for b, (v, i) in enumerate(zip(ev["valid"], ev["inf"])):
        if i and not np.isposinf(np.asarray(got_loss)[b]):
            fails.append("row %d: loss %r, inf expected" % (b, got_loss[b]))
        if v and not i and not (np.isfinite(got_loss[b]) and got_loss[b] > 0):
            fails.append("row %d: loss %r, finite and positive expected" % (b, got_loss[b]))
    return fails, worst


if __name__ == "__main__":
    import time
    t0 = time.time()
    print("%-22s %-8s %-7s %5s %5s | dlogits  loss     rowsum" % ("case", "mode", "family", "T", "Smax"))
    for c, mode in runs():
        ev = evaluated(c["name"], mode)
        dmax = max(e for k, e in ev["emu_err"].items() if k[0] == "d") if any(k[0] == "d" for k in ev["emu_err"]) else 0.0
        lmax = max(e for k, e in ev["emu_err"].items() if k[0] == "loss")
        print("%-22s %-8s %-7s %5d %5d | %.1e  %.1e  %.1e   %.1fs" % (c["name"], mode, ev["fam"], c["T"], max(i["S"] for i in ev["info"]), dmax, lmax,
                                                                      ev["emu_rowsum"], time.time() - t0), flush=True)
