"""Exact and float64 parity of the small kernels per entry point, at their edges: every case of tests/small_ref.py -- clip + Adam
(both grid-stride loops past their caps, the scalar tail, norm == clip, zero and tiny gradients), batch norm (fused and data parallel
with unequal shards, out of place, without xhat and in place), reverse_sequences, greedy decode, merge_repeated, edit_distance, their
chain as AcousticModel runs it, axpy and fill.  Operands are contiguous views inside larger buffers (NaN or a sentinel around inputs,
7.0 or the sentinel around outputs, owed back bit for bit); integer and copied results are owed exactly, float results within 4 x the
error of small_ref's f32 restatement against float64 on the same inputs.  Every case prints one line, SMALLK <name> ..."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ref as R  # noqa: E402
from oracle import model as om  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from rnn_speech_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from rnn_speech_amd import lib as l
    return l


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def out_like(shape, dtype=F32):
    """An output placed with prior contents the call must replace."""
    return R.Placed(np.full(shape, -5, dtype), out=True)


def assert_intact(*placed):
    for i, pl in enumerate(placed):
        assert pl.surroundings_intact(), "the surroundings of output %d were written" % i


# ---- clip + Adam ----------------------------------------------------------------------------------------------------------------
def run_adam(ops, o, clip, steps, off=None):
    """-> (per step dict(norm, p, m, v), the placed buffers); off: {"p": 1} places that buffer one float off 16 bytes."""
    off = off or {}
    pl = {k: R.Placed(o[k], out=k != "g", off=off.get(k, 0)) for k in ("p", "g", "m", "v")}
    pl["norm"] = out_like(1)
    out = []
    for step in range(1, steps + 1):
        ops.clip_adam(pl["p"].view, pl["g"].view, pl["m"].view, pl["v"].view, clip, float(R.lr_t(step)), beta1=R.B1, beta2=R.B2, eps=R.EPS,
                      norm_out=pl["norm"].view)
        torch.cuda.synchronize()
        out.append(dict(norm=pl["norm"].result()[0], p=pl["p"].result(), m=pl["m"].result(), v=pl["v"].result()))
    assert_intact(pl["p"], pl["m"], pl["v"], pl["norm"])
    assert pl["g"].untouched()
    return out, pl


def adam_against_float64(name, got, o, clip, steps):
    ref, bounds = R.adam_f64(o, clip, steps), R.adam_bounds(name)
    worst = {k: 0.0 for k in bounds}
    for g, r in zip(got, ref):
        assert all(np.isfinite(g[k]).all() for k in g)
        for k, e in R.adam_errors(g, r).items():
            worst[k] = max(worst[k], e)
    return worst, bounds


@pytest.mark.parametrize("name", [c["name"] for c in R.ADAM_CASES])
def test_clip_adam_case(ops, name):
    c = R.adam_case_by_name(name)
    o = R.adam_operands(c)
    got, _ = run_adam(ops, o, c["clip"], c["steps"])
    one, b1, b2 = F32(1), F32(R.B1), F32(R.B2)
    line = ""
    if c["kind"] == "ints":
        g, s = o["g"], got[0]
        S = int((g.astype(np.int64) ** 2).sum())
        d = R.ulps(s["norm"], F32(np.sqrt(S)))
        line = "S=%d norm=%r ulps=%d" % (S, float(s["norm"]), d)
        print("SMALLK adam %s %s" % (name, line))
        assert d <= 1, line
        assert R.same_bits(s["m"], (one - b1) * g), "m is not (1 - b1) g at %s" % np.flatnonzero(s["m"] != (one - b1) * g)[:8]
        assert R.same_bits(s["v"], (one - b2) * g * g), "v is not (1 - b2) g^2 at %s" % np.flatnonzero(s["v"] != (one - b2) * g * g)[:8]
        z = g == 0
        assert R.same_bits(s["p"][z], o["p"][z]), "p moved under a zero gradient"
        ref = R.adam_f64(o, c["clip"], 1)[0]
        assert np.all(s["p"][~z] != o["p"][~z]) and np.abs(s["p"] - ref["p"]).max() < R.ADAM_CAPS["p"]
        return
    if c["kind"] == "atclip":
        big, _ = run_adam(ops, o, R.BIG_CLIP, 1)
        print("SMALLK adam %s norm=%r norm(clip=1e9)=%r" % (name, float(got[0]["norm"]), float(big[0]["norm"])))
        assert R.same_bits(got[0]["norm"], F32(1.0)) and R.same_bits(big[0]["norm"], F32(1.0))
        for k in ("p", "m", "v"):
            assert R.same_bits(got[0][k], big[0][k]), "%s differs between clip = norm and clip = 1e9" % k
        assert not R.same_bits(got[0]["p"], o["p"])
        return
    if c["kind"] == "zero":
        s = got[0]
        assert R.same_bits(s["norm"], F32(0.0)) and R.same_bits(s["p"], o["p"]) and R.same_bits(s["m"], o["m"]) and R.same_bits(s["v"], b2 * o["v"])
        o = R.adam_operands(c, with_m=True)
        got, _ = run_adam(ops, o, c["clip"], c["steps"])
        s = got[0]
        assert R.same_bits(s["norm"], F32(0.0)) and R.same_bits(s["m"], b1 * o["m"]) and R.same_bits(s["v"], b2 * o["v"])
    worst, bounds = adam_against_float64(name, got, o, c["clip"], c["steps"])
    print("SMALLK adam %s" % name, " ".join("%s=%.3g(bound %.3g)" % (k, worst[k], bounds[k]) for k in sorted(worst)))
    for k in worst:
        assert worst[k] <= bounds[k], (k, worst[k], bounds[k])


@pytest.mark.parametrize("what", R.ADAM_REFUSED)
def test_clip_adam_refuses(ops, lib, what):
    """A buffer one float off 16 bytes, clip <= 0: an error, nothing written."""
    o = R.adam_operands(R.adam_case_by_name("normal-1023-clipped"))
    off = {what[-1]: 1} if what.startswith("unaligned") else {}
    clip = {"clip-zero": 0.0, "clip-negative": -1.0}.get(what, 1.0)
    pl = {k: R.Placed(o[k], out=k != "g", off=off.get(k, 0)) for k in ("p", "g", "m", "v")}
    pl["norm"] = out_like(1)
    with pytest.raises(lib.AmdSpeechError, match="16-byte aligned" if off else "clip must be positive"):
        ops.clip_adam(pl["p"].view, pl["g"].view, pl["m"].view, pl["v"].view, clip, 1e-4, norm_out=pl["norm"].view)
    torch.cuda.synchronize()
    assert all(x.untouched() for x in pl.values())
    print("SMALLK adam refuses %s" % what)


# ---- batch norm -----------------------------------------------------------------------------------------------------------------
def run_bn_fused(ops, o, mode):
    x, dy = o["x"], o["dy"]
    T, B, H = x.shape
    inplace = mode == "inplace"
    X = R.Placed(x, out=inplace)
    Y = X if inplace else out_like(x.shape)
    XH = out_like(x.shape) if mode != "noxhat" else None
    IS = out_like((T, H))
    ops.batchnorm_fwd(X.view, Y.view, XH.view if XH else None, IS.view)
    torch.cuda.synchronize()
    r = dict(y=Y.result(), inv_std=IS.result())
    assert_intact(Y, IS)
    assert inplace or X.untouched()
    if XH is not None:
        r["xhat"] = XH.result()
        DY = R.Placed(dy, out=inplace)
        DX = DY if inplace else out_like(x.shape)
        ops.batchnorm_bwd(DY.view, XH.view, IS.view, DX.view)
        torch.cuda.synchronize()
        r["dx"] = DX.result()
        assert_intact(XH, DX)
        assert inplace or DY.untouched()
        assert R.same_bits(XH.result(), r["xhat"]) and R.same_bits(IS.result(), r["inv_std"])      # (the backward reads them only)
    return r


def run_bn_dp(lib, o, shards, inplace):
    """sum -> add -> sum of squares with the global sum -> add -> apply per shard; bwd_sums -> add -> bwd_apply per shard."""
    L = lib.load()
    x, dy = o["x"], o["dy"]
    T, B, H = x.shape
    cuts = np.cumsum((0,) + tuple(shards))
    part = lambda a: [np.ascontiguousarray(a[:, lo:hi, :]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    X = [R.Placed(s, out=inplace) for s in part(x)]
    DY = [R.Placed(s, out=inplace) for s in part(dy)]
    Y = X if inplace else [out_like(s.view.shape) for s in X]
    DX = DY if inplace else [out_like(s.view.shape) for s in X]
    XH = [out_like(s.view.shape) for s in X]
    IS = [out_like((T, H)) for _ in X]

    def reduced(call, width):
        local = [out_like((width, T, H)) for _ in X]
        for i, pl in enumerate(local):
            lib.check(call(i, pl.view), "batchnorm sums")
        torch.cuda.synchronize()
        assert_intact(*local)
        total = R.Placed(local[0].result(), out=False)
        for pl in local[1:]:
            total.view += pl.view
        return total

    bs = lambda i: X[i].view.shape[1]
    gsum = reduced(lambda i, out: L.amdspeech_batchnorm_sum(_stream(), _p(X[i].view), _p(None), B, _p(out), T, bs(i), H), 1)
    gsq = reduced(lambda i, out: L.amdspeech_batchnorm_sum(_stream(), _p(X[i].view), _p(gsum.view), B, _p(out), T, bs(i), H), 1)
    for i in range(len(X)):
        lib.check(L.amdspeech_batchnorm_apply(_stream(), _p(X[i].view), _p(gsum.view), _p(gsq.view), B, R.BN_EPS, _p(Y[i].view), _p(XH[i].view),
                                              _p(IS[i].view), T, bs(i), H), "batchnorm_apply")
    sums = reduced(lambda i, out: L.amdspeech_batchnorm_bwd_sums(_stream(), _p(DY[i].view), _p(XH[i].view), _p(out), T, bs(i), H), 2)
    for i in range(len(X)):
        lib.check(L.amdspeech_batchnorm_bwd_apply(_stream(), _p(DY[i].view), _p(XH[i].view), _p(IS[i].view), _p(sums.view), B, _p(DX[i].view),
                                                  T, bs(i), H), "batchnorm_bwd_apply")
    torch.cuda.synchronize()
    assert_intact(*(Y + XH + IS + DX))
    assert inplace or all(pl.untouched() for pl in X + DY)
    for pl in IS[1:]:
        assert R.same_bits(pl.result(), IS[0].result())      # every shard derives the same inv_std
    cat = lambda pls: np.concatenate([pl.result() for pl in pls], axis=1)
    return dict(y=cat(Y), xhat=cat(XH), inv_std=IS[0].result(), dx=cat(DX))


def bn_judge(got, o, bounds, tag, fails):
    """-> the errors of one run against float64 (dx_own: the float64 backward of the run's own xhat and inv_std)."""
    if not all(np.isfinite(v).all() for v in got.values()):
        fails.append("%s: non-finite results" % tag)
        return {}
    ref = R.bn_f64(o, got.get("xhat"), got.get("inv_std")) if "xhat" in got else R.bn_f64(o)
    errs = R.bn_errors(dict(got, dx_own=got["dx"]) if "dx" in got else got, ref)
    for k, e in errs.items():
        if not e <= bounds[k]:
            fails.append("%s %s: %.3g > %.3g" % (tag, k, e, bounds[k]))
    return errs


@pytest.mark.parametrize("name", [c["name"] for c in R.BN_CASES])
def test_batchnorm_case(ops, lib, name):
    c = R.bn_case_by_name(name)
    o = R.bn_operands(c)
    fails, worst = [], {}
    note = lambda errs: worst.update({k: max(worst.get(k, 0.0), e) for k, e in errs.items()})
    bounds = R.bn_bounds(name)
    runs = {mode: run_bn_fused(ops, o, mode) for mode in R.BN_MODES}
    note(bn_judge(runs["xhat"], o, bounds, "fused", fails))
    for mode in ("noxhat", "inplace"):
        for k, v in runs[mode].items():
            if not R.same_bits(v, runs["xhat"][k]):
                fails.append("fused %s: %s is not the out-of-place result bit for bit" % (mode, k))
    if c["data"] == "constcol":
        t, h = c["T"] // 2, c["H"] // 2
        if runs["xhat"]["y"][t, :, h].any():
            fails.append("the constant column does not normalise to exact zeros")
    line = "fused " + " ".join("%s=%.3g(bound %.3g)" % (k, worst[k], bounds[k]) for k in R.BN_OUTPUTS if k in worst)
    for shards in [s for s in (c["shards"], (c["B"],)) if s]:
        single = len(shards) == 1
        dpb = bounds if single else R.bn_bounds(name, shards)      # one shard owes what the fused kernels owe
        dp = {inplace: run_bn_dp(lib, o, shards, inplace) for inplace in (False, True)}
        errs = bn_judge(dp[False], o, dpb, "shards %s" % (shards,), fails)
        for k, v in dp[True].items():
            if not R.same_bits(v, dp[False][k]):
                fails.append("shards %s in place: %s is not the out-of-place result bit for bit" % (shards, k))
        line += " | shards %s " % (shards,) + " ".join("%s=%.3g(bound %.3g)" % (k, errs[k], dpb[k]) for k in R.BN_OUTPUTS if k in errs)
    print("SMALLK bn %s %s" % (name, line))
    assert not fails, "%s:\n  " % name + "\n  ".join(fails)


def test_batchnorm_refuses_xhat_aliasing_y(ops, lib):
    o = R.bn_operands(R.bn_case_by_name("bn-3x2x5-randn"))
    T, B, H = o["x"].shape
    X, Y, IS = R.Placed(o["x"], out=False), out_like(o["x"].shape), out_like((T, H))
    with pytest.raises(lib.AmdSpeechError, match="xhat must not alias y"):
        ops.batchnorm_fwd(X.view, Y.view, Y.view, IS.view)
    S = R.Placed(np.zeros((T, H), F32), out=False)
    rc = lib.load().amdspeech_batchnorm_apply(_stream(), _p(X.view), _p(S.view), _p(S.view), B, R.BN_EPS, _p(Y.view), _p(Y.view), _p(IS.view), T, B, H)
    with pytest.raises(lib.AmdSpeechError, match="xhat must not alias y"):
        lib.check(rc, "batchnorm_apply")
    torch.cuda.synchronize()
    assert X.untouched() and Y.untouched() and IS.untouched()
    print("SMALLK bn refuses xhat aliasing y")


# ---- reverse_sequences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in R.REV_CASES])
def test_reverse_sequences_case(ops, name):
    c = R.rev_case_by_name(name)
    o = R.rev_operands(c)
    shape = o["x"].shape
    X, XI, YI = (R.Placed(o[k], out=False) for k in ("x", "xi", "yi"))

    def rev(src, lengths, prior=None):
        OUT = R.Placed(np.full(shape, np.nan, F32) if prior is None else prior, out=True)
        ops.reverse_sequences(src.view, lengths.view, out=OUT.view, accumulate=prior is not None)
        torch.cuda.synchronize()
        assert_intact(OUT)
        return OUT

    for lengths in c["lengths"]:
        LEN = R.Placed(lengths, out=False)
        r1 = rev(X, LEN)
        want = R.rev_ref(o["x"], lengths)
        assert np.isfinite(r1.result()).all() and R.same_bits(r1.result(), want), (name, lengths)
        assert R.same_bits(rev(r1, LEN).result(), R.rev_masked(o["x"], lengths)), (name, lengths, "reversing twice")
        acc = rev(XI, LEN, prior=o["prior"]).result()
        assert R.same_bits(acc, o["prior"] + R.rev_ref(o["xi"], lengths)), (name, lengths, "accumulate")
        rx, ry = rev(XI, LEN).result().astype(np.int64), rev(YI, LEN).result().astype(np.int64)
        assert (rx * o["yi"].astype(np.int64)).sum() == (o["xi"].astype(np.int64) * ry).sum(), (name, lengths, "adjoint")
        assert X.untouched() and XI.untouched() and YI.untouched() and LEN.untouched()
    print("SMALLK rev %s %d length vectors exact" % (name, len(c["lengths"])))


@pytest.mark.parametrize("what", R.REV_REFUSED)
def test_reverse_sequences_refuses(ops, lib, what):
    H = 6 if what == "h-not-multiple-of-4" else 8
    X = R.Placed(np.arange(2 * 2 * H, dtype=F32).reshape(2, 2, H), out=True)
    OUT = out_like((2, 2, H))
    LEN = R.Placed(np.array([2, 1], np.int32), out=False)
    with pytest.raises(lib.AmdSpeechError, match="H % 4 == 0" if H == 6 else "in place is not supported"):
        ops.reverse_sequences(X.view, LEN.view, out=OUT.view if H == 6 else X.view)
    torch.cuda.synchronize()
    assert X.untouched() and OUT.untouched()
    print("SMALLK rev refuses %s" % what)


# ---- greedy decode, merge_repeated, edit_distance ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in R.GREEDY_CASES])
def test_greedy_decode_case(ops, name):
    c = R.greedy_case_by_name(name)
    o = R.greedy_operands(c)
    T, B, C_ = o["logits"].shape
    LOG, LEN = R.Placed(o["logits"], out=False), R.Placed(o["lengths"], out=False)
    ids, out_len = ops.ctc_greedy_decode(LOG.view, LEN.view)
    ws = ops.CtcWorkspace(T, B, C_, 4)
    ids_ws, out_len_ws = ops.ctc_greedy_decode(LOG.view, LEN.view, ws=ws)
    torch.cuda.synchronize()
    ids, out_len, ids_ws, out_len_ws = (t.cpu().numpy() for t in (ids, out_len, ids_ws, out_len_ws))
    assert LOG.untouched() and LEN.untouched()
    bad = [b for b in range(B) if out_len[b] != o["out_len"][b] or not np.array_equal(ids[b], o["ids"][b])]
    print("SMALLK greedy %s rows=%d kept=%s" % (name, B, [int(v) for v in out_len]))
    assert not bad, [(b, c["rows"][b]["kind"], int(out_len[b]), int(o["out_len"][b]), np.flatnonzero(ids[b] != o["ids"][b])[:6]) for b in bad]
    assert np.array_equal(ids_ws, ids) and np.array_equal(out_len_ws, out_len)
    dec = om.greedy_decode(o["logits"], o["lengths"])
    assert all(dec[b] == list(ids[b, :out_len[b]]) for b in range(B))


@pytest.mark.parametrize("name", R.MERGE_CASES)
def test_merge_repeated_case(ops, name):
    o = R.merge_operands(name)
    IDS, LENS = R.Placed(o["ids"], out=True), R.Placed(o["lens"], out=True)
    ops.merge_repeated(IDS.view, LENS.view, R.MERGE_PAD)
    torch.cuda.synchronize()
    got, got_len = IDS.result(), LENS.result()
    bad = [r for r in range(len(o["rows"])) if got_len[r] != o["want_lens"][r] or not np.array_equal(got[r], o["want_ids"][r])]
    print("SMALLK merge %s rows=%d T=%d" % (name, len(o["rows"]), o["ids"].shape[1]))
    assert not bad, [(o["rows"][r], int(got_len[r]), int(o["want_lens"][r]), np.flatnonzero(got[r] != o["want_ids"][r])[:6]) for r in bad]
    assert_intact(IDS, LENS)


def test_merge_repeated_refuses_a_row_beyond_the_lds(ops, lib):
    IDS = R.Placed(np.zeros((1, R.MERGE_MAX_T + 1), np.int32), out=True)
    LENS = R.Placed(np.array([5], np.int32), out=True)
    with pytest.raises(lib.AmdSpeechError, match="too long for the LDS row"):
        ops.merge_repeated(IDS.view, LENS.view, R.MERGE_PAD)
    torch.cuda.synchronize()
    assert IDS.untouched() and LENS.untouched()
    print("SMALLK merge refuses T=%d" % (R.MERGE_MAX_T + 1))


def run_distance(ops, pairs, lda, ldb):
    packed = R.ed_pack(pairs, lda, ldb)
    placed = [R.Placed(a, out=False) for a in packed]
    out = ops.edit_distance(*(pl.view for pl in placed))
    torch.cuda.synchronize()
    assert all(pl.untouched() for pl in placed)
    host = ops.edit_distance_host(*packed)
    return out.cpu().numpy(), host


@pytest.mark.parametrize("name", R.ED_CASES)
def test_edit_distance_case(ops, name):
    pairs, want = R.ed_pairs(), R.ed_expected()
    if name == "ed-table":      # two calls of 70 pairs
        groups = [list(range(i, min(i + R.ED_GROUP, len(pairs)))) for i in range(0, len(pairs), R.ED_GROUP)]
        assert [len(g) for g in groups] == [R.ED_GROUP, R.ED_GROUP]
    elif name == "ed-single":   # n_pairs = 1: the longest random pair, and a chain across two chunk boundaries
        pick = lambda kind, n, m: next(i for i, p in enumerate(pairs) if p[0] == kind and len(p[1]) == n and len(p[2]) == m)
        groups = [[pick("random-80", 300, 200)], [pick("drop-first", 128, 129)], [pick("random-2", 0, 0)]]
    else:
        pairs = R.ed_largest()
        want = np.array([R.levenshtein(pairs[0][1], pairs[0][2])], np.int32)
        groups = [[0]]
    lda, ldb = (3, R.ED_MAX_LDB) if name == "ed-largest" else (R.ED_LDA, R.ED_LDB)
    n = 0
    for g in groups:
        got, host = run_distance(ops, [pairs[i] for i in g], lda, ldb)
        bad = [(pairs[i][0], len(pairs[i][1]), len(pairs[i][2]), int(got[j]), int(want[i])) for j, i in enumerate(g) if got[j] != want[i]]
        assert not bad, bad[:10]
        assert np.array_equal(host, want[g])
        n += len(g)
    print("SMALLK ed %s pairs=%d calls=%d lda=%d ldb=%d" % (name, n, len(groups), lda, ldb))


def test_edit_distance_refuses_a_second_sequence_beyond_the_lds(ops, lib):
    a, b = torch.zeros(1, 3, dtype=torch.int32, device="cuda"), torch.zeros(1, R.ED_MAX_LDB + 1, dtype=torch.int32, device="cuda")
    n = torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(lib.AmdSpeechError, match="second sequence too long for LDS"):
        ops.edit_distance(a, n, b, n)
    torch.cuda.synchronize()
    print("SMALLK ed refuses ldb=%d" % (R.ED_MAX_LDB + 1))


def test_decode_merge_distance_chain(ops):
    """greedy -> merge_repeated (pad = C) -> edit_distance against the truths, as AcousticModel._error_rate_launch does."""
    c = R.CHAIN_CASE
    o = R.chain_operands()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ids, out_len = ops.ctc_greedy_decode(dev(o["logits"]), dev(o["lengths"]))
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), o["ids"]) and np.array_equal(out_len.cpu().numpy(), o["out_len"])
    ops.merge_repeated(ids, out_len, c["C"])
    dist = ops.edit_distance(ids, out_len, dev(o["truth"]), dev(o["tlen"]))
    torch.cuda.synchronize()
    merged, want = R.chain_ref(o, c["C"])
    ids, out_len = ids.cpu().numpy(), out_len.cpu().numpy()
    for b, row in enumerate(merged):
        assert out_len[b] == len(row) and list(ids[b, :len(row)]) == row and np.all(ids[b, len(row):] == c["C"]), b
    print("SMALLK chain %s distances=%s" % (c["name"], [int(v) for v in dist.cpu().numpy()]))
    assert np.array_equal(dist.cpu().numpy(), want)


# ---- axpy / fill ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.VEC_SIZES)
def test_axpy_and_fill(lib, n):
    L = lib.load()
    o = R.vec_operands(n)
    X, Y, Z = R.Placed(o["x"], out=False), R.Placed(o["y"], out=True), out_like(n)
    lib.check(L.amdspeech_axpy(_stream(), R.AXPY_A, _p(X.view), _p(Y.view), n), "axpy")
    lib.check(L.amdspeech_fill(_stream(), _p(Z.view), R.FILL_VALUE, n), "fill")
    torch.cuda.synchronize()
    print("SMALLK vec n=%d axpy and fill exact" % n)
    assert R.same_bits(Y.result(), o["axpy"]), np.flatnonzero(Y.result() != o["axpy"])[:8]
    assert R.same_bits(Z.result(), np.full(n, R.FILL_VALUE, F32))
    assert X.untouched()
    assert_intact(Y, Z)
