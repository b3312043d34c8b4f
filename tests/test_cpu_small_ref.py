"""CPU checks of tests/small_ref.py: its references against the oracle's functions and against brute force on tiny inputs, the
conditions under which its `ints` results are exact, the restatements' errors against float64 (the GPU bounds are 4 x these, never
stored), the one-pass variance rewrite the offset data must catch, the planned decode paths under the oracle, and the coverage
predicates: every edge the tables were written for is in them.  The host edit distance runs the whole pair table here."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_ref as R  # noqa: E402
from oracle import model as om  # noqa: E402


def test_the_tables_contain_every_edge():
    missing = [k for k, pred in R.COVERAGE.items() if not pred()]
    assert not missing, missing
    for table in (R.ADAM_CASES, R.BN_CASES, R.REV_CASES, R.GREEDY_CASES):
        assert len({c["name"] for c in table}) == len(table)


def test_the_caps_and_limits_are_those_of_the_sources():
    optim = open(os.path.join(ROOT, "rnn-speech_amd", "csrc", "optim.hip")).read()
    assert "SUMSQ_BLOCKS = %d;" % R.SUMSQ_CAP in optim and "if (ablocks > %d) ablocks = %d;" % (R.ADAM_CAP, R.ADAM_CAP) in optim
    assert optim.count("if (blocks > %d) blocks = %d;" % (R.VEC_CAP, R.VEC_CAP)) == 2      # axpy and fill
    ctc = open(os.path.join(ROOT, "rnn-speech_amd", "csrc", "ctc.hip")).read()
    assert "(size_t)T * 4 <= 60 * 1024" in ctc and "(size_t)(ldb + 1) * 4 <= 60 * 1024" in ctc


@pytest.mark.parametrize("name", [c["name"] for c in R.ADAM_CASES if c["kind"] == "ints"])
def test_adam_ints_are_exact_in_any_order(name):
    c = R.adam_case_by_name(name)
    g = R.adam_operands(c)["g"]
    assert set(np.unique(g)) <= {-1.0, 0.0, 1.0} and c["clip"] == R.BIG_CLIP
    S = int((g.astype(np.int64) ** 2).sum())
    assert 0 < S < 2 ** 18
    assert np.all(g[R.adam_planted(c["n"])] != 0)
    if c["n"] > 8:
        assert (g == 0).any()
    # one term more or less moves the norm by >= 16 ulp
    for other in (S - 1, S + 1):
        assert R.ulps(np.float32(np.sqrt(S)), np.float32(np.sqrt(max(other, 0)))) >= 16 or S < 4
    # ... and the restatement in the kernels' order returns the exact sum
    assert R.ulps(R.sumsq_f32(g), np.float32(np.sqrt(S))) <= 1
    geo = R.adam_geometry(c["n"])
    for key in ("sumsq", "adam"):      # both sides of every stride boundary
        for k in range(1, geo[key]["trips"]):
            e = 4 * k * geo[key]["stride4"]
            assert g[e - 1] != 0 and g[e] != 0


def test_adam_geometry_is_the_launch_arithmetic():
    g = R.adam_geometry
    assert g(794957)["sumsq"]["blocks"] == 777      # the largest n of test_clip_adam: neither loop strides twice
    assert g(1048575)["sumsq"] == dict(blocks=1024, capped=False, stride4=262144, trips=1)
    assert g(1048579)["sumsq"]["capped"] and g(1048579)["sumsq"]["trips"] == 1      # capped, yet every float4 still in the first trip
    assert g(1048583)["sumsq"]["trips"] == 2 and g(1048583)["tail"] == 3
    assert g(2097159)["adam"] == dict(blocks=2048, capped=True, stride4=524288, trips=2) and g(2097159)["tail"] == 3
    assert g(4200003)["adam"]["trips"] == 3 and g(4200003)["tail"] == 3


def test_adam_atclip_sums_to_one_exactly():
    c = R.adam_case_by_name("atclip-1048583")
    g = R.adam_operands(c)["g"]
    assert int((g != 0).sum()) == 65536 and set(np.unique(np.abs(g[g != 0]))) == {2.0 ** -8}
    assert R.sumsq_f32(g) == np.float32(1.0) == np.float32(c["clip"])
    assert np.all(g[R.adam_planted(c["n"])] != 0)


@pytest.mark.parametrize("name", [c["name"] for c in R.ADAM_CASES if c["kind"] in ("normal", "tiny", "zero")])
def test_adam_restatement_against_float64(name):
    c = R.adam_case_by_name(name)
    o = R.adam_operands(c)
    gn = float(np.sqrt((o["g"].astype(np.float64) ** 2).sum()))
    if "unclipped" in name:
        assert gn < c["clip"]
    if "-clipped" in name:
        assert gn > c["clip"]
    if c["kind"] == "tiny":      # eps dominates the denominator after every step
        assert all(np.sqrt(s["v"]).max() < 1e-3 * R.EPS for s in R.adam_f64(o, c["clip"], c["steps"]))
    measured, bounds = R.adam_measured(name), R.adam_bounds(name)
    print("SMALLREF adam %s" % name, " ".join("%s=%.3g(bound %.3g)" % (k, measured[k], bounds[k]) for k in sorted(measured)))
    for k in R.ADAM_CAPS:      # the new bounds are never looser than test_clip_adam's, and the restatement itself meets them
        assert R.HALF_ULP <= measured[k] < R.ADAM_CAPS[k] and bounds[k] <= R.ADAM_CAPS[k]


def test_adam_restatement_is_the_oracle_on_exact_data():
    """m = (1 - b1) g and v = (1 - b2) g^2 of the ints kind: the f32 products the GPU test asks for, and the oracle within an ulp."""
    c = R.adam_case_by_name("ints-1023")
    o = R.adam_operands(c)
    f32 = R.adam_f32(o, c["clip"], 1)[0]
    one = np.float32(1)
    assert R.same_bits(f32["m"], (one - np.float32(R.B1)) * o["g"]) and R.same_bits(f32["v"], (one - np.float32(R.B2)) * o["g"] * o["g"])
    assert R.same_bits(f32["p"][o["g"] == 0], o["p"][o["g"] == 0])
    ref = R.adam_f64(o, c["clip"], 1)[0]
    assert R.rel_err(f32["m"], ref["m"]) < 1e-6 and np.abs(f32["p"] - ref["p"]).max() < 2e-6


@pytest.mark.parametrize("name", [c["name"] for c in R.BN_CASES])
def test_bn_restatement_against_float64(name):
    c = R.bn_case_by_name(name)
    o = R.bn_operands(c)
    ref = R.bn_f64(o)
    if c["B"] == 1:
        assert not ref["y"].any() and np.allclose(ref["inv_std"], 1.0 / np.sqrt(R.BN_EPS))
    if c["data"] == "constcol":
        t, h = c["T"] // 2, c["H"] // 2
        f32 = R.bn_f32(o)
        assert not f32["y"][t, :, h].any() and f32["inv_std"][t, h] == np.float32(1) / np.sqrt(np.float32(R.BN_EPS))
    measured = R.bn_measured(name)
    print("SMALLREF bn %s" % name, " ".join("%s=%.3g" % (k, measured[k]) for k in R.BN_OUTPUTS))
    assert set(measured) == set(R.BN_OUTPUTS) and all(R.HALF_ULP <= e < 1e-4 for e in measured.values())
    # brute force of the float64 reference at one column
    t, h = c["T"] - 1, c["H"] - 1
    col = o["x"][t, :, h].astype(np.float64)
    mean = sum(col) / len(col)
    var = sum((v - mean) ** 2 for v in col) / len(col)
    assert abs(ref["inv_std"][t, h] - 1.0 / np.sqrt(var + 1e-3)) < 1e-12 * ref["inv_std"][t, h]
    assert np.allclose(ref["y"][t, :, h], (col - mean) / np.sqrt(var + 1e-3), rtol=1e-12, atol=1e-12)
    if c["shards"]:
        assert sum(c["shards"]) == c["B"] and len(set(c["shards"])) == len(c["shards"])
        dp = R.bn_measured(name, c["shards"])
        print("SMALLREF bn %s shards %s" % (name, c["shards"]), " ".join("%s=%.3g" % (k, dp[k]) for k in R.BN_OUTPUTS))
        assert all(e < 1e-4 for e in dp.values())
    # one shard is the fused formula up to mean = sum * (1 / n) for sum / n
    one = R.bn_dp_f32(o, (c["B"],))
    assert R.rel_err(one["y"], R.bn_f32(o)["y"]) < 1e-4


@pytest.mark.parametrize("name", [c["name"] for c in R.BN_CASES if c["data"] == "offset" and c["B"] > 1])
def test_bn_offset_data_catches_the_one_pass_variance(name):
    """var = E[x^2] - mean^2 in f32 at offset 100 is outside the bound of inv_std that the two-pass restatement sets."""
    o = R.bn_operands(R.bn_case_by_name(name))
    ref = R.bn_f64(o)["inv_std"]
    two, one, bound = R.rel_err(R.bn_f32(o)["inv_std"], ref), R.rel_err(R.bn_one_pass_f32(o), ref), R.bn_bounds(name)["inv_std"]
    print("SMALLREF bn %s inv_std two-pass=%.3g one-pass=%.3g bound=%.3g" % (name, two, one, bound))
    assert two < bound < one and one > 100 * bound


@pytest.mark.parametrize("name", [c["name"] for c in R.REV_CASES])
def test_reverse_reference(name):
    c = R.rev_case_by_name(name)
    o = R.rev_operands(c)
    T, B = c["T"], c["B"]
    for lengths in c["lengths"]:
        ref = R.rev_ref(o["x"], lengths)
        assert R.same_bits(ref, om.reverse_sequences(o["x"], lengths))      # (the oracle clamps too)
        for b in range(B):      # brute force
            n = min(max(int(lengths[b]), 0), T)
            for t in range(T):
                want = o["x"][n - 1 - t, b] if t < n else np.zeros(c["H"], np.float32)
                assert R.same_bits(ref[t, b], want)
        assert R.same_bits(R.rev_ref(ref, lengths), R.rev_masked(o["x"], lengths))
        lhs = (R.rev_ref(o["xi"], lengths).astype(np.int64) * o["yi"].astype(np.int64)).sum()
        assert lhs == (o["xi"].astype(np.int64) * R.rev_ref(o["yi"], lengths).astype(np.int64)).sum()
    assert np.abs(o["xi"]).max() * np.abs(o["yi"]).max() * o["xi"].size < 2 ** 24 * 64      # (summed in int64 on the host anyway)
    assert np.abs(o["prior"]).max() + np.abs(o["xi"]).max() < 2 ** 24


@pytest.mark.parametrize("name", [c["name"] for c in R.GREEDY_CASES] + [R.CHAIN_CASE["name"]])
def test_planned_paths_decode_to_the_table_under_the_oracle(name):
    c = R.greedy_case_by_name(name)
    o = R.greedy_operands(c)
    T, C = c["T"], c["C"]
    assert np.isfinite(o["logits"][np.isfinite(o["logits"])]).all() and not np.isnan(o["logits"]).any()
    best = o["logits"].argmax(axis=2)
    dec = om.greedy_decode(o["logits"], o["lengths"])
    for b, r in enumerate(c["rows"]):
        n = max(0, min(r["length"], T))
        assert np.array_equal(best[:n, b], r["path"][:n]), (name, b)
        for t, tied in r["ties"].items():
            top = np.flatnonzero(o["logits"][t, b] == o["logits"][t, b].max())
            assert tuple(top) == tuple(sorted(tied)) and best[t, b] == min(tied)
        if n < T:      # past the length the logits say something else, loudly
            assert np.all(best[n:, b] != C - 1) or r["ninf"]
        assert dec[b] == list(o["ids"][b, :o["out_len"][b]]) and np.all(o["ids"][b, o["out_len"][b]:] == C)
        if r["kind"] == "same":
            assert o["out_len"][b] == 1
        if r["kind"] in ("lbl", "diff"):
            assert o["out_len"][b] == 2
        if r["kind"] == "blank":
            assert o["out_len"][b] == 0
        if r["kind"] == "alternating" and C > 2:
            assert o["out_len"][b] == n
        if r["kind"] == "ninf":
            assert dec[b] == [0]


def test_merge_reference():
    for name in R.MERGE_CASES:
        o = R.merge_operands(name)
        for r, (content, n) in enumerate(o["rows"]):
            seq = list(o["ids"][r, :n])
            want = [k for i, k in enumerate(seq) if i == 0 or k != seq[i - 1]]      # brute force
            kept = o["want_lens"][r]
            assert list(o["want_ids"][r, :kept]) == want and np.all(o["want_ids"][r, kept:n] == R.MERGE_PAD)
            assert np.array_equal(o["want_ids"][r, n:], o["ids"][r, n:]) and np.all(o["ids"][r, n:] >= 1000)
            if content == "equal":
                assert kept == min(n, 1)
            if content in ("distinct", "alternating"):
                assert kept == n
            if content == "seamrun":
                for k in R.SEAMS:
                    if n > k:
                        assert seq[k - 1] == seq[k]
    o = R.merge_operands("merge-largest")
    assert o["ids"].shape == (1, R.MERGE_MAX_T) and 1 < o["want_lens"][0] < R.MERGE_MAX_T


def test_levenshtein_against_the_oracle_and_the_host_library():
    pairs, want = R.ed_pairs(), R.ed_expected()
    assert len(pairs) == 2 * R.ED_GROUP
    small = [i for i, p in enumerate(pairs) if len(p[1]) * len(p[2]) <= 64 * 129]
    assert len(small) > 80
    for i in small:
        assert want[i] == om.edit_distance(pairs[i][1], pairs[i][2]), pairs[i][0]
    for i, (kind, a, b, known) in enumerate(pairs):
        if known is not None:
            assert want[i] == known
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import ops
    got = ops.edit_distance_host(*R.ed_pack(pairs, R.ED_LDA, R.ED_LDB))
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    big = R.ed_largest()
    d = R.levenshtein(big[0][1], big[0][2])
    assert R.ED_MAX_LDB - 3 <= d <= R.ED_MAX_LDB - 2
    assert ops.edit_distance_host(*R.ed_pack(big, 3, R.ED_MAX_LDB))[0] == d


def test_chain_reference():
    o = R.chain_operands()
    merged, dist = R.chain_ref(o, R.CHAIN_CASE["C"])
    assert any(len(m) < n for m, n in zip(merged, o["out_len"]))      # the merge has work to do
    assert len(set(dist)) > 2 and (o["tlen"] > 0).all()


def test_axpy_ints_are_exact():
    for n in R.VEC_SIZES:
        o = R.vec_operands(n)
        assert np.abs(o["axpy"]).max() < 2 ** 24 and R.same_bits(o["axpy"], o["y"] + np.float32(R.AXPY_A) * o["x"])
    assert np.float32(R.FILL_VALUE).view(np.uint32) & 0xFFF      # low mantissa bits set
