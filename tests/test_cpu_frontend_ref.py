"""CPU checks of tests/frontend_ref.py: every case's expected plan equals amdspeech_frontend_plan (the table cannot drift from the
dispatch), the table reaches every kernel variant and every edge it was written for, the float64 references are what they claim to
be, MEASURED equals the float32 emulation, and every planted fault breaks the bound of its case.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref as R  # noqa: E402
from oracle import frontend as ofe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from rnn_speech_amd import ops as o
    return o


def _switch_is_default():
    return os.environ.get("AMDSPEECH_FRONTEND_MFMA", "1") != "0"


def _plan_in_child(cases):
    """The plans of `cases` under AMDSPEECH_FRONTEND_MFMA=0 (the library reads the switch once per process): a child process, no GPU."""
    import json
    import subprocess
    code = ("import json, sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import frontend_ref as R; from rnn_speech_amd import ops; "
            "print(json.dumps([ops.frontend_plan(**R.plan_args(R.by_name(n))) for n in %r]))" % (ROOT, os.path.join(ROOT, "tests"), cases))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **R.FALLBACK_ENV), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_struct_layout_equals_the_header(ops):
    from rnn_speech_amd import lib
    header = open(os.path.join(ROOT, "include", "amdspeech.h")).read()
    decl = header.split("typedef struct amdspeech_frontend_plan_info {")[1].split("}")[0]
    assert [n.strip() for n in decl.replace("int", "").replace(";", "").split(",")] == [n for n, _ in lib.FrontendPlanInfo._fields_]
    assert ctypes.sizeof(lib.FrontendPlanInfo) == 4 * len(lib.FrontendPlanInfo._fields_)
    assert set(R.expected_plan("mfcc", 16000, 20, 1, 16000, 10)) == {n for n, _ in lib.FrontendPlanInfo._fields_}


def test_every_expected_plan_equals_the_plan_query(ops):
    assert _switch_is_default()
    for c in R.CASES:
        got = ops.frontend_plan(**R.plan_args(c))
        diff = {k: (v, got[k]) for k, v in c["plan"]["default"].items() if got[k] != v}
        assert not diff, (c["name"], "default", diff, got)
        assert got == R.expected_plan(c["mode"], c["sr"], c["n_mfcc"], c["B"], c["n_max"], c["t_max"]), c["name"]
    names = [c["name"] for c in R.CASES if "fallback" in c["plan"]]
    for name, got in zip(names, _plan_in_child(names)):
        c = R.by_name(name)
        diff = {k: (v, got[k]) for k, v in c["plan"]["fallback"].items() if got[k] != v}
        assert not diff, (name, "fallback", diff, got)
        assert got == R.expected_plan(c["mode"], c["sr"], c["n_mfcc"], c["B"], c["n_max"], c["t_max"], mfma=False), name


def test_refusals_match_the_call(ops):
    from rnn_speech_amd import lib
    h = lib.load()
    info = lib.FrontendPlanInfo()
    ok = dict(mode=0, sr=16000, n_mfcc=20, B=2, n_max=16000, t_max=100)
    call = lambda **kw: h.amdspeech_frontend_plan(*[{**ok, **kw}[k] for k in ("mode", "sr", "n_mfcc", "B", "n_max", "t_max")], ctypes.byref(info))
    assert call() == 0
    for bad, msg in ((dict(n_mfcc=0), b"n_mfcc out of range"), (dict(n_mfcc=129), b"n_mfcc out of range"), (dict(B=0), b"bad shape"),
                     (dict(n_max=0), b"bad shape"), (dict(t_max=0), b"bad shape"), (dict(sr=999), b"bad shape"), (dict(mode=2), b"mode"),
                     (dict(sr=82000), b"max 2048")):
        assert call(**bad) != 0, bad
        assert msg in h.amdspeech_last_error(), (bad, h.amdspeech_last_error())
        assert R.expected_plan("mfcc", *[{**ok, **bad}[k] for k in ("sr", "n_mfcc", "B", "n_max", "t_max")]) is None or "mode" in bad
    assert call(mode=1, n_mfcc=0) == 0 and call(mode=1, n_mfcc=0, sr=96000) == 0      # (fbank: no n_mfcc, 512 points at every rate)
    assert call(sr=81900) == 0 and info.n_dft == 2048 and info.frames_kernel == 0      # (the largest DFT the call takes)
    assert h.amdspeech_frontend_plan(0, 16000, 20, 2, 16000, 100, None) != 0
    with pytest.raises(lib.AmdSpeechError, match="n_mfcc out of range"):
        ops.frontend_plan("mfcc", 16000, 200, 1, 16000, 10)
    # the call itself refuses through the same function: with null buffers it stops at its pointer check, before any device work
    assert h.amdspeech_frontend_mfcc(None, None, None, 1, 16000, 16000, 20, 10, None, None, None) != 0


def test_the_table_reaches_every_variant_and_every_edge():
    cases = {c["name"]: c for c in R.CASES}
    assert len(cases) == len(R.CASES)
    plans = {m: [c["plan"][m] for c in R.CASES if m in c["plan"]] for m in ("default", "fallback")}
    assert {(p["frames_kernel"], p["maxq"]) for p in plans["default"]} == {(0, 0), (1, 4), (1, 5), (1, 9)}
    assert {(p["frames_kernel"], p["maxq"]) for p in plans["fallback"]} == {(0, 0)}
    assert {p["dct_kernel"] for p in plans["default"]} == {-1, 1} and {p["dct_kernel"] for p in plans["fallback"]} == {-1, 0}
    assert {p["meta_by_copy"] for p in plans["default"]} == {0, 1}
    full = [R.expected_plan(c["mode"], c["sr"], c["n_mfcc"], c["B"], c["n_max"], c["t_max"]) for c in R.CASES]
    assert any(p["frames_kernel"] == 1 and p["n_items"] > p["workgroups"] for p in full) and any(p["n_items"] == p["workgroups"] for p in full)
    for mode in ("mfcc", "fbank"):          # the queue longer than the grid in both modes
        assert any(c["mode"] == mode and p["n_items"] > p["workgroups"] == 512 for c, p in zip(R.CASES, full))
    assert {c["row"] for c in R.CASES} == set(R.ROWS)
    # every row of the table, by what it was written for
    want = {"mfcc8k_edges", "mfcc16k_n128", "mfcc16k_n13", "mfcc16k_n17", "mfcc16k_n1", "mfcc16k_n16", "mfcc16k_n65", "mfcc22k", "mfcc25k",
            "mfcc25k6", "mfcc32k", "mfcc35k", "mfcc36k", "mfcc44k", "fbank96k", "fbank8k", "fbank16k", "fbank22k", "fbank44k", "mfcc8k_queue",
            "fbank8k_queue", "mfcc8k_b257", "mfcc16k_burst", "mfcc16k_quiet", "mfcc16k_silence", "fbank16k_silence"}
    assert set(cases) == want, set(cases) ^ want
    nf = lambda c: [R.num_frames(c["mode"], c["sr"], n) for n in c["rows"]]
    c = cases["mfcc8k_edges"]
    assert nf(c) == [2, 31, 32, 33, 65, 0] and c["rows"][0] == R.geometry("mfcc", 8000)["n_dft"] // 2 + 1 and c["t_max"] == 40
    assert c["plan"]["default"]["bin_tiles"] == 7 and 7 % 4 == 3          # (waves 0 .. 2 own two tiles, wave 3 one)
    assert nf(cases["mfcc16k_n128"]) == [33, 64]
    for n in ("mfcc16k_n128", "mfcc16k_n13", "mfcc16k_n17", "mfcc16k_n1", "mfcc16k_n16", "mfcc16k_n65"):
        assert (cases[n]["t_max"] * cases[n]["B"]) % 32 != 0 and "fallback" in cases[n]["plan"]
    for n in ("mfcc22k", "mfcc25k", "mfcc25k6", "mfcc32k", "mfcc35k", "mfcc36k"):
        assert nf(cases[n]) == [33, 65], n
    assert R.geometry("mfcc", 22050)["n_dft"] % 2 == 1 and R.geometry("mfcc", 25000)["n_dft"] % 2 == 1
    assert (cases["mfcc25k"]["plan"]["default"]["bin_tiles"], cases["mfcc25k6"]["plan"]["default"]["bin_tiles"]) == (20, 21)
    assert cases["mfcc35k"]["plan"]["default"]["lds_bytes"] == 162612 <= R.LDS_MAX
    for n in ("fbank8k", "fbank16k", "fbank22k", "fbank44k"):
        assert nf(cases[n]) == [9, 32, 33, 65, 0] and min(nf(cases[n])[:4]) < cases[n]["t_max"] < max(nf(cases[n])), n
    assert R.geometry("fbank", 22050)["win"] == 551 and R.geometry("fbank", 96000)["win"] == 2400
    assert cases["mfcc8k_b257"]["B"] == 257 and all(800 <= n <= 1600 for n in cases["mfcc8k_b257"]["rows"])
    assert nf(cases["mfcc16k_burst"]) == [74] and 74 - 10 == 2 * R.FR
    assert cases["mfcc16k_burst"]["kinds"] == ["burst"] and cases["mfcc16k_quiet"]["kinds"] == ["quiet"]
    assert cases["mfcc16k_silence"]["kinds"] == ["silence"] == cases["fbank16k_silence"]["kinds"]
    assert {cases[n]["n_mfcc"] for n in cases if cases[n]["row"] in ("dct_widths", "maxq4_13tiles")} == {1, 13, 16, 17, 65, 128}
    assert set(R.FAULT_CASE) == set(R.FAULTS) and set(R.FAULT_CASE.values()) <= set(cases) and set(R.MEASURED) == set(cases)


def test_dispatch_sweep_agrees_on_both_sides_of_every_cut(ops):
    """8 .. 96 kHz in steps of 50 Hz and every rate beside a cut: the plan query against the arithmetic restated in frontend_ref.py
    and against the cuts themselves, stated here a third time as plain numbers."""
    assert _switch_is_default()
    from rnn_speech_amd import lib

    def q(mode, sr):
        try:
            return ops.frontend_plan(mode, sr, 20, 3, 2 * sr, 50)
        except lib.AmdSpeechError:
            return None

    seen = {"mfcc": set(), "fbank": set()}
    for mode in ("mfcc", "fbank"):
        for sr in range(8000, 96001, 50):
            got = q(mode, sr)
            assert got == R.expected_plan(mode, sr, 20, 3, 2 * sr, 50), (mode, sr, got)
            if got:
                seen[mode].add((got["frames_kernel"], got["maxq"]))
    assert seen["mfcc"] == {(1, 4), (1, 5), (1, 9), (0, 0)} and seen["fbank"] == {(1, 5), (0, 0)}

    def first_rate(mode, pred):          # the first integer rate from 8 kHz at which pred(plan) holds
        sr = next(s for s in range(8000, 96001, 50) if pred(q(mode, s))) - 50
        return next(s for s in range(sr, sr + 51) if pred(q(mode, s)))

    # 16 -> 17 tiles: n_bins 257 = n_dft 512 = round(0.025 sr), from sr = 20,460.  20 -> 21 tiles: n_dft 640, from sr = 25,580 (25.6 kHz
    # is the first rate of the issue's list on <9>).  The LDS cut of mfcc: 4 (64 (kp + 4) + 31 hop + n_dft) <= 163,584.
    cut = first_rate("mfcc", lambda p: p["maxq"] != 4)
    assert (q("mfcc", cut - 1)["bin_tiles"], q("mfcc", cut - 1)["maxq"], q("mfcc", cut)["bin_tiles"], q("mfcc", cut)["maxq"]) == (16, 4, 17, 5)
    assert q("mfcc", cut)["n_dft"] == 512 and cut == 20460
    cut = first_rate("mfcc", lambda p: p["maxq"] not in (4, 5))
    assert (q("mfcc", cut - 1)["bin_tiles"], q("mfcc", cut - 1)["maxq"], q("mfcc", cut)["bin_tiles"], q("mfcc", cut)["maxq"]) == (20, 5, 21, 9)
    assert q("mfcc", cut)["n_dft"] == 640 and cut == 25580
    cut = first_rate("mfcc", lambda p: p["frames_kernel"] == 0)
    below, above = q("mfcc", cut - 1), q("mfcc", cut)
    assert (below["frames_kernel"], below["maxq"], above["frames_kernel"], above["maxq"]) == (1, 9, 0, 0) and 35000 < cut <= 36000 and cut == 35750
    assert 4 * (64 * (below["kp"] + 4) + 31 * below["hop"] + below["n_dft"]) == below["lds_bytes"] <= R.LDS_MAX
    assert 4 * (64 * (above["kp"] + 4) + 31 * above["hop"] + above["n_dft"]) > R.LDS_MAX
    assert above["lds_bytes"] == 4 * (8 * above["n_dft"] + 2 * above["n_dft"] + 8 * above["n_bins"])
    assert q("mfcc", 35000)["frames_kernel"] == 1 and q("mfcc", 36000)["frames_kernel"] == 0 and q("mfcc", 32001)["frames_kernel"] == 1
    # fbank: 512 points at every rate, so <5> until the PCM span of 32 frames (31 hops + 512) no longer fits beside e / o
    cut = first_rate("fbank", lambda p: p["frames_kernel"] == 0)
    below, above = q("fbank", cut - 1), q("fbank", cut)
    assert (below["maxq"], below["bin_tiles"], below["kp"], above["maxq"]) == (5, 17, 288, 0)
    assert below["lds_bytes"] == 4 * (64 * 292 + 31 * below["hop"] + 512) <= R.LDS_MAX < 4 * (64 * 292 + 31 * above["hop"] + 512)
    assert (below["hop"], above["hop"]) == (699, 700) and cut == 69950
    assert q("fbank", 44100)["frames_kernel"] == 1 and q("fbank", 48000)["maxq"] == 5 and q("fbank", 96000)["frames_kernel"] == 0
    # mfcc is refused from the first rate whose window exceeds 2048 points
    assert q("mfcc", 81900)["n_dft"] == 2048 and q("mfcc", 82000) is None and q("fbank", 96000) is not None


def test_references_are_what_they_claim():
    D = R.D128
    assert np.abs(D @ D.T - np.eye(128)).max() < 1.6e-14
    for name in ("mfcc8k_edges", "mfcc22k", "mfcc16k_burst", "mfcc16k_quiet", "mfcc16k_silence"):
        c = R.by_name(name)
        for sig, ref in zip(R.signals(name), R.reference(name)):
            if len(sig) == 0:
                continue
            assert np.abs(R.invert_dct128(ref["feat"]) - ref["stage"]).max() < 1e-10
            assert np.abs(ref["feat"] - ofe.mfcc(sig, c["sr"], n_mfcc=128)).max() < 1e-10
            assert np.abs(ref["stage"] @ ofe.dct2_ortho_matrix(20, 128).T - ofe.mfcc(sig, c["sr"], n_mfcc=20)).max() < 1e-10
            assert len(ref["feat"]) == R.num_frames("mfcc", c["sr"], len(sig))
    for name in ("fbank8k", "fbank22k", "fbank96k"):
        c = R.by_name(name)
        for sig, ref in zip(R.signals(name), R.reference(name)):
            if len(sig) == 0:
                continue
            assert np.array_equal(ref["feat"], ofe.fbank(sig, c["sr"])) and np.array_equal(ref["feat"][:, :40], ref["stage"])
            assert np.array_equal(ref["feat"][:, 40:], ref["delta"]) and len(ref["feat"]) == R.num_frames("fbank", c["sr"], len(sig))


def test_signals_are_what_the_cases_name():
    for c in R.CASES:
        for kind, sig, ref in zip(c["kinds"], R.signals(c["name"]), R.reference(c["name"])):
            if kind != "synth" or len(sig) == 0 or c["mode"] != "mfcc":
                continue
            # the noise floor: 99 % of the log-mels within 55 dB of the peak, the clamp far away.  (Single values dip lower: a
            # one-bin filter over noise is chi-square distributed; and the filters that hold no bin at all -- at 8 kHz 128 filters
            # meet 101 bins -- sit at the clamp exactly, in every arithmetic.)
            live = ofe.slaney_mel_filterbank(c["sr"], R.geometry("mfcc", c["sr"])["n_dft"], 128).any(axis=1)
            st = ref["stage"][:, live]
            assert st.max() - np.percentile(st, 1) < 55.0, (c["name"], st.max() - np.percentile(st, 1))
            assert (ref["stage"][:, ~live] == ref["stage"].max() - 80.0).all()
    burst = R.reference("mfcc16k_burst")[0]["stage"]
    assert burst[-10:].max() == burst.max() and burst[:64].max() < burst.max() - 60.0
    assert (burst[:64] == burst.max() - 80.0).mean() > 0.2          # the clamp binds in the quiet part, against the LAST tile's maximum
    quiet = R.reference("mfcc16k_quiet")[0]["stage"]
    assert quiet.max() < -80.0 and (quiet > -100.0).mean() > 0.5          # a negative maximum; most values above the 1e-10 floor
    sil = R.reference("mfcc16k_silence")[0]
    assert np.abs(sil["feat"][:, 0] + 100.0 * np.sqrt(128.0)).max() < 1e-9 and np.abs(sil["feat"][:, 1:]).max() < 1e-9
    assert np.abs(R.reference("fbank16k_silence")[0]["feat"]).max() <= 1.1e-8


def test_measured_table_equals_the_emulation():
    for c in R.CASES:
        m, held = R.measure(c["name"]), R.MEASURED[c["name"]]
        for k in ("feature", "stage", "delta"):
            assert abs(m[k] - held[k]) <= 1e-3 * held[k] + 1e-300, (c["name"], k, m[k], held[k])       # (the table holds four digits)
        assert m["feature"] < R.FEATURE_TOL, (c["name"], m)          # float32 itself stays inside the feature tolerance
        if c["stage"]:
            assert 0.0 < R.STAGE_FACTOR * held["stage"] < 2e-2, (c["name"], held)


def test_every_planted_fault_breaks_the_bound_of_its_case():
    """Each fault, planted in the emulation, misses the bound of the case written for it by a factor of 2 or more; and which of them
    the feature-level check (2e-3 on the final features, mfcc at n_mfcc = 20) would have let through."""
    missed = []
    for fault in R.FAULTS:
        c = R.by_name(R.FAULT_CASE[fault])
        errs, bnds = R.case_errors(c, R.emulate(c["name"], fault)), R.bounds(c)
        worst = max(e / b for e, b in zip(errs, bnds) if e is not None and b is not None)
        print("FRONTFAULT %s %s feature=%.3g stage=%s delta=%s worst_over_bound=%.3g" % (fault, c["name"], errs[0], errs[1], errs[2], worst))
        assert worst >= 2.0, (fault, c["name"], errs, bnds)
        if fault == "savgol_edge":          # (the statics are untouched: only the separate delta check sees it)
            assert errs[1] < bnds[1] and errs[2] >= 2.0 * bnds[2]
        if c["mode"] == "mfcc":
            at20 = 0.0
            for sig, got in zip(R.signals(c["name"]), R.emulate(c["name"], fault, n_mfcc=20)):
                if len(sig):
                    at20 = max(at20, float(np.abs(got - ofe.mfcc(sig, c["sr"], n_mfcc=20)).max()))
        else:
            at20 = errs[0]
        if at20 < R.FEATURE_TOL:
            missed.append(fault)
    assert tuple(missed) == R.MISSED_AT_FEATURE_LEVEL, missed
    # without a fault the emulation passes every bound of every fault case
    for name in set(R.FAULT_CASE.values()):
        c = R.by_name(name)
        assert all(e < b for e, b in zip(R.case_errors(c, R.emulate(name)), R.bounds(c)) if e is not None and b is not None), name
