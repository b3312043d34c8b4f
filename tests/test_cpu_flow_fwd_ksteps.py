"""Host side of the extended half roles of the forward dataflow kernel (csrc/lstm_flow_fwd.h: ME), without a GPU: the plan query
exists, the plan struct keeps its 16 ints, the workspace size does not depend on AMDSPEECH_FLOW_FWD_WORKERS (the half role takes more
K into the SAME tile: nothing new is reserved), and a numpy restatement of the three-way split of x . W_ih -- what the recurrence wave
keeps, the full role's tile, the extended half role's tile -- adds up to the whole product exactly, for every ME, while an
off-by-one k-step range does not."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rnn_speech_amd import lib as _l

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototype_exists_and_plan_struct_is_still_16_ints():
    assert "amdspeech_lstm_plan_xw_ksteps" in _l.PROTOTYPES
    assert _l.PROTOTYPES["amdspeech_lstm_plan_xw_ksteps"] == _l.PROTOTYPES["amdspeech_lstm_plan_xw_halves"]
    assert hasattr(_l.load(), "amdspeech_lstm_plan_xw_ksteps")
    assert C.sizeof(_l.LstmPlanInfo) == 16 * C.sizeof(C.c_int) and len(_l.LstmPlanInfo._fields_) == 16
    with open(os.path.join(ROOT, "include", "amdspeech.h")) as fh:
        assert "int amdspeech_lstm_plan_xw_ksteps(const amdspeech_lstm_desc* d, int C, int U);" in fh.read()


_CHILD = """
import ctypes as C, json, sys
from rnn_speech_amd import lib as _l
lib = _l.load()
out = {}
for (B, H, L) in ((32, 512, 3), (16, 512, 2), (20, 512, 2)):
    for T in (1, 64, 1001):
        d = _l.LstmDesc(T, B, H, L, 1.0, 1.0, 0, 0, 0)
        out["%d,%d,%d,%d" % (B, H, L, T)] = int(lib.amdspeech_lstm_workspace_bytes(C.byref(d)))
print(json.dumps(out))
"""


def test_workspace_bytes_do_not_depend_on_the_switch():
    sizes = {}
    for switch in (None, "3", "2", "1", "0"):
        env = dict(os.environ)
        env.pop("AMDSPEECH_FLOW_FWD_WORKERS", None)
        if switch is not None:
            env["AMDSPEECH_FLOW_FWD_WORKERS"] = switch
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        sizes[switch] = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(sizes[None]) == 9 and all(v > 0 for v in sizes[None].values())
    for switch, got in sizes.items():
        assert got == sizes[None], (switch, got, sizes[None])


# ---- the split, restated.  H = 512: KB = 4 K blocks of 16 rows per recurrence wave and half, MV = 1.  Row k of W_ih lies in K block
# k // 16, which belongs to wave (k // 16) // KB as its block (k // 16) % KB; inside the block the row is k-step k % 4 of lane group
# (k % 16) // 4 (pack_fwd_kernel / packed_off: k = kb * 16 + 4 * kq + m).  Gate g of a unit is N tile g (i, j, f, o).
KB, MV, H = 4, 1, 512


def split_masks(me, cut_from=None):
    """Boolean masks [H rows of W_ih, 4 gates] of who multiplies what: the recurrence wave, the full role (block KB-1, all four N
    tiles), the half role (block KB-1-MV, N tiles 2 and 3, and with ME > 0 k-steps 4-ME .. 3 of block KB-2-MV for the same tiles).
    cut_from: where the recurrence wave stops multiplying those two tiles of block KB-2-MV (4 - ME when the two sides agree)."""
    cut_from = 4 - me if cut_from is None else cut_from
    k = np.arange(H)
    blk, step = (k // 16) % KB, k % 4
    full = np.zeros((H, 4), bool)
    half = np.zeros((H, 4), bool)
    rec = np.zeros((H, 4), bool)
    full[blk == KB - 1, :] = True
    half[blk == KB - 1 - MV, 2:] = True
    half[(blk == KB - 2 - MV) & (step >= 4 - me), 2:] = True
    rec[blk < KB - 1 - MV, :] = True
    rec[blk == KB - 1 - MV, :2] = True
    rec[(blk == KB - 2 - MV) & (step >= cut_from), 2:] = False
    return rec, full, half


@pytest.mark.parametrize("me", [0, 1, 2, 3])
def test_three_way_split_adds_up_exactly(me):
    rng = np.random.RandomState(me)
    x = rng.randint(-3, 4, size=(16, H)).astype(np.float32)
    w = rng.randint(-3, 4, size=(H, 4, 16)).astype(np.float32)           # [row, gate, unit of one 16-unit block]
    whole = np.einsum("bk,kgu->bgu", x, w)
    rec, full, half = split_masks(me)
    assert not (rec & full).any() and not (rec & half).any() and not (full & half).any()
    assert (rec | full | half).all()
    parts = [np.einsum("bk,kgu->bgu", x, w * m[:, :, None]) for m in (rec, full, half)]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)          # (integers below 2^24: f32 sums are exact)
    # per recurrence wave and step: 16 MFMAs per block and N tile quartet -- 40 - 2 ME for the wave's x half, 64 + 16 ME per half role
    per_wave_rec = rec.sum() // 4 // 8        # (k-steps x N tiles per wave; one MFMA covers 4 rows)
    assert per_wave_rec == 40 - 2 * me
    assert half.sum() // 4 == 64 + 16 * me and full.sum() // 4 == 128


@pytest.mark.parametrize("me", [1, 2, 3])
def test_an_off_by_one_kstep_range_breaks_the_split(me):
    rng = np.random.RandomState(10 + me)
    x = rng.randint(1, 4, size=(16, H)).astype(np.float32)
    w = rng.randint(1, 4, size=(H, 4, 16)).astype(np.float32)            # (positive: a dropped or doubled k-step cannot cancel)
    whole = np.einsum("bk,kgu->bgu", x, w)
    for cut_from in (4 - me - 1, 4 - me + 1):                            # the wave drops one k-step too many / keeps one too many
        rec, full, half = split_masks(me, cut_from=cut_from)
        got = sum(np.einsum("bk,kgu->bgu", x, w * m[:, :, None]) for m in (rec, full, half))
        assert np.array_equal(got[:, :2], whole[:, :2])                   # gates i and j are not part of it
        assert (got[:, 2:] != whole[:, 2:]).all(), cut_from
