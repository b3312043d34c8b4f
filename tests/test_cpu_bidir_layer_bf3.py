"""Layer-wise bidirectional stacks at precision = bf16x3: the library's workspace and path queries, which run on the host (no GPU
needed).  The f32 sizes are pinned to what the library returned before bf16x3 existed: its regions come after all of them."""
import ctypes

import pytest

SHAPES = [(17, 3, 64, 2), (50, 20, 128, 3), (200, 32, 256, 2), (1001, 32, 512, 3), (998, 64, 1024, 5)]      # T, B, H, L

# amdspeech_lstm_bidir_workspace_bytes / _layer_stride at precision 0 before the bf16x3 kernels were added
F32_BYTES = {(17, 3, 64, 2): (687104, 59520), (50, 20, 128, 3): (35984128, 2314240), (200, 32, 256, 2): (341116928, 29523968),
             (1001, 32, 512, 3): (4593033472, 295272448), (998, 64, 1024, 5): (27737465088, 1177550848),
             (40, 12, 128, 2): (12841728, 1112064), (30, 8, 64, 2): (3215872, 278528)}


def _lib():
    from rnn_speech_amd import lib as _l
    return _l, _l.load()


def query(T, B, H, L, precision):
    _l, lib = _lib()
    d = _l.LstmDesc(T, B, H, L, 1.0, 1.0, 0, precision)
    return (lib.amdspeech_lstm_bidir_workspace_bytes(ctypes.byref(d)), lib.amdspeech_lstm_bidir_path(ctypes.byref(d)),
            lib.amdspeech_lstm_bidir_layer_stride(ctypes.byref(d)))


def ring_bytes(B, H):
    """Two directions x two slots of the split loop-carried panel: [16 * ceil(B / 16)][4H] bf16 hi + lo."""
    return 2 * 2 * ((B + 15) // 16 * 16) * 4 * H * 4


@pytest.mark.parametrize("shape", sorted(F32_BYTES), ids=lambda s: "T%d-B%d-H%d-L%d" % s)
def test_f32_sizes_are_unchanged(shape):
    nbytes, path, stride = query(*shape, precision=0)
    assert (nbytes, stride) == F32_BYTES[shape]
    assert path >= 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-B%d-H%d-L%d" % s)
def test_bf3_workspace_is_the_f32_layout_plus_the_rings(shape):
    T, B, H, L = shape
    nbytes, path, stride = query(T, B, H, L, precision=1)
    assert nbytes > 0 and path >= 0
    assert nbytes == F32_BYTES[shape][0] + ring_bytes(B, H)
    assert stride == F32_BYTES[shape][1]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-B%d-H%d-L%d" % s)
def test_plain_bf16_stays_unsupported(shape):
    nbytes, path, stride = query(*shape, precision=2)
    assert nbytes == 0 and path == -3 and stride == -1          # AMDSPEECH_EUNSUPPORTED


@pytest.mark.parametrize("H", [288, 416, 800])
def test_bf3_refuses_hidden_sizes_its_kernels_cannot_take(H):
    _l, lib = _lib()
    nbytes, path, _ = query(20, 4, H, 2, precision=1)
    assert nbytes == 0 and path == -3
    assert "hidden size %d" % H in lib.amdspeech_last_error().decode()
    assert query(20, 4, H, 2, precision=0)[0] > 0                # (exact f32 takes them)


@pytest.mark.parametrize("H", [32, 96, 160, 224, 320, 768])
def test_bf3_takes_other_hidden_sizes_its_kernels_split(H):
    assert query(20, 4, H, 2, precision=1)[0] > 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d-B%d-H%d-L%d" % s)
def test_bf3_workspace_covers_every_shorter_run_length(shape):
    """ops.BidirWorkspace.prefix re-lays one max_T allocation out for each shorter mini-batch: the size must be monotone in T."""
    T, B, H, L = shape
    root = query(T, B, H, L, precision=1)[0]
    step = 1 if T <= 256 else 7
    for t in list(range(1, T, step)) + [T - 1]:
        n = query(t, B, H, L, precision=1)[0]
        assert 0 < n <= root, (t, n, root)
