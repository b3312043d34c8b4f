"""First-pass fusion end to end on the GPU: a small random language model behind LmStepper and FusedDecoder against
lm_fusion_ref's dictionary decoder driven by the float64 step, and stt.build_rescorer at lm_fusion : beam."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_fusion_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(L, H, seed, width) for (L, H), rows in sorted(F.GPU_CASES.items()) for seed, width in rows]


def _reference(lm, lg, width):
    """Per utterance: the dictionary decoder's winner and the smallest gap over the mini-batch."""
    paths, gap = [], np.inf
    for b, Tb in enumerate(F.GPU_LENGTHS):
        if Tb == 0:
            paths.append([])
            continue
        ranked, g = F.fused_prefix_beam_search(lg[:Tb, b], F.GPU_C - 1, width, lm, F.GPU_LM_WEIGHT, F.GPU_BONUS)
        paths.append(ranked[0][0])
        gap = min(gap, g)
    return paths, gap


@pytest.fixture(scope="module")
def oracle_lms():
    return {(L, H): F.OracleLm(F.gpu_lm_params(L, H), L) for L, H in F.GPU_LM_SHAPES}


def test_the_case_table_holds_the_shapes_and_widths_asked_for():
    assert sorted(F.GPU_CASES) == [(1, 16), (2, 48)] and F.GPU_C == 6 and F.GPU_T == 30 and F.GPU_LENGTHS == (30, 17, 0)
    assert all({w for _, w in rows} == {4, 8} for rows in F.GPU_CASES.values())


@pytest.mark.parametrize("L,H,seed,width", CASES)
def test_the_fused_decoder_on_the_gpu_equals_the_reference_decoder(oracle_lms, L, H, seed, width):
    from rnn_speech_amd.language_model import FusedDecoder
    lg = F.gpu_posteriors(seed)
    want, gap = _reference(oracle_lms[(L, H)], lg, width)
    assert gap > F.GPU_GAP, "the case table must hold only seeds whose reference gap is clear (%g)" % gap
    dec = FusedDecoder(F.gpu_lm_params(L, H), F.GPU_LM_WEIGHT, width, F.GPU_BONUS)
    ids, out_len = dec(lg, np.array(F.GPU_LENGTHS, np.int32), width, False)
    assert [list(ids[b, :out_len[b]]) for b in range(len(want))] == want
    st = dec.stepper
    assert st.n_slots == 3 * 2 * width + 1 and st.calls <= F.GPU_T + 1 and st.rows > st.calls
    # and the model mattered: the acoustic beam alone decodes something else
    from rnn_speech_amd import ops
    plain, plain_len, _ = ops.ctc_beam_search(lg, list(F.GPU_LENGTHS), width, False)
    assert [list(plain[b, :plain_len[b]]) for b in range(len(want))] != want


def test_build_rescorer_returns_a_fused_decoder_that_decode_passes_through(tmp_path, oracle_lms):
    import stt
    from rnn_speech_amd.acoustic_model import AcousticModel
    from rnn_speech_amd.language_model import FusedDecoder, NbestRescorer
    L, H = 2, 48
    seed, width = F.GPU_CASES[(L, H)][0]
    hp = {"lm_num_layers": L, "lm_hidden_size": H, "lm_batch_size": 2, "max_target_seq_length": 40, "char_map_length": F.GPU_C,
          "precision": "f32", "checkpoint_dir": str(tmp_path), "lm_weight": F.GPU_LM_WEIGHT, "lm_length_bonus": F.GPU_BONUS,
          "lm_nbest": 4, "lm_fusion": "beam"}
    model = stt._language_model(hp, training=False)
    model.engine.load_numpy(F.gpu_lm_params(L, H))
    model.save(None, hp["checkpoint_dir"])
    assert isinstance(stt.build_rescorer(dict(hp, lm_fusion="rescore")), NbestRescorer)
    assert stt.build_rescorer(dict(hp, lm_weight=0)) is None
    rescorer = stt.build_rescorer(hp)
    assert isinstance(rescorer, FusedDecoder) and rescorer.lm_weight == F.GPU_LM_WEIGHT and rescorer.lm_length_bonus == F.GPU_BONUS
    lg = F.gpu_posteriors(seed)
    want, gap = _reference(oracle_lms[(L, H)], lg, width)
    assert gap > F.GPU_GAP
    me = types.SimpleNamespace(decoder="beam", rescorer=rescorer, engine=types.SimpleNamespace(logits=torch.as_tensor(lg).cuda()),
                               beam_width=width, merge_repeated=False, num_labels=F.GPU_C)
    dense = AcousticModel._decode(me, torch.as_tensor(np.array(F.GPU_LENGTHS, np.int32)).cuda())
    assert dense.shape == (3, max(len(w) for w in want))
    for b, w in enumerate(want):
        assert list(dense[b, :len(w)]) == w and all(v == F.GPU_C for v in dense[b, len(w):])
