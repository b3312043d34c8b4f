"""The engine's library-call sequence against tests/golden/engine_calls.json, configuration by configuration: same calls, same order,
same scalars, same views of the same buffers, same waits, same hook placements as the engine recorded before it was rebuilt on the
recurrence drivers (tests/engine_calls.py says what an entry holds).  The parity tests compare numbers within tolerances; a reordered
launch, a swapped buffer, a dropped accumulate or a wait that moved behind the recurrence can stay inside those.  Exact: no tolerance."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_calls  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_calls.json")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(engine_calls.CONFIGS))
def test_engine_records_the_golden_call_sequence(name):
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert name in golden, "no golden sequence for configuration %r" % name
    got = json.loads(json.dumps(engine_calls.record(name)))
    want = golden[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "entry %d of %s:\n  recorded %s\n  golden   %s" % (i, name, json.dumps(g), json.dumps(w))
    longer, n = (got, len(want)) if len(got) > len(want) else (want, len(got))
    assert len(got) == len(want), "%s: %d entries recorded, %d in the golden; the first one past the shorter list: %s" % (
        name, len(got), len(want), json.dumps(longer[n]))


def test_golden_holds_exactly_the_configurations():
    with open(GOLDEN) as fh:
        assert list(json.load(fh)) == list(engine_calls.CONFIGS)
