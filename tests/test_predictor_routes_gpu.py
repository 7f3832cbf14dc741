"""The host side of the LayerNorm score predictor against tests/golden/predictor_routes.json (tools/gen_predictor_routes.py, recorded
before the four copies of its launch sequence - PredictorFn, SmallPredictorFn, ragged_predictor_forward, RaggedPredictorFn - were folded
into predictor_forward_sequence / predictor_backward_sequence of d2s/functional.py): for every configuration of tests/predictor_routes.py the C-ABI entries the forward and the backward
issue are the recorded ones in the recorded order, the bytes saved for the backward are the recorded ones (nothing under no_grad), and
the peak of allocated memory is not above the recorded one."""
import json
import os

import pytest

from tests import predictor_routes

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predictor_routes.json")


def test_predictor_routes_saved_bytes_and_peak_memory_are_the_recorded_ones():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    configs = predictor_routes.configurations()
    assert sorted(name for name, _ in configs) == sorted(fixture)
    bad = []
    for name, cfg in configs:          # in the order of the recording: the caching allocator then rounds as it did there
        got, _ = predictor_routes.record(cfg)
        want = fixture[name]
        print(f"{name}: forward {len(got['forward'])} backward {len(got['backward'])} calls, saved {got['saved_bytes']} B, "
              f"peak {got['peak_bytes']} B (recorded {want['peak_bytes']} B)")
        if not cfg["train"]:
            assert got["saved_bytes"] == 0 and not got["backward"], name
        for k in ("forward", "backward", "saved_bytes"):
            if got[k] != want[k]:
                bad.append((name, k, got[k], want[k]))
        if got["peak_bytes"] > want["peak_bytes"]:
            bad.append((name, "peak_bytes", got["peak_bytes"], want["peak_bytes"]))
    assert not bad, bad
