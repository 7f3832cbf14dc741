"""The host side of the transformer block against tests/golden/block_routes.json (tools/gen_block_routes.py, recorded before the five
copies of the launch sequence in d2s/functional.py were folded into one, and the token-merging configurations before the copies in
d2s/functional_tome.py followed them): for every configuration of tests/block_routes.py the C-ABI entries the forward and the backward
issue are the recorded ones in the recorded order, the bytes saved for the backward are the recorded ones (nothing under no_grad), and
the peak of allocated memory is not above the recorded one."""
import json
import os

import pytest

from tests import block_routes

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_routes.json")


def test_block_routes_saved_bytes_and_peak_memory_are_the_recorded_ones():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    configs = block_routes.configurations()
    assert sorted(name for name, _ in configs) == sorted(fixture)
    bad = []
    for name, cfg in configs:          # in the order of the recording: the caching allocator then rounds as it did there
        got, _ = block_routes.record(cfg)
        want = fixture[name]
        print(f"{name}: forward {len(got['forward'])} backward {len(got['backward'])} calls, saved {got['saved_bytes']} B, "
              f"peak {got['peak_bytes']} B (recorded {want['peak_bytes']} B)")
        if not cfg.get("train", cfg["kind"] == "attn"):
            assert got["saved_bytes"] == 0 and not got["backward"], name
        for k in ("forward", "backward", "saved_bytes"):
            if got[k] != want[k]:
                bad.append((name, k, got[k], want[k]))
        if got["peak_bytes"] > want["peak_bytes"]:
            bad.append((name, "peak_bytes", got["peak_bytes"], want["peak_bytes"]))
    assert not bad, bad
