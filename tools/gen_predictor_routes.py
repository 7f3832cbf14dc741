#!/usr/bin/env python3
"""Record tests/golden/predictor_routes.json: for every configuration of tests/predictor_routes.py (the LayerNorm score predictor, large
and small, on dense and on packed rows, across arithmetic modes, grad modes and what wants a gradient) the C-ABI entries issued by the
forward and by the backward, the bytes saved for the backward and the peak of allocated memory.  Needs the GPU.  It goes through the
public entry points only, so the same file runs on any commit: record on the commit whose host-side behaviour is to be kept, change the
code, let tests/test_predictor_routes_gpu.py compare.  The options are tools/gen_block_routes.py's, whose main this runs:

    python tools/gen_predictor_routes.py                  # rewrite the fixture
    python tools/gen_predictor_routes.py --dump DIR       # write every output and gradient tensor to DIR/predictor_routes.pt instead
    python tools/gen_predictor_routes.py --compare DIR    # torch.equal of every tensor against such a file, and the routes against the fixture
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_block_routes import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main("predictor_routes"))
