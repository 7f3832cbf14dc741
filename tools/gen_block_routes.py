#!/usr/bin/env python3
"""Record tests/golden/block_routes.json: for every configuration of tests/block_routes.py (BlockFn, ragged_block_forward, AttnCoreFn
across arithmetic modes, grad modes, policies, stochastic depth; the token-merging block across merge counts, sizes and replays; the
graph-rank, key-metric and LTP soft blocks; ragged blocks with an LTP or an ATS stage) the
C-ABI entries issued by the forward and by the backward, the bytes saved for the backward and the peak of allocated memory.  Needs the
GPU.  It goes through the public entry points only, so the same file runs on any commit: record on the commit whose host-side behaviour
is to be kept, change the code, let tests/test_block_routes_gpu.py compare.

    python tools/gen_block_routes.py                  # rewrite the fixture
    python tools/gen_block_routes.py --dump DIR       # write every output and gradient tensor to DIR/block_routes.pt instead
    python tools/gen_block_routes.py --compare DIR    # torch.equal of every tensor against such a file, and the routes against the fixture
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "dense2sparse-vit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(stem="block_routes"):
    """stem: the recorder under tests/ (tools/gen_predictor_routes.py passes its own), also the name of the fixture and of the dump"""
    import importlib

    import torch
    recorder = importlib.import_module(f"tests.{stem}")
    fixture_path = os.path.join(REPO, "tests", "golden", f"{stem}.json")
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--compare", metavar="DIR")
    args = ap.parse_args()
    routes, tensors = recorder.record_all()
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        torch.save(tensors, os.path.join(args.dump, f"{stem}.pt"))
        print(f"{len(tensors)} configurations, {sum(len(v) for v in tensors.values())} tensors -> {args.dump}")
        return 0
    if args.compare:
        want = torch.load(os.path.join(args.compare, f"{stem}.pt"))
        with open(fixture_path) as f:
            fixture = json.load(f)
        bad = [f"{name}: configurations differ" for name in set(want) ^ set(tensors)]
        for name in sorted(set(want) & set(tensors)):
            if sorted(want[name]) != sorted(tensors[name]):
                bad.append(f"{name}: tensors {sorted(tensors[name])}, expected {sorted(want[name])}")
                continue
            bad += [f"{name}: {k} differs" for k, t in want[name].items() if not torch.equal(t, tensors[name][k])]
            for k in ("forward", "backward", "saved_bytes"):
                if routes[name][k] != fixture[name][k]:
                    bad.append(f"{name}: {k} {routes[name][k]}, fixture {fixture[name][k]}")
            if routes[name]["peak_bytes"] > fixture[name]["peak_bytes"]:
                bad.append(f"{name}: peak_bytes {routes[name]['peak_bytes']} above the fixture's {fixture[name]['peak_bytes']}")
        print("\n".join(bad) if bad else
              f"{len(tensors)} configurations, {sum(len(v) for v in tensors.values())} tensors: bit for bit equal, routes as recorded")
        return 1 if bad else 0
    with open(fixture_path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(routes[k], sort_keys=True)}" for k in sorted(routes)) + "\n}\n")      # one line each
    print(f"{len(routes)} configurations -> {fixture_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
