#!/usr/bin/env python3
"""Generate tests/golden/droppath_micro.npz by running the REFERENCE's own student on the CPU with drop_path_rate = 0.5.

Runs only where the reference exists (never on the GPU machine).  The reference's model file is loaded the way tools/gen_golden.py loads
it; the `timm.models.layers.DropPath` it imports is the reference's own restatement, taken from the text of vit_models/deit.py
(`drop_path` and `class DropPath`) by `ast` at run time, as tests/golden/param_groups.json was made from utils.py.  A thin subclass
records the 0/1 vector of every call: it replays the generator state to see the draw the real call is about to make, and changes nothing.

Two sections, outputs only:
  (plain keys)  the smallest model case of tests/cases.py (micro1) with a batch of 4, training mode: masks [2 * depth, B], logits, a
                slice and the sums of the features, pred_logits and kept ids per stage, the loss of a fixed linear probe of the three
                differentiable outputs and per-parameter gradient norms + leading elements
  thr_*         the dynamic-keep-ratio case micro_thr1 (patch_score_threshold set: no token is removed, the keep mask is the attention
                policy) at the same rate: the same quantities, with the keep mask in place of the kept ids

The torch seed is searched from SEED0 upwards until the recorded masks are not vacuous: at least half of the rows with a non-zero rate
hold both a 0 and a 1, and no sample is dropped in every such row.

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_droppath_fixture.py
"""
import ast
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402
from d2s import synth  # noqa: E402
from tests import cases  # noqa: E402

RATE = 0.5
BATCH = 4
SEED0 = 2026


def reference_drop_path():
    """(drop_path, DropPath) as vit_models/deit.py defines them"""
    tree = ast.parse(open(os.path.join(G.REF, "vit_models", "deit.py")).read())
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name == "drop_path") or
            (isinstance(n, ast.ClassDef) and n.name == "DropPath")]
    assert len(body) == 2, "deit.py no longer defines drop_path and DropPath at module level"
    ns = {"torch": torch, "nn": nn}
    exec(compile(ast.Module(body=body, type_ignores=[]), "deit.py(drop_path, DropPath)", "exec"), ns)
    return ns["drop_path"], ns["DropPath"]


def load_reference_with_drop_path():
    drop_path, RefDropPath = reference_drop_path()

    class RecordingDropPath(RefDropPath):
        def forward(self, x):
            if self.training and self.drop_prob:
                state = torch.get_rng_state()
                probe = drop_path(torch.ones((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype), self.drop_prob, True)
                torch.set_rng_state(state)                       # the real call below makes the same draw
                self.__dict__.setdefault("recorded", []).append((probe.flatten() != 0).float())
            return super().forward(x)

    dv, losses, _ = G._load_reference()
    dv.DropPath = RecordingDropPath              # the name Block.__init__ resolves at :249
    return dv


def build(dv, case, threshold=None):
    cfg = case["cfg"]
    with contextlib.redirect_stdout(io.StringIO()):
        student = dv.VisionTransformerDiffPruning(
            img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
            mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
            token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True, small_predictor=cfg["small_predictor"],
            predictor_loss_type=cfg["loss_type"], drop_path_rate=RATE, patch_score_threshold=threshold)
    sd_s, _ = cases.make_weights(case)
    G._load_sd(student, sd_s)
    return student.train()


def recorded_masks(student, B):
    rows = []
    for blk in student.blocks:
        rec = getattr(blk.drop_path, "recorded", None)
        if rec is None:
            assert isinstance(blk.drop_path, nn.Identity)
            rows += [torch.ones(B), torch.ones(B)]
        else:
            assert len(rec) == 2, "one call per residual branch"
            rows += rec
            del rec[:]
    return torch.stack(rows)


def vacuous(masks, rates):
    live = masks[[r for r, p in enumerate(rates) if p > 0]]
    mixed = sum(1 for row in live if 0 < row.sum() < row.numel())
    return mixed * 2 < live.shape[0] or bool((live.sum(dim=0) == 0).any())


def run(dv, case, tag, threshold=None):
    cfg = case["cfg"]
    B = case["batch"]
    x = G._t(synth.images(B, 3, cfg["img_size"], seed=case["seed"]))
    student = build(dv, case, threshold)
    rates = [p for p in (q.item() for q in torch.linspace(0, RATE, cfg["depth"])) for _ in (0, 1)]
    for seed in range(SEED0, SEED0 + 1000):
        torch.manual_seed(seed)
        logits, features, pred_logits, sel = student(x.clone())
        masks = recorded_masks(student, B)
        if not vacuous(masks, rates):
            break
    assert not vacuous(masks, rates), "no seed gave masks with both values in half of the rows and no sample dropped everywhere"
    if threshold is not None:                    # :1011 returns the last stage's tensors only
        pred_logits, sel = [pred_logits], [sel]
    g1 = G._t(synth.normal(f"droppath/{tag}/g1", tuple(logits.shape), seed=case["seed"]))
    g2 = G._t(synth.normal(f"droppath/{tag}/g2", tuple(features.shape), seed=case["seed"]))
    g3 = [G._t(synth.normal(f"droppath/{tag}/g3/{i}", tuple(p.shape), seed=case["seed"])) for i, p in enumerate(pred_logits)]
    probe = (logits * g1).sum() + (features * g2).sum() / features.shape[1] + sum((p * g).sum() for p, g in zip(pred_logits, g3))
    student.zero_grad()
    probe.backward()
    out = {"seed": np.array(seed), "rate": np.array(RATE), "batch": np.array(B), "masks": G._np(masks), "rates": np.array(rates),
           "logits": G._np(logits), "features_slice": G._np(features[:, :4, :16]), "features_sum": G._np(features.double().sum(dim=(1, 2))),
           "features_shape": np.array(features.shape), "probe_loss": G._np(probe)}
    for i, (p, s) in enumerate(zip(pred_logits, sel)):
        out[f"pred_logits_{i}"] = G._np(p)
        out[f"kept_{i}"] = G._np(s)
    names, norms, heads = [], [], []
    for n_, p in student.named_parameters():
        names.append(n_)
        if p.grad is None:
            norms.append(-1.0)
            heads.append(np.zeros(8, np.float32))
        else:
            g = p.grad.detach().flatten()
            norms.append(float(g.double().norm()))
            h = np.zeros(8, np.float32)
            h[: min(8, g.numel())] = G._np(g[:8])
            heads.append(h)
    out["grad_names"], out["grad_norms"], out["grad_heads"] = np.array(names), np.array(norms, np.float64), np.stack(heads)
    print(f"[golden] droppath {tag}: seed {seed}, masks\n{masks.int().numpy()}\n probe loss {float(probe):.6f}")
    return out


def main():
    dv = load_reference_with_drop_path()
    out = run(dv, dict(cases.MODEL_CASES["micro1"], batch=BATCH), "micro1")
    thr_case = cases.THRESHOLD_CASES["micro_thr1"]
    thr = run(dv, thr_case, "micro_thr1", threshold=thr_case["threshold"])
    out.update({"thr_" + k: v for k, v in thr.items()})
    path = os.path.join(G.OUT, "droppath_micro.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 500 * 1024
    print(f"[golden] wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
