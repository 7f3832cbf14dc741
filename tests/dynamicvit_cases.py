"""The DynamicViT baseline's parity cases (micro geometry: D 128, 2 heads, depth 4, 64x64 images, N = 16, B = 4), shared by
tools/gen_dynamicvit_fixture.py and the tests.  Weights and images are re-derived from d2s.synth, never stored."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "dense2sparse-vit_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from d2s import synth  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "dynamicvit_micro.npz")


def _cfg(pruning_loc, token_ratio):
    return dict(img_size=64, patch=16, dim=128, depth=4, heads=2, num_classes=10, init_n=16, pruning_loc=tuple(pruning_loc),
                token_ratio=tuple(token_ratio))


CASES = {
    "stage1": dict(cfg=_cfg((1,), (0.5,)), batch=4, seed=71),
    "stage2": dict(cfg=_cfg((1, 2), (0.5, 0.25)), batch=4, seed=72),
}


def param_shapes(cfg):
    D, P, hid = cfg["dim"], cfg["patch"], cfg["dim"] * 4
    N = (cfg["img_size"] // P) ** 2
    s = {"cls_token": (1, 1, D), "pos_embed": (1, N + 1, D), "patch_embed.proj.weight": (D, 3, P, P), "patch_embed.proj.bias": (D,),
         "norm.weight": (D,), "norm.bias": (D,), "head.weight": (cfg["num_classes"], D), "head.bias": (cfg["num_classes"],)}
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        s.update({b + "norm1.weight": (D,), b + "norm1.bias": (D,), b + "attn.qkv.weight": (3 * D, D), b + "attn.qkv.bias": (3 * D,),
                  b + "attn.proj.weight": (D, D), b + "attn.proj.bias": (D,), b + "norm2.weight": (D,), b + "norm2.bias": (D,),
                  b + "mlp.fc1.weight": (hid, D), b + "mlp.fc1.bias": (hid,), b + "mlp.fc2.weight": (D, hid), b + "mlp.fc2.bias": (D,)})
    for j in range(len(cfg["pruning_loc"])):
        b = f"score_predictor.{j}."
        s.update({b + "in_conv.0.weight": (D,), b + "in_conv.0.bias": (D,), b + "in_conv.1.weight": (D, D), b + "in_conv.1.bias": (D,),
                  b + "out_conv.0.weight": (D // 2, D), b + "out_conv.0.bias": (D // 2,), b + "out_conv.2.weight": (D // 4, D // 2),
                  b + "out_conv.2.bias": (D // 4,), b + "out_conv.4.weight": (2, D // 4), b + "out_conv.4.bias": (2,)})
    return s


def make_weights(case):
    sd = synth.fill_state_dict(list(param_shapes(case["cfg"]).items()), seed=case["seed"], std=0.02, std_overrides={"score_predictor": 0.08})
    return synth.perturb_affine(sd, seed=case["seed"])


def make_images(case):
    return synth.images(case["batch"], 3, case["cfg"]["img_size"], seed=case["seed"])


GRAD_SAMPLES = 16


def grad_sample(g):
    """GRAD_SAMPLES evenly strided elements of a flattened gradient (parameters are listed in sorted-name order in the fixture)"""
    import torch
    flat = g.reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, GRAD_SAMPLES).long()
    return flat[idx]
