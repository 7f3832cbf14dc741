#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own Python on CPU.

Runs only in the survey/build container (needs /root/reference); the GPU box never runs this.  The
reference's files are imported unmodified, by path, without executing vit_models/__init__.py (which
pulls in model files that need timm/torchvision).  Seven third-party symbols that are absent here are
provided as in-memory modules; none of them is on the arithmetic path at the
configurations used (drop_path=0 -> nn.Identity at dynamic_vit.py:249, mixup off -> CrossEntropyLoss
at losses.py:174, init values are overwritten by synth weights).

Weights / inputs are NOT stored: they are re-derived anywhere from dense2sparse-vit_amd/d2s/synth.py.
Only reference OUTPUTS are stored (plus the torch-RNG noise tensor of the perturbed top-k cases, which
is captured from the reference's autograd ctx because it cannot be re-derived).

usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "dense2sparse-vit_amd"))
sys.path.insert(0, REPO)
from d2s import synth  # noqa: E402
from tests import cases  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")


def _install_standins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            assert p == 0.0

        def forward(self, x):
            return x

    class SoftTargetCrossEntropy(nn.Module):
        def forward(self, x, target):
            return torch.sum(-target * torch.log_softmax(x, dim=-1), dim=-1).mean()

    def to_2tuple(x):
        return tuple(x) if isinstance(x, (tuple, list)) else (x, x)

    mod("timm")
    mod("timm.data", IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225))
    mod("timm.models")
    mod("timm.models.layers", DropPath=DropPath, to_2tuple=to_2tuple, trunc_normal_=nn.init.trunc_normal_)
    mod("timm.models.registry", register_model=lambda f: f)
    mod("timm.models.helpers", load_pretrained=lambda *a, **k: None)
    mod("timm.loss", SoftTargetCrossEntropy=SoftTargetCrossEntropy)


def _load_reference():
    _install_standins()
    pkg = types.ModuleType("vit_models")
    pkg.__path__ = [os.path.join(REF, "vit_models")]
    sys.modules["vit_models"] = pkg

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    load("vit_models.peturbed_topk", os.path.join(REF, "vit_models", "peturbed_topk.py"))
    dv = load("vit_models.dynamic_vit", os.path.join(REF, "vit_models", "dynamic_vit.py"))
    losses = load("ref_losses", os.path.join(REF, "losses.py"))
    for f in ("transformer_block", "token_transformer", "token_performer", "t2t_vit"):
        load("vit_models." + f, os.path.join(REF, "vit_models", f + ".py"))
    return dv, losses, sys.modules["vit_models.peturbed_topk"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.detach().cpu().numpy()


def _load_sd(module, sd):
    own = module.state_dict()
    buffers = {k for k in own if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}   # BatchNorm buffers keep their
    assert set(own.keys()) - buffers == set(sd.keys()), (sorted((set(own) - buffers) ^ set(sd)))          # fresh-module values
    module.load_state_dict({**{k: own[k] for k in buffers}, **{k: _t(v) for k, v in sd.items()}}, strict=True)


class _Args:
    pass


def build_ref_models(dv, case):
    cfg = case["cfg"]
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        student = dv.VisionTransformerDiffPruning(
            img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
            num_heads=cfg["heads"], mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"],
            pruning_loc=list(cfg["pruning_loc"]), token_ratio=list(cfg["token_ratio"]), distill=True,
            topk_selection=True, small_predictor=cfg["small_predictor"], predictor_loss_type=cfg["loss_type"],
            predictor_bn=bool(cfg.get("predictor_bn")))
        teacher = dv.VisionTransformerTeacher(
            img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"],
            num_heads=cfg["heads"], mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"])
    sd_s, sd_t = cases.make_weights(case)
    _load_sd(student, sd_s)
    _load_sd(teacher, sd_t)
    return student, teacher


def gen_model_case(dv, losses, name):
    case = cases.MODEL_CASES[name]
    cfg = case["cfg"]
    student, teacher = build_ref_models(dv, case)
    x = _t(cases.make_images(case))
    y = _t(cases.make_labels(case))
    out = {}

    # ---- training-mode step exactly as train.py:40-57 (minus the optimiser) ----
    student.train()
    teacher.eval()
    args = _Args()
    args.keep_ratios = list(cfg["token_ratio"])
    args.mask_loss_type = cfg["loss_type"]
    args.mixup = 0.0
    args.patch_score_threshold = None
    mask_fn = losses.MaskLoss(args, "train")
    bb_fn = losses.BackboneLoss(args)
    metrics = {}
    logits_t, token_t, cls_attn = teacher(x.clone())
    logits_s, token_s, pred_logits, kept = student(x.clone())
    mask_loss = mask_fn(pred_logits, cls_attn, kept, metrics)
    bb_loss = bb_fn(logits_s, token_s, logits_t, token_t, kept, y, metrics)
    total = bb_loss + mask_loss
    student.zero_grad()
    total.backward()

    out["logits_t"] = _np(logits_t)
    out["cls_attn_t"] = _np(cls_attn)
    out["token_t_slice"] = _np(token_t[:, :4, :16])
    out["token_t_sum"] = _np(token_t.double().sum(dim=(1, 2)))
    out["logits_s"] = _np(logits_s)
    out["token_s_slice"] = _np(token_s[:, :4, :16])
    out["token_s_sum"] = _np(token_s.double().sum(dim=(1, 2)))
    out["token_s_shape"] = np.array(token_s.shape)
    for i, (pl, k_) in enumerate(zip(pred_logits, kept)):
        out[f"pred_logits_{i}"] = _np(pl)
        out[f"kept_{i}"] = _np(k_)
        out[f"dropped_{i}"] = _np(student.dropped_token_indices[i])
    out["mask_loss"] = _np(mask_loss)
    out["backbone_loss"] = _np(bb_loss)
    for k_, v in metrics.items():
        out["metric_" + k_] = np.array(float(v))
    out["student_cls_attn_0"] = _np(student.cls_attns[0])
    out["student_cls_attn_last"] = _np(student.cls_attns[-1])
    names = []
    norms = []
    heads = []
    for n_, p in student.named_parameters():
        names.append(n_)
        if p.grad is None:
            norms.append(-1.0)
            heads.append(np.zeros(8, np.float32))
        else:
            g = p.grad.detach().flatten()
            norms.append(float(g.double().norm()))
            h = np.zeros(8, np.float32)
            h[: min(8, g.numel())] = _np(g[:8])
            heads.append(h)
    out["grad_names"] = np.array(names)
    out["grad_norms"] = np.array(norms, np.float64)
    out["grad_heads"] = np.stack(heads)

    for k_, v in student.state_dict().items():          # BatchNorm running estimates after this one training step (predictor_bn)
        if k_.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["buf_" + k_] = _np(v)

    # predictor-only gradient probe: logits.sum().backward() leaves predictors at None
    # ---- eval-mode forward (dynamic_vit.py:1015) ----
    student.eval()
    with torch.no_grad():
        e_logits, e_cls, e_pl, e_kept = student(x.clone())
        full = teacher.forward_cls_attention(x.clone())
    out["eval_logits"] = _np(e_logits)
    out["eval_n_cls"] = np.array(len(e_cls))
    out["eval_cls_shapes"] = np.array([list(c.shape) for c in e_cls])
    out["eval_cls_3"] = _np(e_cls[min(3, len(e_cls) - 1)])
    for i, k_ in enumerate(e_kept):
        out[f"eval_kept_{i}"] = _np(k_)
    out["teacher_cls_attention_equal"] = np.array(bool(torch.equal(full, cls_attn)))
    np.savez_compressed(os.path.join(OUT, f"model_{name}.npz"), **out)
    print(f"[golden] model_{name}: mask_loss={float(mask_loss):.6f} backbone_loss={float(bb_loss):.6f} "
          f"kept shapes={[tuple(k_.shape) for k_ in kept]}")


def gen_threshold_case(dv, name):
    """Dynamic keep ratio: the reference's student in TRAINING mode with patch_score_threshold set (dynamic_vit.py:880-894,981-983 -
    threshold selection + softmax_with_policy attention in every block; this forward runs as written).  Stored: logits, features,
    the last stage's pred_logits and keep mask (what :1011 returns), the per-image keep ratios, and the parameter gradients of a fixed
    linear probe of the three differentiable outputs (the reference's own losses cannot run on this path, losses.py:81,216-218).
    The eval-mode forward of this path raises NameError (`score`, :936) in the reference: recorded, nothing to store."""
    case = cases.THRESHOLD_CASES[name]
    cfg = case["cfg"]
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        student = dv.VisionTransformerDiffPruning(
            img_size=cfg["img_size"], patch_size=cfg["patch"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
            mlp_ratio=cfg["mlp_ratio"], qkv_bias=True, num_classes=cfg["num_classes"], pruning_loc=list(cfg["pruning_loc"]),
            token_ratio=list(cfg["token_ratio"]), distill=True, topk_selection=True, predictor_loss_type=cfg["loss_type"],
            patch_score_threshold=case["threshold"])
    sd_s, _ = cases.make_weights(case)
    _load_sd(student, sd_s)
    student.train()
    x = _t(cases.make_images(case))
    logits, features, pred_logits, keep_mask = student(x.clone())
    out = {"logits": _np(logits), "features_slice": _np(features[:, :4, :16]), "features_sum": _np(features.double().sum(dim=(1, 2))),
           "features_shape": np.array(features.shape), "pred_logits_last": _np(pred_logits), "keep_mask_last": _np(keep_mask),
           "keep_ratios": _np(student.keep_ratios)}
    g1 = _t(synth.normal(f"thr/{name}/g1", tuple(logits.shape), seed=case["seed"]))
    g2 = _t(synth.normal(f"thr/{name}/g2", tuple(features.shape), seed=case["seed"]))
    g3 = _t(synth.normal(f"thr/{name}/g3", tuple(pred_logits.shape), seed=case["seed"]))
    student.zero_grad()
    ((logits * g1).sum() + (features * g2).sum() / features.shape[1] + (pred_logits * g3).sum()).backward()
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
            h[: min(8, g.numel())] = _np(g[:8])
            heads.append(h)
    out["grad_names"], out["grad_norms"], out["grad_heads"] = np.array(names), np.array(norms, np.float64), np.stack(heads)
    student.eval()
    try:
        with torch.no_grad():
            student(x.clone())
        out["eval_error"] = np.array("none")
    except Exception as e:      # NameError: name 'score' is not defined (dynamic_vit.py:936)
        out["eval_error"] = np.array(f"{type(e).__name__}: {e}")
    np.savez_compressed(os.path.join(OUT, f"threshold_{name}.npz"), **out)
    print(f"[golden] threshold_{name}: kept per image {keep_mask.sum(dim=1).tolist()}  eval: {out['eval_error']}")


def gen_threshold_selection():
    """Threshold selection alone on the selection fixtures' probability rows (incl. exact ties and a constant row), with the
    reference's own four calls (dynamic_vit.py:881-883,891: sort ascending, cumsum, compare, scatter) executed verbatim here because
    they sit inline in forward() - the model-level threshold fixtures pin the same lines through the reference's class."""
    out = {}
    for N in (196, 576, 16):
        p = _t(cases.make_selection_probs(N))
        for th in (0.1, 0.35, 0.8):
            val, idx = torch.sort(p.detach().clone())
            cum_sum = torch.cumsum(val, dim=-1)
            t = (cum_sum > th)
            spatial_mask = torch.empty(p.shape, dtype=torch.bool)
            spatial_mask = torch.scatter(input=spatial_mask, dim=1, index=idx, src=t)
            out[f"mask_{N}_{th}"] = _np(spatial_mask)
            # margin of the decision: distance of the nearest running sum to the threshold (rows below ~1e-6 are rounding-decided)
            out[f"margin_{N}_{th}"] = _np((cum_sum - th).abs().min(dim=1).values)
    np.savez_compressed(os.path.join(OUT, "threshold_selection.npz"), **out)
    print(f"[golden] threshold_selection: {len(out)} arrays")


def gen_micro_intermediates(dv, name="micro1"):
    """Every intermediate of the micro geometry: per-op fixtures for LN / attention / MLP / predictor."""
    case = cases.MODEL_CASES[name]
    student, _ = build_ref_models(dv, case)
    student.train()
    x = _t(cases.make_images(case))
    out = {}
    with torch.no_grad():
        t = student.patch_embed(x)
        out["patch_embed"] = _np(t)
        B = t.shape[0]
        t = torch.cat((student.cls_token.expand(B, -1, -1), t), dim=1) + student.pos_embed
        out["tokens0"] = _np(t)
        blk = student.blocks[0]
        ln1 = blk.norm1(t)
        out["blk0_ln1"] = _np(ln1)
        a, cls_row = blk.attn(ln1, policy=None, return_cls_attn=True)
        out["blk0_attn_out"] = _np(a)
        out["blk0_cls_row"] = _np(cls_row)
        t1 = t + a
        ln2 = blk.norm2(t1)
        m = blk.mlp(ln2)
        out["blk0_mlp_out"] = _np(m)
        t2 = t1 + m
        out["blk0_out"] = _np(t2)
        scores, probs = student.score_predictor[0](t2[:, 1:])
        out["pred0_scores"] = _np(scores)
        out["pred0_probs"] = _np(probs)
        h = student.score_predictor[0].in_conv(t2[:, 1:])
        out["pred0_in_conv"] = _np(h)
        # softmax_with_policy (dynamic_vit.py:195-214) on a deterministic attn / policy pair
        attn = _t(synth.normal("policy/attn", (2, 2, 9, 9), std=2.0, seed=7))
        pol = _t((synth.normal("policy/mask", (2, 9, 1), seed=7) > 0).astype(np.float32))
        pol[:, 0] = 1.0
        out["policy_attn_in"] = _np(attn)
        out["policy_mask"] = _np(pol)
        out["policy_softmax"] = _np(blk.attn.softmax_with_policy(attn, pol))
    np.savez_compressed(os.path.join(OUT, f"intermediates_{name}.npz"), **out)
    print(f"[golden] intermediates_{name}: {len(out)} tensors")


def gen_selection():
    """Selection fixtures (dynamic_vit.py:858-862) incl. deliberate exact ties and collapsed softmax rows."""
    out = {}
    for N, ks in ((196, (137, 98, 58)), (576, (172, 288, 58)), (16, (9, 5)), (4, (4,))):
        probs = cases.make_selection_probs(N)
        out[f"probs_{N}"] = probs
        p = _t(probs)
        for k in ks:
            order = torch.argsort(p, dim=1, descending=True)
            kept = torch.sort(order[:, :k], dim=1)[0]
            dropped = torch.sort(order[:, k:], dim=1)[0]
            out[f"kept_{N}_{k}"] = _np(kept)
            out[f"dropped_{N}_{k}"] = _np(dropped)
            srt = torch.sort(p, dim=1, descending=True)[0]
            kk = min(k, N - 1)
            out[f"margin_{N}_{k}"] = _np(srt[:, kk - 1] - srt[:, kk]) if k < N else np.zeros(p.shape[0], np.float32)
    np.savez_compressed(os.path.join(OUT, "selection.npz"), **out)
    print(f"[golden] selection: {len(out)} arrays")


def gen_perturbed_topk(ptk):
    out = {}
    for tag, (b, nS, d, k, sigma) in cases.PTK_CASES.items():
        x = _t(synth.normal(f"ptk/{tag}/x", (b, d), std=1.0, seed=3)).requires_grad_(True)
        ind = ptk.PerturbedTopKFunction.apply(x, k, nS, sigma)
        noise = ind.grad_fn.noise
        onehot = ind.grad_fn.perturbed_output
        g = _t(synth.normal(f"ptk/{tag}/g", (b, k, d), std=1.0, seed=4))
        ind.backward(g)
        out[f"{tag}_noise"] = _np(noise)
        out[f"{tag}_indicators"] = _np(ind)
        out[f"{tag}_ids"] = _np(onehot.argmax(dim=-1))
        out[f"{tag}_grad_x"] = _np(x.grad)
    np.savez_compressed(os.path.join(OUT, "perturbed_topk.npz"), **out)
    print(f"[golden] perturbed_topk: {len(out)} arrays")


def gen_t2t():
    """T2T_ViT (performer and transformer token encoders) at a micro geometry, eval mode (dropout off): per-module outputs,
    logits, per-block normed outputs and parameter-gradient norms of sum(logits * g)."""
    import contextlib
    import io
    t2t = sys.modules["vit_models.t2t_vit"]
    out = {}
    for tt in ("performer", "transformer"):
        c = cases.T2T_CASE
        with contextlib.redirect_stdout(io.StringIO()):
            m = t2t.T2T_ViT(img_size=c["img_size"], tokens_type=tt, embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"],
                            mlp_ratio=c["mlp_ratio"], num_classes=c["num_classes"], token_dim=64)
        sd = cases.make_t2t_weights(tt)
        own = m.state_dict()
        assert list(own.keys()) == list(sd.keys()), [k for k in own if k not in sd] + [k for k in sd if k not in own]
        m.load_state_dict({k: _t(v) for k, v in sd.items()})
        m.eval()
        x = _t(cases.make_t2t_images())
        tok0 = m.tokens_to_token.soft_split0(x).transpose(1, 2)
        a1 = m.tokens_to_token.attention1(tok0)
        out[f"{tt}_unfold0"] = _np(tok0)
        out[f"{tt}_attention1"] = _np(a1)
        out[f"{tt}_t2t_module"] = _np(m.tokens_to_token(x))
        logits, heads = m.forward_features(x)[0], None
        cls_feat, block_heads = m.forward_features(x)
        logits = m.head(cls_feat)
        out[f"{tt}_logits"] = _np(logits)
        out[f"{tt}_block_head_last"] = _np(block_heads[-1])
        g = _t(synth.normal("t2t/g", tuple(logits.shape), seed=9))
        m.zero_grad()
        (logits * g).sum().backward()
        names, norms = [], []
        for n_, p_ in m.named_parameters():
            names.append(n_)
            norms.append(-1.0 if p_.grad is None else float(p_.grad.double().norm()))
        out[f"{tt}_grad_names"] = np.array(names)
        out[f"{tt}_grad_norms"] = np.array(norms)
    np.savez_compressed(os.path.join(OUT, "t2t.npz"), **out)
    print(f"[golden] t2t: {len(out)} arrays")


def gen_t2t_224():
    """BASELINE config 4 at its own geometry: the reference's T2T_ViT with the T2T-ViT-14 hyper-parameters (t2t_vit.py:182-199) on one
    224x224 image, both token encoders (performer = T2t_vit_14, transformer = T2t_vit_t_14), eval mode: the 3136-token soft split and
    first token encoder, the T2T module output, logits, the last block's normed output and every parameter-gradient norm of
    sum(logits * g).  Slices + fp64 sums are stored where the tensors are large."""
    import contextlib
    import io
    t2t = sys.modules["vit_models.t2t_vit"]
    c = cases.T2T_224_CASE
    out = {}
    for tt in ("performer", "transformer"):
        with contextlib.redirect_stdout(io.StringIO()):
            m = t2t.T2T_ViT(img_size=c["img_size"], tokens_type=tt, embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"],
                            mlp_ratio=c["mlp_ratio"], num_classes=c["num_classes"], token_dim=64)
        sd = cases.make_t2t_weights(tt, case=c)
        own = m.state_dict()
        assert list(own.keys()) == list(sd.keys())
        m.load_state_dict({k: _t(v) for k, v in sd.items()})
        m.eval()
        x = _t(cases.make_t2t_images(c))
        tok0 = m.tokens_to_token.soft_split0(x).transpose(1, 2)
        a1 = m.tokens_to_token.attention1(tok0)
        tm = m.tokens_to_token(x)
        out[f"{tt}_unfold0_shape"] = np.array(tok0.shape)
        out[f"{tt}_unfold0_slice"] = _np(tok0[:, 1000:1004, :])
        out[f"{tt}_attention1_slice"] = _np(a1[:, ::392, :])
        out[f"{tt}_attention1_sum"] = _np(a1.double().sum(dim=(0, 2)))[::49]
        out[f"{tt}_t2t_module_shape"] = np.array(tm.shape)
        out[f"{tt}_t2t_module_slice"] = _np(tm[:, ::28, ::8])
        out[f"{tt}_t2t_module_sum"] = _np(tm.double().sum(dim=2))
        cls_feat, block_heads = m.forward_features(x)
        logits = m.head(cls_feat)
        out[f"{tt}_logits"] = _np(logits)
        out[f"{tt}_block_head_last_slice"] = _np(block_heads[-1][:, ::16])
        out[f"{tt}_n_block_heads"] = np.array(len(block_heads))
        g = _t(synth.normal("t2t224/g", tuple(logits.shape), seed=9))
        m.zero_grad()
        (logits * g).sum().backward()
        names, norms = [], []
        for n_, p_ in m.named_parameters():
            names.append(n_)
            norms.append(-1.0 if p_.grad is None else float(p_.grad.double().norm()))
        out[f"{tt}_grad_names"] = np.array(names)
        out[f"{tt}_grad_norms"] = np.array(norms)
        print(f"[golden] t2t_224 {tt}: logits[:3] {logits[0, :3].tolist()}")
    np.savez_compressed(os.path.join(OUT, "t2t_224.npz"), **out)
    print(f"[golden] t2t_224: {len(out)} arrays")


def gen_mask_loss_mse(losses):
    """MaskLoss with mask_loss_type='mse' (losses.py:61-73) at loss level: synthetic scores / teacher CLS-attention rows / kept ids in,
    loss and d loss / d scores out (two stages, so that the re-gather + renormalisation of the target is covered)."""
    B, L, H, N = 3, 4, 2, 16
    k0, k1 = 11, 5
    normal = lambda name, shape, std: synth.normal(name, shape, std=std, seed=13)
    cls_attn = torch.softmax(_t(normal("mse/cls", (B, L, H, N + 1), 1.0)), dim=-1)
    p0 = _t(normal("mse/p0", (B, N), 0.5)).requires_grad_(True)
    p1 = _t(normal("mse/p1", (B, k0), 0.5)).requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    kept0 = torch.stack([torch.randperm(N, generator=g)[:k0].sort().values for _ in range(B)])
    kept1 = torch.stack([torch.randperm(k0, generator=g)[:k1].sort().values for _ in range(B)])
    args = _Args()
    args.keep_ratios, args.mask_loss_type = [0.7, 0.35], "mse"
    fn = losses.MaskLoss(args, "train")
    metrics = {}
    loss = fn([p0, p1], cls_attn, [kept0, kept1], metrics)
    loss.backward()
    np.savez_compressed(os.path.join(OUT, "mask_loss_mse.npz"), cls_attn=_np(cls_attn), p0=_np(p0), p1=_np(p1), kept0=_np(kept0), kept1=_np(kept1),
                        loss=_np(loss), g0=_np(p0.grad), g1=_np(p1.grad), metric_keys=np.array(sorted(metrics)))
    print("mask_loss_mse.npz loss", float(loss), sorted(metrics))


def gen_param_groups(dv):
    """Optimiser parameter groups and the per-epoch LR / freeze schedule of the reference (utils.py:66-147).  utils.py as a module
    needs torchvision and the whole model zoo, so only its two function definitions are taken from its text (ast) and executed against
    the reference's own student class; the fixture stores group membership by parameter name and, per epoch, the group learning
    rates, every parameter's requires_grad flag and the top-k sigma."""
    import ast
    import contextlib
    import io
    import json
    import math
    tree = ast.parse(open(os.path.join(REF, "utils.py")).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("get_param_groups", "adjust_learning_rate")]
    assert len(fns) == 2
    ns = {"math": math, "torch": torch}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "utils.py(two functions)", "exec"), ns)
    case = cases.MODEL_CASES["micro2"]
    student, _ = build_ref_models(dv, case)
    args = _Args()
    args.weight_decay, args.lr, args.min_lr, args.epochs, args.warmup_steps = 0.05, 5e-4, 1e-5, 10, 3
    args.topk_selection, args.initial_sigma, args.early_exit = True, 0.05, False
    groups = ns["get_param_groups"](student, args)
    by_id = {id(p): n for n, p in student.named_parameters()}
    out = {"args": {k: getattr(args, k) for k in ("weight_decay", "lr", "min_lr", "epochs", "warmup_steps", "initial_sigma")},
           "groups": {g["name"]: {"weight_decay": g["weight_decay"], "params": [by_id[id(p)] for p in g["params"]]} for g in groups},
           "epochs": []}
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            ns["adjust_learning_rate"](groups, args, epoch, student, warmup_predictor=False, warming_up_step=args.warmup_steps, base_multi=0.1)
        out["epochs"].append({"lr": {g["name"]: g["lr"] for g in groups}, "sigma": args.current_sigma,
                              "frozen": sorted(n for n, p in student.named_parameters() if not p.requires_grad)})
    json.dump(out, open(os.path.join(OUT, "param_groups.json"), "w"), indent=1)
    print("param_groups.json", {k: len(v["params"]) for k, v in out["groups"].items()}, [len(e["frozen"]) for e in out["epochs"]])


def gen_checkpoint_ingestion(dv):
    """checkpoint_filter_fn / resize_pos_embed of the reference (dynamic_vit.py:1178-1213) on a synthetic DeiT-style checkpoint: a
    {'model': ...} wrapper, a patch projection stored as a matrix, and a 4x4-grid position table loaded into a 6x6-grid model."""
    normal = lambda name, shape, std: synth.normal(name, shape, std=std, seed=11)
    D, P = 16, 4
    model = types.SimpleNamespace(patch_embed=types.SimpleNamespace(proj=types.SimpleNamespace(weight=torch.zeros(D, 3, P, P))),
                                  pos_embed=torch.zeros(1, 1 + 36, D))
    sd = {"pos_embed": _t(normal("ckpt.pos", (1, 1 + 16, D), 0.5)), "patch_embed.proj.weight": _t(normal("ckpt.proj", (D, 3 * P * P), 0.1)),
          "head.bias": _t(normal("ckpt.hb", (10,), 0.1))}
    out = dv.checkpoint_filter_fn({"model": dict(sd)}, model)
    np.savez_compressed(os.path.join(OUT, "checkpoint.npz"), **{"in." + k: _np(v) for k, v in sd.items()}, **{"out." + k: _np(v) for k, v in out.items()})
    print("checkpoint.npz", {k: tuple(v.shape) for k, v in out.items()})


def gen_gemm_workspace_bytes():
    """What the BUILT library's two GEMM workspace queries return (host arithmetic; the CU count falls back to 256 without a GPU), recorded
    before a change to the GEMM host code so that the changed library can be held to the same numbers: `gen_golden.py gemm_workspace`."""
    import json
    from d2s import lib
    from tests import gemm_cases as C
    deit = [(D, no, ni) for D in (192, 384, 768) for (no, ni) in ((3 * D, D), (D, D), (4 * D, D), (D, 4 * D))]
    shapes = list(C.all_shapes())
    shapes += [(rows, no, ni) for (_, no, ni) in deit for rows in (197, 99, 197 * 32, 197 * 128)]           # forward / dgrad: M = rows
    shapes += [(no, ni, rows) for (_, no, ni) in deit for rows in (197, 99, 197 * 32, 197 * 128)]           # weight gradient: K = rows
    # K no multiple of 32 / of 64 (padded pieces), and long reductions where rounding to K blocks lowers the slice count
    shapes += [(64, 96, 40), (96, 72, 600), (130, 132, 1000), (2048, 1024, 100), (4096, 256, 72), (384, 384, 21800), (384, 384, 25216 + 32),
               (256, 256, 2080), (300, 260, 4100), (1536, 384, 2049)]
    gemm = [[lay, M, N, K, mode, lib.query("d2s_gemm_f32_workspace_bytes", lay, M, N, K, mode)]
            for (M, N, K) in sorted(set(shapes)) for lay in (0, 1, 2) for mode in (0, 1, 2)]
    wgrad = [[t, no, ni, mode, lib.query("d2s_linear_wgrad_workspace_bytes", t, no, ni, mode)]
             for (_, no, ni) in deit for t in (2048, 25216, 50000) for mode in (0, 1, 2)]
    with open(os.path.join(OUT, "gemm_workspace_bytes.json"), "w") as f:
        json.dump({"d2s_gemm_f32_workspace_bytes": gemm, "d2s_linear_wgrad_workspace_bytes": wgrad}, f, separators=(",", ":"))
    print("gemm_workspace_bytes.json", len(gemm), len(wgrad))


def main():
    if sys.argv[1:] == ["gemm_workspace"]:      # needs the built library only, not the reference
        return gen_gemm_workspace_bytes()
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dv, losses, ptk = _load_reference()
    gen_selection()
    gen_perturbed_topk(ptk)
    gen_micro_intermediates(dv)
    gen_t2t()
    gen_t2t_224()
    gen_checkpoint_ingestion(dv)
    gen_param_groups(dv)
    gen_mask_loss_mse(losses)
    gen_threshold_selection()
    for name in cases.THRESHOLD_CASES:
        gen_threshold_case(dv, name)
    for name in cases.MODEL_CASES:
        gen_model_case(dv, losses, name)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"[golden] total fixture bytes: {total}")
    # hygiene: the reference tree must stay pristine (no __pycache__)
    for root, dirs, _ in os.walk(REF):
        assert "__pycache__" not in dirs, f"bytecode cache written under {root}"


if __name__ == "__main__":
    main()
