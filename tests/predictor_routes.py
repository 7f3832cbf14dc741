"""What the LayerNorm score predictor's host code does, per configuration, through the public entry points only
(PredictorLG.forward_tokens, functional_ragged.ragged_predictor_forward and ragged_predictor_train): the C-ABI entries it issues (forward,
backward), the bytes it saves for the backward - once per distinct storage, so a slot that aliases another is not counted twice - and its
peak of allocated memory.  Shared by tools/gen_predictor_routes.py, which records tests/golden/predictor_routes.json, and
tests/test_predictor_routes_gpu.py, which compares a fresh recording with it.  The spy and the allocator discipline are
tests/block_routes.py's (record_call).

Geometry, the smallest at which every branch is live: D = 64 (the bf16 data path needs D % 32 == 0; the large predictor's exact-fp32 tail
is 32 -> 16 -> 1 wide); dense B = 2, n = 33; packed the row counts ROWS of tests/test_ragged_train_gpu.py (a CLS-only image, one token,
fewer rows than a wave, more than one tile)."""
import torch

from tests import block_routes
from tests.test_ragged_train_gpu import ROWS, _cu, _t

DEV = block_routes.DEV
D = 64
B, N = 2, 33
MODES = block_routes.MODES


def configurations():
    """[(name, dict)] in the order they are run"""
    out = []

    def add(kind, small, mode, train, grads="all"):
        name = f"{kind}/{'small' if small else 'large'}/{mode}/{'train' if train else 'nograd'}"
        out.append((name + ("" if grads == "all" else f"/only_{grads}"), dict(kind=kind, small=small, mode=mode, train=train, grads=grads)))
    for small in (False, True):          # the small predictor keeps fp32 activations: no bf16 data path to record
        for mode in (("exact", "split") if small else MODES):
            for train in (True, False):
                add("dense", small, mode, train)
    for small in (False, True):
        for mode in (("exact", "split") if small else MODES):
            add("packed_forward", small, mode, False)
    for small in (False, True):          # training on the packed batch is refused in the bf16 mode
        for mode in ("exact", "split"):
            for train in (True, False):
                add("packed_train", small, mode, train)
    for kind in ("dense", "packed_train"):          # the backward prunes its launches by what wants a gradient
        for small in (False, True):
            for grads in ("x", "params"):
                add(kind, small, "bf16" if (kind == "dense" and not small) else "exact", True, grads)
    return out


_HOST = {}


def _synth(tag, shape):
    """a fresh device tensor per call; the values are made once"""
    from d2s import synth
    if (tag, shape) not in _HOST:
        _HOST[tag, shape] = _t(synth.normal(f"predictor_routes/{tag}", shape, seed=23))
    return _HOST[tag, shape].to(DEV)


def _predictor(small):
    """a fresh PredictorLG on the device; the weights are made once (LayerNorm affines and biases perturbed: every term non-trivial)"""
    from d2s import synth
    from vit_models.dynamic_vit import PredictorLG
    pred = PredictorLG(D, topk_selection=True, k=8, small_predictor=small)
    if ("weights", small) not in _HOST:
        shapes = [(k, tuple(v.shape)) for k, v in pred.state_dict().items()]
        _HOST["weights", small] = {k: _t(v) for k, v in synth.perturb_affine(synth.fill_state_dict(shapes, seed=23), seed=23).items()}
    pred.load_state_dict(_HOST["weights", small], strict=True)
    return pred.to(DEV)


def _make(cfg):
    """-> (call, leaves, gy) as tests/block_routes.py's record_call takes them"""
    from d2s.functional_ragged import ragged_predictor_forward, ragged_predictor_train
    pred = _predictor(cfg["small"])
    for p in pred.parameters():
        p.requires_grad_(cfg["grads"] in ("all", "params"))
    leaves = {f"dp/{k}": p for k, p in pred.named_parameters()}
    grad_mode = torch.enable_grad if cfg["train"] else torch.no_grad
    if cfg["kind"] == "dense":
        x = _synth("x", (B, N, D)).requires_grad_(cfg["grads"] in ("all", "x"))
        gy = _synth("gy", (B, N - 1))

        def call():
            with grad_mode():
                scores, probs = pred.forward_tokens(x)
            return dict(scores=scores, probs=probs), (scores if cfg["train"] else None)
    else:
        cu = _cu(ROWS).to(DEV)
        total = sum(ROWS)
        x = _synth("xp", (total, D)).requires_grad_(cfg["grads"] in ("all", "x"))
        gy = _synth("gyp", (total,))
        entry = ragged_predictor_train if cfg["kind"] == "packed_train" else ragged_predictor_forward

        def call():
            with grad_mode():
                scores = entry(pred, x, cu, len(ROWS))
            return dict(scores=scores), (scores if cfg["train"] else None)
    leaves["dx"] = x
    return call, leaves, gy


def record(cfg):
    """One configuration.  -> ({forward, backward, saved_bytes, peak_bytes}, {name: output or gradient tensor})"""
    return block_routes.record_call(lambda: _make(cfg), cfg["mode"], distinct=True)


def record_all():
    """-> ({name: route}, {name: {tensor name: tensor}})"""
    routes, tensors = {}, {}
    for name, cfg in configurations():
        routes[name], outs = record(cfg)
        tensors[name] = {k: t.detach().cpu() for k, t in outs.items() if t is not None}
    return routes, tensors
