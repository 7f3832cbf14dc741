"""GPU tier of save / resume / evaluate and of the EMA weights kept inside the fused AdamW launch (d2s_adamw_step_ema).

A resumed run must continue THE SAME trajectory: the schedule is 2 epochs x 2 steps with warmup_steps=1, so epoch 0 trains the predictors
only and the per-tensor AdamW counters of predictor and backbone differ when the checkpoint is taken.  Two uninterrupted runs are
compared first (the control); everything else is held to the control, bit for bit.

EMA parity bound (test_ema_matches_a_float64_restatement): per step the kernel rounds three times (two products and a sum, or a product
and a fused multiply-add) with unit round-off 2**-24, and the recurrence e <- d e + (1 - d) p is a contraction, so after K steps
|ema - e64| <= 3 K 2**-24 max(|p|, |e|) per tensor (largest error against largest magnitude), and element by element against the
largest |p| or |e| the element went through during the K steps.  Derived, not measured."""
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.test_model_gpu import build_models, make_args, _t

pytestmark = pytest.mark.gpu

HP = dict(lr=5e-4, min_lr=1e-5, weight_decay=0.05, epochs=4, warmup_steps=1)
CASES = ["micro2", "micro1"]          # build_models switches topk_selection on for every case; micro2 has two pruning stages
DEV = "cuda:0"


def _step(case, graph=False, ema=None, scramble=False, cfg=None):
    """New student, teacher and TrainStep.  scramble: the student starts from other weights than the case's (drawn from torch's RNG,
    which a later load_state_dict has to put back)."""
    from d2s.engine import TrainStep
    dev = torch.device(DEV)
    if cfg is not None:
        case = dict(case, cfg=cfg)
    student, teacher, _, _ = build_models(case, dev)
    if scramble:
        with torch.no_grad():
            for p in student.parameters():
                p.add_(0.01 * torch.randn(p.shape).to(dev))
    ts = TrainStep(student, teacher, make_args(case["cfg"]), graph=graph, **HP)
    if ema is not None:
        ts.enable_ema(ema)
    return ts


def _batches(case, n, first=0):
    from d2s import synth
    cfg, dev = case["cfg"], torch.device(DEV)
    return [(_t(synth.images(case["batch"], 3, cfg["img_size"], seed=700 + i)).to(dev),
             _t(synth.labels(case["batch"], cfg["num_classes"], seed=700 + i)).to(dev)) for i in range(first, first + n)]


def _epoch(ts, epoch, data):
    """-> per step: kept ids of every stage and the gradient arena (what the step computed from the weights it found)"""
    ts.set_epoch(epoch)
    rec = []
    for x, y in data:
        info = ts(x, y)
        torch.cuda.synchronize()
        rec.append(([k.clone() for k in info["kept"]], ts.arena.grads.clone(), info["loss"].clone()))
    return rec


def _snap(ts):
    torch.cuda.synchronize()
    out = dict(params=ts.arena.params.clone(), exp_avg=ts.opt.exp_avg.clone(), exp_avg_sq=ts.opt.exp_avg_sq.clone(),
               chunk_steps=ts.opt.chunk_steps.clone())
    if ts.opt.ema is not None:
        out["ema"] = ts.opt.ema.clone()
    return out


def _assert_same(a, b, tag, keys=None):
    for k in keys or a:
        if not torch.equal(a[k], b[k]):
            d = (a[k].double() - b[k].double()).abs()
            raise AssertionError(f"{tag}: {k} differs in {int((d > 0).sum())} of {d.numel()} elements, max abs {float(d.max()):.3e}")


def _assert_same_steps(ra, rb, tag):
    assert len(ra) == len(rb)
    for i, ((ka, ga, la), (kb, gb, lb)) in enumerate(zip(ra, rb)):
        for s, (p, q) in enumerate(zip(ka, kb)):
            assert torch.equal(p, q), f"{tag}: kept ids of step {i}, stage {s} differ"
        assert torch.equal(la, lb), f"{tag}: loss of step {i} differs ({float(la)} vs {float(lb)})"
        assert torch.equal(ga, gb), f"{tag}: gradients of step {i} differ"


def _uninterrupted(case, ema=None, graph=False, seed=1234):
    ts = _step(case, ema=ema, graph=graph)
    torch.manual_seed(seed)               # after the models are built: their constructors draw from the same generator
    r0 = _epoch(ts, 0, _batches(case, 2))
    r1 = _epoch(ts, 1, _batches(case, 2, first=2))
    return ts, r0, r1


def _interrupted(case, tmp_path, ema=None, graph=False, seed=1234):
    """epoch 0 -> state_dict -> file -> weights_only load -> NEW objects with other initial weights -> load_state_dict -> epoch 1"""
    ts = _step(case, ema=ema, graph=graph)
    torch.manual_seed(seed)
    _epoch(ts, 0, _batches(case, 2))
    path = os.path.join(str(tmp_path), "last.pt")
    torch.save(ts.state_dict(best_acc=0.5), path)
    del ts
    sd = torch.load(path, map_location="cpu", weights_only=True)
    torch.manual_seed(999)
    ts2 = _step(case, ema=ema, graph=graph, scramble=True)
    assert ts2.load_state_dict(sd) == 0 and sd["best_acc"] == 0.5
    return ts2, sd


@pytest.mark.parametrize("name", CASES)
def test_control_two_uninterrupted_runs_are_bit_identical(name):
    case = cases.MODEL_CASES[name]
    a, a0, a1 = _uninterrupted(case)
    b, b0, b1 = _uninterrupted(case)
    _assert_same_steps(a0 + a1, b0 + b1, "control")
    _assert_same(_snap(a), _snap(b), "control")
    steps = a.opt.chunk_steps.cpu().numpy()                  # the counters the checkpoint has to carry: 4 / 2 / 0
    for i, n in enumerate(a.arena.names):
        c0, c1 = a.arena.chunk_range(i)
        want = 0 if ("cls_token" in n or "pos_embed" in n) else (4 if "predictor" in n else 2)
        assert (steps[c0:c1] == want).all(), (n, steps[c0:c1], want)


@pytest.mark.parametrize("name", CASES)
def test_resume_continues_the_same_trajectory(name, tmp_path):
    from d2s import ops
    case = cases.MODEL_CASES[name]
    ctrl, _, c1 = _uninterrupted(case)
    ts, sd = _interrupted(case, tmp_path)
    ts.arena.check_alias()                                   # loading copied INTO the arena
    for n, p in ts.student.named_parameters():
        assert torch.equal(p.detach().cpu(), sd["model"][n]), n
    w = ts.student.blocks[1].mlp.fc1.weight
    assert torch.equal(ops.transposed_weight(w), w.detach().t()), "a cached W^T copy survived the load"
    r1 = _epoch(ts, 1, _batches(case, 2, first=2))
    # the first step after the load computed its gradients - input-gradient GEMMs included - from the loaded weights
    _assert_same_steps(c1, r1, "resumed epoch 1")
    _assert_same(_snap(ctrl), _snap(ts), "resumed run")
    # the file speaks in parameter names and shapes, not in arena terms
    own = {n: tuple(p.shape) for n, p in ts.student.named_parameters()}
    assert set(sd["optimizer"]["state"]) == set(own)
    for n, e in sd["optimizer"]["state"].items():
        assert tuple(e["exp_avg"].shape) == own[n] == tuple(e["exp_avg_sq"].shape) and isinstance(e["step"], int)
    assert sd["optimizer"]["state"]["blocks.0.attn.qkv.weight"]["step"] == 0 and sd["optimizer"]["state"]["score_predictor.0.in_conv.1.weight"]["step"] == 2
    assert list(sd["model"]) == list(ts.student.state_dict()) and sd["epoch"] == 0


def test_hand_over_of_the_model_section(tmp_path):
    """sd['model'] in a file of its own -> weights_only load -> checkpoint_filter_fn -> a fresh student: same eval logits."""
    import vit_models
    case = cases.MODEL_CASES["micro2"]
    ts, _, _ = _uninterrupted(case)
    x = _batches(case, 1, first=9)[0][0]
    ts.student.eval()
    with torch.no_grad():
        want = ts.student(x)[0].clone()
    path = os.path.join(str(tmp_path), "student.pt")
    torch.save(ts.state_dict()["model"], path)
    fresh, _, _, _ = build_models(case, torch.device(DEV))
    with torch.no_grad():
        for p in fresh.parameters():
            p.mul_(0.5)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    missing, unexpected = fresh.load_state_dict(vit_models.checkpoint_filter_fn(sd, fresh), strict=True)
    assert not missing and not unexpected
    fresh.eval()
    with torch.no_grad():
        got = fresh(x)[0]
    assert torch.equal(want, got)


def test_mismatching_checkpoint_is_refused_and_nothing_is_written():
    from d2s.lib import D2SError
    from oracle import d2s_oracle as O
    case = cases.MODEL_CASES["micro1"]
    geom = dict(img_size=64, dim=128, depth=4, heads=2, num_classes=10, pruning_loc=(1,), init_n=16)
    src = _step(case, cfg=O.make_cfg(token_ratio=(0.5,), **geom))
    dst = _step(case, cfg=O.make_cfg(token_ratio=(0.7,), **geom), ema=0.9)
    dst.arena.params.mul_(1.5)
    before = _snap(dst)
    sd = src.state_dict()
    with pytest.raises(D2SError, match="token_ratio"):
        dst.load_state_dict(sd)
    sd["config"]["token_ratio"] = [0.7]                       # config made to fit, one tensor of the wrong shape
    sd["optimizer"]["state"]["head.bias"]["exp_avg"] = torch.zeros(3)
    with pytest.raises(D2SError, match="head.bias"):
        dst.load_state_dict(sd)
    _assert_same(before, _snap(dst), "after two refused loads")
    dst.arena.check_alias()


@pytest.mark.parametrize("name", CASES)
def test_ema_does_not_disturb_training(name):
    case = cases.MODEL_CASES[name]
    plain, p0, p1 = _uninterrupted(case)
    ema, e0, e1 = _uninterrupted(case, ema=0.9)
    _assert_same_steps(p0 + p1, e0 + e1, "with / without EMA")
    _assert_same(_snap(plain), _snap(ema), "with / without EMA", keys=["params", "exp_avg", "exp_avg_sq", "chunk_steps"])
    assert plain.opt.ema is None


def test_ema_matches_a_float64_restatement():
    case = cases.MODEL_CASES["micro2"]
    d, K = 0.9, 5
    ts = _step(case, ema=d)
    torch.manual_seed(7)
    data = _batches(case, K)
    e64 = ts.arena.params.double().cpu().numpy().copy()          # lazy start: the average begins at the weights before step 1
    seen = np.abs(e64)                                           # largest |p| or |e| an element went through
    k = 0
    for epoch, n in ((0, 2), (1, 3)):                            # frozen backbone, then everything
        ts.set_epoch(epoch)
        for _ in range(n):
            ts(*data[k])
            k += 1
            torch.cuda.synchronize()
            p = ts.arena.params.double().cpu().numpy()
            e64 = d * e64 + (1.0 - d) * p
            seen = np.maximum(seen, np.maximum(np.abs(p), np.abs(e64)))
    got = ts.opt.ema.double().cpu().numpy()
    err = np.abs(got - e64)
    tol = 3 * K * 2.0 ** -24
    a = ts.arena
    worst = worst_elem = 0.0
    pad = np.ones(a.total, dtype=bool)
    for n, o, sz in zip(a.names, a.offsets, a.sizes):
        pad[o:o + sz] = False
        sl = slice(o, o + sz)
        size = max(float(np.abs(p[sl]).max()), float(np.abs(e64[sl]).max()))          # per tensor: max(|p|, |e|)
        ratio = float(err[sl].max()) / (tol * size) if size > 0 else float(err[sl].max() > 0)
        # element by element the roundings of a step are relative to what the element was AT that step - an element whose weight
        # crosses zero ends smaller than the errors it collected - so the element-wise form of the bound takes the largest magnitude
        # the element went through
        ratio_elem = float((err[sl] / np.maximum(tol * seen[sl], 1e-300)).max()) if (seen[sl] > 0).any() else 0.0
        worst, worst_elem = max(worst, ratio), max(worst_elem, ratio_elem)
        assert err[sl].max() <= tol * size, (n, ratio)
        assert (err[sl] <= tol * seen[sl]).all(), (n, ratio_elem)
    print(f"[ema parity] worst |ema - e64| / bound over {len(a.names)} tensors: {worst:.3f} per tensor, {worst_elem:.3f} element-wise")
    assert pad.any() and (got[pad] == 0).all(), "padding of the EMA arena must stay exactly zero"
    # tensors that no step ever updates (cls_token, pos_embed) went through the loop above as well: their average stays at their value
    moved = [n for n, o, sz in zip(a.names, a.offsets, a.sizes) if (got[o:o + sz] != p[o:o + sz]).any()]
    assert any("predictor" in n for n in moved) and any(n.startswith("blocks.") for n in moved)


def test_ema_starts_from_the_weights_of_the_first_step_after_enabling():
    case = cases.MODEL_CASES["micro2"]
    d = 0.9
    ts = _step(case, ema=d)
    ts.arena.params.mul_(0.5)                                    # what a broadcast into the arena does, after enable_ema
    p0 = ts.arena.params.double().cpu().numpy().copy()
    ts.set_epoch(1)
    ts(*_batches(case, 1)[0])
    torch.cuda.synchronize()
    p1 = ts.arena.params.double().cpu().numpy()
    want = d * p0 + (1.0 - d) * p1
    got = ts.opt.ema.double().cpu().numpy()
    assert (np.abs(got - want) <= 3 * 2.0 ** -24 * np.maximum(np.abs(p1), np.abs(want))).all()
    assert np.abs(got - (d * 2.0 * p0 + (1.0 - d) * p1)).max() > 1e-3, "the average started from the weights before the overwrite"


def test_ema_weights_context_swaps_and_restores(tmp_path):
    case = cases.MODEL_CASES["micro2"]
    runs = []
    for enter in (True, False):
        ts, _, _ = _uninterrupted(case, ema=0.9)
        if enter:
            before = _snap(ts)
            assert not torch.equal(before["params"], before["ema"])
            x = _batches(case, 1, first=9)[0][0]
            fresh, _, _, _ = build_models(case, torch.device(DEV))
            fresh.load_state_dict(ts.ema_state_dict(), strict=True)
            fresh.eval()
            with torch.no_grad():
                want = fresh(x)[0].clone()
            with ts.ema_weights():
                assert torch.equal(ts.arena.params, before["ema"]) and torch.equal(ts.opt.ema, before["params"])
                ts.arena.check_alias()
                ts.student.eval()
                with torch.no_grad():
                    got = ts.student(x)[0].clone()
            assert torch.equal(want, got), "the student inside ema_weights() is not the model of ema_state_dict()"
            _assert_same(before, _snap(ts), "after ema_weights()")
        torch.manual_seed(5)
        rec = _epoch(ts, 1, _batches(case, 1, first=4))
        runs.append((rec, _snap(ts)))
    _assert_same_steps(runs[0][0], runs[1][0], "step after ema_weights()")
    _assert_same(runs[0][1], runs[1][1], "step after ema_weights()")


def test_resume_with_ema(tmp_path):
    case = cases.MODEL_CASES["micro2"]
    ctrl, _, c1 = _uninterrupted(case, ema=0.9)
    ts, sd = _interrupted(case, tmp_path, ema=0.9)
    assert sd["ema_decay"] == 0.9 and list(sd["model_ema"]) == list(sd["model"])
    r1 = _epoch(ts, 1, _batches(case, 2, first=2))
    _assert_same_steps(c1, r1, "resumed epoch 1 (EMA on)")
    _assert_same(_snap(ctrl), _snap(ts), "resumed run (EMA on)")


def test_resume_in_graph_mode_drops_the_captured_steps(tmp_path):
    """Graph vs eager is held to what tests/test_graph_gpu.py holds it to: bit-identical."""
    case = cases.MODEL_CASES["micro2"]
    data0, data1 = _batches(case, 4), _batches(case, 4, first=4)

    def first_epoch(graph):
        ts = _step(case, graph=graph)
        torch.manual_seed(21)
        _epoch(ts, 0, data0)
        return ts

    eager = first_epoch(False)
    path = os.path.join(str(tmp_path), "last.pt")
    torch.save(eager.state_dict(), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    e1 = _epoch(eager, 1, data1)                                  # the eager continuation (= eager resume, test_resume_*)

    graph = first_epoch(True)
    assert graph.last_step_captured and len(graph._graphs) == 1
    _epoch(graph, 1, data1)                                       # runs on: other weights, a second captured graph
    assert len(graph._graphs) == 2
    graph.load_state_dict(sd)
    assert graph._graphs == {} and graph._ahead is None
    graph.set_epoch(1)
    captured, rec = [], []
    for x, y in data1:
        info = graph(x, y)
        torch.cuda.synchronize()
        captured.append(graph.last_step_captured)
        rec.append(([k.clone() for k in info["kept"]], graph.arena.grads.clone(), info["loss"].clone()))
    warm = graph.GRAPH_WARM_STEPS
    assert captured == [False] * warm + [True] * (4 - warm), captured     # warmed up and captured again, nothing stale replayed
    _assert_same_steps(e1, rec, "graph resume vs eager")
    _assert_same(_snap(eager), _snap(graph), "graph resume vs eager")


def test_cli_saves_resumes_and_evaluates(tmp_path, capsys):
    import mask_predictor
    out_dir = str(tmp_path / "run")
    base = ["--arch", "deit_tiny", "--pruning-locs", "3", "--keep-ratios", "0.5", "--warmup-steps", "1", "--batch-size", "4",
            "--steps-per-epoch", "2", "--val-steps", "1", "--topk-selection"]
    last, best = os.path.join(out_dir, "last.pt"), os.path.join(out_dir, "best.pt")

    mask_predictor.main(base + ["--epochs", "2", "--output-dir", out_dir, "--model-ema"])
    out = capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == ["best.pt", "last.pt"], os.listdir(out_dir)
    assert "val_acc_ema=" in out and "Epoch 2/2" in out and "checkpoint: state_dict + write" in out
    sd = torch.load(last, map_location="cpu", weights_only=True)
    assert sd["epoch"] == 1 and "model_ema" in sd and sd["config"]["embed_dim"] == 192
    assert torch.load(best, map_location="cpu", weights_only=True)["epoch"] in (0, 1)  # written after epoch 1 whatever its accuracy; 0.0 on
                                                                                       # 4 synthetic images, so epoch 2 rarely replaces it

    mask_predictor.main(base + ["--epochs", "3", "--output-dir", out_dir, "--model-ema", "--resume", last])
    out = capsys.readouterr().out
    assert "Epoch 3/3" in out and "Epoch 1/3" not in out and "Epoch 2/3" not in out and "Training complete" in out
    assert torch.load(last, map_location="cpu", weights_only=True)["epoch"] == 2

    def val_acc(text):
        line = [ln for ln in text.splitlines() if ln.startswith("eval only:")]
        assert len(line) == 1, text
        return line[0].split("val_acc=")[1].split(",")[0]

    before = open(best, "rb").read()
    mask_predictor.main(base + ["--eval-only", "--resume", best])
    out3 = capsys.readouterr().out
    assert "val loss:" in out3 and "Training complete" not in out3 and "Epoch 1/" not in out3
    assert open(best, "rb").read() == before and sorted(os.listdir(out_dir)) == ["best.pt", "last.pt"]

    mask_predictor.main(base + ["--eval-only", "--student-checkpoint", best])
    out4 = capsys.readouterr().out
    assert "Training complete" not in out4 and val_acc(out4) == val_acc(out3)
    val_loss = lambda text: [ln for ln in text.splitlines() if ln.startswith("val loss:")][0]
    assert val_loss(out3) == val_loss(out4), "the two ways of loading best.pt evaluate different weights"
