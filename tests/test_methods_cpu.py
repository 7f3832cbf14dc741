"""The host glue of the student families (d2s, dynamicvit, tome, ats, avit, evo, ltp), pinned as text: every message the command line,
TrainStep's constructor and train_one_epoch refuse a family with, what an accepted command line prints and leaves in args, and the key
order and values of the checkpoint config.  tests/method_messages.json holds what collect() gave before the families were described in
one table (methods.py); it must give the same afterwards.

    python -m tests.test_methods_cpu --write PATH        regenerates the file
"""
import contextlib
import io
import json
import os
import sys
import types

from tests import cases  # noqa: F401  (puts the package on sys.path)

RECORDED = os.path.join(cases.REPO, "tests", "method_messages.json")
MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4.0, qkv_bias=True, num_classes=10)
METHODS = ("d2s", "dynamicvit", "tome", "ats", "avit", "evo", "ltp")
LOGITS_ONLY = ("tome", "ats", "avit", "evo", "ltp")
# one extra flag (with its value) after --method M; the last probe adds nothing
PROBES = (
    ["--tome-r", "2"], ["--ats-tokens", "8"],
    ["--avit-gate-scale", "4"], ["--avit-gate-center", "1"], ["--avit-ponder-scale", "0.001"], ["--avit-prior-alpha", "0.1"],
    ["--avit-target-depth", "5"],
    ["--evo-start", "2"], ["--evo-keep", "0.25"], ["--evo-tradeoff", "0.9"],
    ["--ltp-phase", "hard"], ["--ltp-temperature", "0.01"], ["--ltp-lambda", "0.1"], ["--ltp-init-threshold", "0.01"],
    ["--tome-train"], ["--tome-bf16"], ["--ats-train"],
    ["--topk-selection"], ["--attn-selection"], ["--fuse-dropped"], ["--squeeze-dropped"], ["--diff-topk"], ["--patch-score-threshold", "0.4"],
    ["--drop-path", "0.1"], ["--torch-optim"], ["--warmup-steps", "2"], ["--gemm-mode", "bf16"], ["--gemm-mode", "split"],
    ["--eval-only", "--student-checkpoint", "x"],
    [],
)


def _plain(v):
    """what json can hold, lists for tuples"""
    return json.loads(json.dumps(v, default=repr))


def _command_line():
    import mask_predictor
    import utils
    defaults = _plain(vars(utils.parse_args([])))
    out = {"defaults": sorted(defaults.items())}
    for method in METHODS:
        for probe in PROBES:
            argv = ["--method", method] + probe
            args = utils.parse_args(argv)
            printed = io.StringIO()
            try:
                with contextlib.redirect_stdout(printed):
                    mask_predictor.check_supported(args)
            except SystemExit as e:
                out[" ".join(argv)] = {"exit": str(e), "stdout": printed.getvalue()}
                continue
            # vars(args), as the entries that differ from the defaults recorded once above
            have = _plain(vars(args))
            assert set(have) == set(defaults)
            out[" ".join(argv)] = {"stdout": printed.getvalue(), "args": sorted((k, v) for k, v in have.items() if v != defaults[k])}
    return out


def _students():
    """one micro student per family, each as its CPU test builds it"""
    import vit_models
    import vit_models.default_dynamic_vit as DV
    return {
        "d2s": lambda **kw: vit_models.VisionTransformerDiffPruning(pruning_loc=[1], token_ratio=[0.05], distill=True,
                                                                   predictor_loss_type="kl_div", **MICRO, **kw),
        "dynamicvit": lambda **kw: DV.DefaultVisionTransformerDiffPruning(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2,
                                                                          num_classes=10, pruning_loc=[1], token_ratio=[0.5], distill=True, **kw),
        "tome": lambda **kw: vit_models.VisionTransformerToMe(**MICRO, **{**dict(tome_r=3, train_merge=True), **kw}),
        "ats": lambda **kw: vit_models.VisionTransformerATS(**MICRO, **{**dict(ats_locs=[1, 2], ats_tokens=4, train_sample=True), **kw}),
        "avit": lambda **kw: vit_models.VisionTransformerAViT(**MICRO, **kw),
        "evo": lambda **kw: vit_models.VisionTransformerEvo(**MICRO, **kw),
        "ltp": lambda **kw: vit_models.VisionTransformerLTP(**MICRO, **{**dict(pruning_loc=[0, 1]), **kw}),
    }


def _raised(fn):
    try:
        fn()
    except Exception as e:      # the type is part of the record
        return [type(e).__name__, str(e)]
    return None


def _train_step():
    from d2s import ops
    from d2s.engine import TrainStep
    from train import train_one_epoch
    make = _students()
    args = types.SimpleNamespace(mixup=0.0)
    out = {}
    with ops.gemm_mode(ops.GEMM_EXACT):
        for fam in LOGITS_ONLY:
            out[f"{fam} warmup_steps=1"] = _raised(lambda: TrainStep(make[fam](), None, args, warmup_steps=1))
            if fam != "evo":        # the one family whose step may be captured: graph=True goes on to the device
                out[f"{fam} graph=True"] = _raised(lambda: TrainStep(make[fam](), None, args, graph=True))
            dp = make[fam]()
            dp.drop_path_rate = 0.1                # the constructors refuse it; a model altered afterwards
            out[f"{fam} drop_path_rate=0.1"] = _raised(lambda: TrainStep(dp, None, args))
            out[f"{fam} not a TrainStep"] = _raised(lambda: train_one_epoch(args, make[fam](), None, [], object()))
        out["tome without train_merge"] = _raised(lambda: TrainStep(make["tome"](train_merge=False), None, args))
        out["ats without train_sample"] = _raised(lambda: TrainStep(make["ats"](ats_locs=[1], train_sample=False), None, args))
        with ops.gemm_mode(ops.GEMM_BF16):
            for phase in ("soft", "hard"):
                out[f"ltp {phase} in the bf16 mode"] = _raised(lambda: TrainStep(make["ltp"](ltp_phase=phase), None, args))
        out["d2s teacher=None"] = _raised(lambda: TrainStep(make["d2s"](), None, args))
        out["ats without stages teacher=None"] = _raised(lambda: TrainStep(make["ats"](ats_locs=[]), None, args))
        ragged = make["d2s"]()
        ragged.ragged_train = True
        out["ragged_train not a TrainStep"] = _raised(lambda: train_one_epoch(args, ragged, None, [], object()))
    return out


def _config():
    from d2s import ops
    from d2s.engine import TrainStep, checkpoint_config
    make = _students()
    args = types.SimpleNamespace(mask_loss_type="kl_div")
    out = {}
    with ops.gemm_mode(ops.GEMM_EXACT):
        for fam in METHODS:
            cfg = TrainStep.config(types.SimpleNamespace(student=make[fam](), args=args))
            out[fam] = [[k, v] for k, v in cfg.items()]
        cfg = TrainStep.config(types.SimpleNamespace(student=make["ltp"](), args=types.SimpleNamespace(mask_loss_type="kl_div", ltp_lambda=0.3)))
        out["ltp --ltp-lambda 0.3"] = [[k, v] for k, v in cfg.items()]
    out["checkpoint_config({})"] = [[k, v] for k, v in checkpoint_config({}).items()]
    return out


def collect():
    return _plain({"command line": _command_line(), "TrainStep": _train_step(), "config": _config()})


def test_messages_and_key_orders_are_what_was_recorded():
    with open(RECORDED) as f:
        recorded = json.load(f)
    got = collect()
    for part in recorded:
        for key in recorded[part]:
            assert got[part].get(key) == recorded[part][key], f"{part}: {key}"
    assert got == recorded


def test_every_method_and_probe_is_recorded():
    with open(RECORDED) as f:
        recorded = json.load(f)
    assert len(recorded["command line"]) == 1 + len(METHODS) * len(PROBES)
    assert all(v is not None for v in recorded["TrainStep"].values())          # every probe of the constructor is a refusal
    assert [k for k, _ in recorded["config"]["d2s"]][-1] == "squeeze_dropped"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        raise SystemExit("usage: python -m tests.test_methods_cpu --write PATH")
    with open(sys.argv[2], "w") as f:
        json.dump(collect(), f, indent=1, sort_keys=False)
        f.write("\n")
