"""CPU tier of the save / resume / evaluate feature: the new command-line flags and their refusals, the atomic file write, the documented
checkpoint layout through torch.save -> torch.load(weights_only=True), and the C-ABI entry of the AdamW + EMA launch."""
import ctypes
import os

import pytest
import torch

from tests import cases


def test_new_flags_parse_with_their_defaults():
    import utils
    a = utils.parse_args([])
    assert a.output_dir is None and a.save_every == 1 and a.resume is None and a.eval_only is False
    assert a.model_ema is False and a.model_ema_decay == 0.99996
    a = utils.parse_args(["--output-dir", "out", "--save-every", "3", "--resume", "out/last.pt", "--eval-only", "--model-ema",
                          "--model-ema-decay", "0.9"])
    assert (a.output_dir, a.save_every, a.resume, a.eval_only, a.model_ema, a.model_ema_decay) == ("out", 3, "out/last.pt", True, True, 0.9)


@pytest.mark.parametrize("extra,flag", [
    (["--resume", "x.pt", "--torch-optim"], "--resume"),
    (["--model-ema", "--torch-optim"], "--model-ema"),
    (["--eval-only"], "--eval-only"),
    (["--save-every", "0"], "--save-every"),
    (["--model-ema", "--model-ema-decay", "1.0"], "--model-ema-decay"),
])
def test_check_supported_refuses(extra, flag):
    import mask_predictor
    import utils
    with pytest.raises(SystemExit, match="not on the accelerated path") as e:
        mask_predictor.check_supported(utils.parse_args(extra))
    assert flag in str(e.value)


def test_check_supported_accepts_the_new_flags(capsys):
    import mask_predictor
    import utils
    mask_predictor.check_supported(utils.parse_args(["--output-dir", "out", "--model-ema", "--resume", "out/last.pt"]))
    mask_predictor.check_supported(utils.parse_args(["--eval-only", "--student-checkpoint", "w.pt"]))
    mask_predictor.check_supported(utils.parse_args(["--eval-only", "--student-checkpoint", "w.pt", "--torch-optim"]))
    capsys.readouterr()
    mask_predictor.check_supported(utils.parse_args(["--output-dir", "out", "--torch-optim"]))      # allowed, and says what it saves
    assert "weights only" in capsys.readouterr().out


def test_atomic_save_keeps_the_old_file_when_the_writer_dies(tmp_path):
    import utils
    final = tmp_path / "last.pt"
    utils.atomic_save({"epoch": 0, "w": torch.arange(1000.)}, str(final))
    before = final.read_bytes()
    assert torch.load(str(final), weights_only=True)["epoch"] == 0

    def dies_halfway(obj, f):
        f.write(b"half a file")
        f.flush()
        raise RuntimeError("killed")

    with pytest.raises(RuntimeError, match="killed"):
        utils.atomic_save({"epoch": 1}, str(final), writer=dies_halfway)
    assert final.read_bytes() == before, "the file under the final name changed"
    assert sorted(os.listdir(tmp_path)) == ["last.pt"], "a temporary file was left behind"
    # no earlier file: a writer that dies must not create the final name at all
    with pytest.raises(RuntimeError, match="killed"):
        utils.atomic_save({"epoch": 1}, str(tmp_path / "best.pt"), writer=dies_halfway)
    assert sorted(os.listdir(tmp_path)) == ["last.pt"]
    utils.atomic_save({"epoch": 2}, str(final))                                                     # and a good write replaces it
    assert torch.load(str(final), weights_only=True)["epoch"] == 2 and sorted(os.listdir(tmp_path)) == ["last.pt"]


def test_documented_layout_survives_a_weights_only_round_trip(tmp_path):
    """A hand-built dict in the layout of TrainStep.state_dict(): tensors, numbers, strings, lists and nested
    dicts only, so torch.load(weights_only=True) - which executes nothing from the file - reads it back unchanged."""
    import utils
    g = torch.Generator().manual_seed(0)
    model = {"cls_token": torch.randn(1, 1, 8, generator=g), "blocks.0.attn.qkv.weight": torch.randn(24, 8, generator=g),
             "score_predictor.0.in_conv.0.bn.num_batches_tracked": torch.tensor(3)}
    names = [k for k in model if "num_batches" not in k]
    sd = {
        "model": model,
        "optimizer": {"state": {n: {"exp_avg": torch.randn_like(model[n]), "exp_avg_sq": torch.rand_like(model[n]), "step": i}
                                for i, n in enumerate(names)},
                      "betas": [0.9, 0.999], "eps": 1e-8, "steps": 4},
        "model_ema": {k: v.clone() for k, v in model.items()},
        "ema_decay": 0.99996,
        "epoch": 1,
        "best_acc": 0.25,
        "rng": {"cpu": torch.get_rng_state(), "device": torch.zeros(16, dtype=torch.uint8)},
        "config": {"format": 1, "model": "VisionTransformerDiffPruning", "embed_dim": 8, "depth": 1, "num_heads": 1, "num_classes": 10,
                   "img_size": [64, 64], "patch_size": [16, 16], "pruning_loc": [3], "token_ratio": [0.5], "init_n": 196,
                   "topk_selection": True, "small_predictor": False, "predictor_bn": True, "mask_loss_type": "kl_div",
                   "patch_score_threshold": None, "gemm_mode": 0},
    }
    path = str(tmp_path / "last.pt")
    utils.atomic_save(sd, path)
    back = torch.load(path, map_location="cpu", weights_only=True)

    def same(a, b, where):
        assert type(a) is type(b), where
        if isinstance(a, dict):
            assert list(a) == list(b), where
            for k in a:
                same(a[k], b[k], f"{where}.{k}")
        elif torch.is_tensor(a):
            assert a.dtype == b.dtype and torch.equal(a, b), where
        else:
            assert a == b, where
    same(sd, back, "sd")
    # the same file is what --student-checkpoint reads: checkpoint_filter_fn unwraps 'model'
    import vit_models
    stub = torch.nn.Module()
    stub.patch_embed = torch.nn.Module()
    stub.patch_embed.proj = torch.nn.Conv2d(3, 8, 16, 16)
    stub.pos_embed = torch.nn.Parameter(torch.zeros(1, 17, 8))
    assert list(vit_models.checkpoint_filter_fn(back, stub)) == list(model)


def test_library_exports_the_ema_entry_with_the_declared_signature():
    from d2s import lib
    header = open(os.path.join(cases.REPO, "include", "d2s_hip.h")).read()
    assert "int d2s_adamw_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* chunk_desc, int n_chunks," in header
    assert "float grad_scale, int* chunk_steps, float* ema, float ema_decay," in header
    handle = lib.load()
    fn = handle.d2s_adamw_step_ema
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    # params grads exp_avg exp_avg_sq desc | n_chunks | beta1 beta2 eps | step | grad_scale | chunk_steps ema | ema_decay | stream
    assert fn.argtypes == [P, P, P, P, P, I, F, F, F, I, F, P, P, F, P] and fn.restype is I
    assert handle.d2s_adamw_step.argtypes == [P, P, P, P, P, I, F, F, F, I, F, P, P], "the plain entry keeps its signature"
    # argument checks come before any launch, so they run without a device: null arenas, then a decay outside [0, 1)
    assert fn(None, None, None, None, None, 1, 0.9, 0.999, 1e-8, 1, 1.0, None, None, 0.9, None) != 0
    a, e = ctypes.c_void_p(4096), ctypes.c_void_p(8192)       # never dereferenced: every call below is refused on its arguments
    for decay in (1.0, -0.1, 1.5, float("nan")):
        assert fn(a, a, a, a, a, 1, 0.9, 0.999, 1e-8, 1, 1.0, None, e, decay, None) != 0, decay
    assert fn(a, a, a, a, a, 1, 0.9, 0.999, 1e-8, 1, 1.0, None, a, 0.9, None) != 0, "ema must not be the parameter arena itself"
