"""bench.py --dump-outputs (what the timed path returned, as .npy files two builds can be compared by) and the options that need --full.
CPU only: the dump helper is fed host tensors shaped like a train step's outputs."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases

BENCH = os.path.join(cases.REPO, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _info(g):
    return dict(loss=torch.tensor(1.25), logits_s=torch.randn(4, 10, generator=g, requires_grad=True),
                kept=[torch.randint(0, 196, (4, 98), generator=g)], pred_logits=[torch.randn(4, 196, 2, generator=g).bfloat16()],
                token_t=torch.randn(3, 197, 2000, generator=g), note="not a tensor")


def test_dump_outputs_is_deterministic_typed_and_sampled(tmp_path):
    bench = _bench()
    n = bench.DUMP_SAMPLE
    info, params = _info(torch.Generator().manual_seed(3)), torch.randn(2 * n + 7, generator=torch.Generator().manual_seed(4))
    total = bench.dump_outputs(str(tmp_path / "a"), info, params)
    bench.dump_outputs(str(tmp_path / "b"), info, params.clone())
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["kept_0.npy", "logits_s.npy", "loss.npy", "pred_logits_0.npy", "student_params.npy",
                                                           "token_t.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for k, v in got.items():
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / f"{k}.npy"), err_msg=k)
    assert total == sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES
    assert got["kept_0"].dtype == np.float64 and np.array_equal(got["kept_0"], info["kept"][0].numpy())
    assert got["logits_s"].dtype == np.float32 and np.array_equal(got["logits_s"], info["logits_s"].detach().numpy())
    assert got["pred_logits_0"].dtype == np.float32 and got["pred_logits_0"].shape == (4, 196, 2) and float(got["loss"]) == 1.25
    # outputs above DUMP_SAMPLE elements: a sample of exactly that size, every value taken from the output itself
    for k, src in (("token_t", info["token_t"]), ("student_params", params)):
        assert got[k].shape == (n,) and got[k].dtype == np.float32
        assert np.isin(got[k], src.reshape(-1).numpy()).all(), k


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    bench = _bench()
    big = [torch.zeros(bench.DUMP_SAMPLE + 1) for _ in range(bench.DUMP_MAX_BYTES // (4 * bench.DUMP_SAMPLE) + 1)]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "d"), dict(many=big), torch.zeros(1))
    assert not (tmp_path / "d").exists()


@pytest.mark.parametrize("flag", [["--gemm-shapes-out", "shapes.txt"], ["--time-kernels-in-region"]])
def test_per_kernel_options_need_full(flag):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + flag, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--full" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
