"""The yardsticks of tests/test_attention_bf16_dense_gpu.py checked on their own, without a GPU: every case's input conditions, the bounds,
the float64 reference against the closed form the kernels evaluate, and the rounding emulation against the bounds - the evidence that the
reference and the roundings alone stay inside the bounds before any kernel is involved."""
import pytest
import torch

from tests import attention_bf16_ref as AR


@pytest.mark.parametrize("B,H,n", AR.SHAPES)
@pytest.mark.parametrize("kind", AR.KINDS)
def test_reference_bounds_and_emulation(B, H, n, kind):
    ref = AR.reference(B, H, n, kind)                       # asserts the argmax conditions and max |S| < 30
    arg = ref["S"].argmax(dim=-1)
    if kind == "sink":
        assert bool((arg == 0).all())
    if kind == "last":
        assert bool((arg == n - 1).all())
    assert ref["smax"] < 30.0
    qkv, dout = AR.inputs(B, H, n, kind)
    assert torch.equal(qkv, qkv.bfloat16().float()) and qkv.shape == (B * n, 3 * H * 64) and dout.shape == (B * n, H * 64)
    for name in AR.OUTPUTS:
        b = ref[name + "_bound"]
        assert b.shape == ref[name].shape and bool(torch.isfinite(b).all()) and float(b.min()) > 0.0, name
    cf = AR.closed_form(B, H, n, kind)
    for name in ("dq", "dk", "dv"):
        assert float((cf[name] - ref[name]).abs().max()) <= 1e-12, name
    emu = AR.emulate(B, H, n, kind)
    fracs = AR.bound_fractions(emu, ref)
    print(f"emulation B{B} H{H} n{n} {kind}: max |S| {ref['smax']:.1f}; max err / bound " + " ".join(f"{k} {v:.3f}" for k, v in fracs.items()))
    for k, v in fracs.items():
        assert v <= 1.0, (k, v)


def test_emulation_rounds_and_the_reference_does_not():
    """the emulation's error is a bf16 rounding's, not zero and not the reference itself; rb() rounds ties to even"""
    B, H, n, kind = 2, 2, 33, "normal"
    ref, emu = AR.reference(B, H, n, kind), AR.emulate(B, H, n, kind)
    for name in AR.L2_OUTPUTS:
        err, norm = AR.l2_errors(emu, ref, name)
        rel = err / norm
        assert 2.0 ** -15 < float(rel.min()) and float(rel.max()) < 2.0 ** -5, (name, rel)      # one rounding is <= 2^-8; 33 keys average it, three stack
    for name in ("lse", "cls_row"):                         # no bf16 rounding enters these
        assert float((emu[name] - ref[name]).abs().max()) <= 1e-13
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    assert AR.rb(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
