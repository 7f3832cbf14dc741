"""A-ViT baseline (Yin et al. 2022; DESIGN.md section 25 - the build's own definition, no counterpart in the reference): the dense DeiT
trunk in which every token decides its own depth.  After every block a token adds sigmoid(gate_scale * channel 0 - gate_center) to its
cumulative halting score and halts once that exceeds 1 - eps_halt; halted tokens leave the ragged packed batch before the next block, in
training as at inference.  No predictor and no new parameter: the model has the teacher's state-dict keys and loads any DeiT checkpoint.
The head reads the CLS token's halting-weighted mean over the layers it lived through."""
import torch

from d2s import functional_ats as AF
from d2s import functional_avit as VF
from d2s import ops
from .dynamic_vit import VisionTransformerTeacher, _GEOM, _load_local


class VisionTransformerAViT(VisionTransformerTeacher):
    """forward returns the logits, in train() and eval() mode through the same ragged forward (eval keeps nothing for a backward).
    Afterwards: tokens_per_layer - [L] ints, the rows of the packed batch block l ran on; tokens_per_layer_counts - [L, B] int32 (host),
    the same per image (a finished image goes on as its dead CLS row and counts 1); halt_layer - [B, N] int32 on the device, the layer
    every token halted at (N counts CLS); avg_depth - 0-d device tensor, the mean of halt_layer; ponder_loss, prior_loss - the two penalty
    terms of AViTLoss (0-d, differentiable in training), which target_depth shapes; avit_run - the d2s.functional_avit.AViTRun.
    train_bf16: the training forward also runs in the bf16 arithmetic mode - every block on the bf16 data path (_Ragged(bf16=True)), every
    boundary's backward handing on the bf16 form of its gradient (AViTRun(bf16=True)).  Under an fp32 mode the keyword changes nothing;
    without it the bf16 mode is refused by the ragged block as before."""

    def __init__(self, *args, gate_scale=10.0, gate_center=30.0, eps_halt=0.01, target_depth=7.0, train_bf16=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.gate_scale, self.gate_center, self.eps_halt = float(gate_scale), float(gate_center), float(eps_halt)
        self.target_depth = float(target_depth)
        self.train_bf16 = bool(train_bf16)
        if not 0.0 < self.eps_halt < 1.0:
            raise ValueError(f"eps_halt: a value in (0, 1), got {eps_halt!r}")
        if len(self.blocks) > 64:
            raise ValueError(f"depth {len(self.blocks)}: the penalty kernels hold at most 64 layers")
        if float(getattr(self, "drop_path_rate", 0.0)) > 0.0:
            raise ValueError("drop_path_rate > 0: stochastic depth is not built for a ragged block")
        self.grad_ready_hook = None          # set by a data-parallel TrainStep: called with i when block i's input gradient exists
        self._tgt = None
        self._reset_records()

    def _reset_records(self):
        self.tokens_per_layer, self.tokens_per_layer_counts = [], None
        self.halt_layer = self.avg_depth = self.ponder_loss = self.prior_loss = self.avit_run = None

    def _target(self, device):
        if self._tgt is None or self._tgt.device != device or self._tgt_depth != self.target_depth:
            self._tgt = VF.target_distribution(len(self.blocks), self.target_depth).to(device)
            self._tgt_depth = self.target_depth
        return self._tgt

    def forward(self, x):
        self._reset_records()
        train = self.training and torch.is_grad_enabled()
        x = self._embed(x)
        B, n, D = x.shape
        L = len(self.blocks)
        bf16 = train and self.train_bf16 and ops.get_gemm_mode() == ops.GEMM_BF16
        run = VF.AViTRun(B, n, D, L, self.gate_scale, self.gate_center, self.eps_halt, x.device, **(dict(bf16=True) if bf16 else {}))
        x = x.contiguous().view(B * n, D)
        for i, blk in enumerate(self.blocks):
            a = blk.attn
            if train:
                if self.grad_ready_hook is not None and x.requires_grad:
                    x.register_hook(lambda g, i=i, cb=self.grad_ready_hook: (cb(i), None)[1])
                x = AF.ragged_block_train(x, blk._params(), blk.norm1.eps,
                                          AF._Ragged(run.cu, B, run.max_n, a.num_heads, a.scale, **(dict(bf16=True) if bf16 else {})))
            else:
                x = blk.forward_ragged(x, run.cu, B, run.max_n)
            x = VF.halt(x, run, i + 1)
        acc, part = x
        pen = VF.penalties(part, self._target(acc.device), run)
        self.avit_run = run
        self.ponder_loss, self.prior_loss = pen[0], pen[1]
        self.halt_layer = run.st["nh"]
        self.avg_depth = run.st["nh"].float().mean()
        self.tokens_per_layer = [sum(r) for r in run.rows_per_layer]
        self.tokens_per_layer_counts = torch.tensor(run.rows_per_layer, dtype=torch.int32)
        return self._head(acc.view(B, 1, D))[0]


def _avit(size, checkpoint_path=None, **kwargs):
    model = VisionTransformerAViT(patch_size=16, depth=12, mlp_ratio=4, qkv_bias=True, **_GEOM[size], **kwargs)
    return _load_local(model, checkpoint_path, strict=True)


def avit_deit_tiny_patch16_224(checkpoint_path=None, **kwargs):
    return _avit("tiny", checkpoint_path, **kwargs)


def avit_deit_small_patch16_224(checkpoint_path=None, **kwargs):
    return _avit("small", checkpoint_path, **kwargs)


def avit_deit_base_patch16_224(checkpoint_path=None, **kwargs):
    return _avit("base", checkpoint_path, **kwargs)
