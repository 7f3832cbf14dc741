"""The student families of --method, one record each: what d2s.engine.TrainStep, train.py, evaluate.py, mask_predictor.py and
utils.parse_args have to know about a family beyond its model class (vit_models/) and its kernels (d2s/functional_*.py).  A record holds
what the families differ in - names, the fragments of the refusal texts, the loss, the flags, the checkpoint config, the evaluation's
extra metrics; whatever only one family does stays spelled out where it happens."""
from typing import Callable, NamedTuple, Optional

from losses import DynamicViTLoss, ToMeLoss, AViTLoss, LTPLoss


class Method(NamedTuple):
    name: str                                   # --method NAME
    cls: str                                    # type(student).__name__
    article: str = ""                           # student = "<article> <title> student"
    title: str = ""
    logits_only: bool = False                   # the training forward returns logits alone: one loss, the teacher optional, no warm-up epochs
    prefix: Optional[str] = None                # factories vit_models.<prefix>_<arch>_patch16_224, arch = deit_{tiny, small, base}
    has_none: str = ""                          # "... the warm-up epochs train the score predictors only, and <has_none>"
    no_predictor: str = ""                      # load_trunk: why a checkpoint's predictor tensors are ignored
    block: str = ""                             # "stochastic depth is not built for <block>"
    no_graph: Optional[str] = None              # why TrainStep(graph=True) is refused; None: the step may be captured
    opt_in: Optional[tuple] = None              # (model attribute, student -> is it needed, the refusal after "TrainStep with ")
    bf16_refusal: Optional[Callable] = None     # () -> why TrainStep refuses the bf16 arithmetic mode
    cli: str = ""                               # the subject of the command line's refusals
    cli_bf16: Optional[tuple] = None            # --gemm-mode bf16: (why not, does --eval-only run in it all the same)
    cli_selection: str = ""                     # why the d2s selection flags have no meaning
    optim_noun: str = ""                        # "--torch-optim (<optim_noun> trains through the fused step only)"
    loss: Optional[Callable] = None             # args -> the loss module (d2s: MaskLoss and BackboneLoss, built where they are used)
    loss_extras: Callable = lambda s: ()        # student -> the loss's positional arguments after metrics
    token_record: str = "tokens_per_block"      # the model attribute that holds the last forward's token counts
    flags: tuple = ()                           # the flags only this family takes: (attr, flag, default); parse_args leaves them None
    config_keys: tuple = ()                     # checkpoint config: None for every other family
    config: Optional[Callable] = None           # (student, args) -> the values of config_keys
    eval_extras: tuple = ()                     # evaluation: (model attribute, metric key), a mean over the batches

    @property
    def student(self):
        return f"{self.article} {self.title} student"

    def factory(self, arch):
        return f"{self.prefix}_{arch}_patch16_224"


def flag_values(m, args):
    """{attr: value} of the family's own flags, the default where args has none."""
    return {attr: default if getattr(args, attr, None) is None else getattr(args, attr) for attr, _, default in m.flags}


def _ltp_bf16_refusal():
    from d2s.functional_ltp import BF16_REFUSAL
    return BF16_REFUSAL


D2S = Method("d2s", "VisionTransformerDiffPruning")
# the three numbers of ltp are this build's guesses: no trained checkpoint exists here to tune them on
METHODS = (
    D2S,
    Method("dynamicvit", "DefaultVisionTransformerDiffPruning", loss=DynamicViTLoss),
    Method("tome", "VisionTransformerToMe", "a", "Token Merging", True, "tome",
           has_none="token merging has none", no_predictor="token merging has no predictor", block="a merging block",
           no_graph="a captured merging step is not built",
           opt_in=("train_merge", lambda s: any(v > 0 for v in s.tome_r),
                   "a merging VisionTransformerToMe needs train_merge=True (training through the merge is opt-in)"),
           cli="--tome-train", optim_noun="a merging student", loss=ToMeLoss),
    Method("ats", "VisionTransformerATS", "an", "Adaptive Token Sampling", True, "ats",
           has_none="a sampling stage has none", no_predictor="adaptive token sampling has no predictor", block="a ragged block",
           no_graph="every stage reads its row count on the host, which a captured step cannot",
           opt_in=("train_sample", lambda s: True,
                   "a sampling VisionTransformerATS needs train_sample=True (training through the stages is opt-in)"),
           cli="--ats-train", cli_bf16=("training through a sampling stage is built on the fp32 data path; exact and split run", False),
           cli_selection="a sampling stage scores tokens by the block's own CLS attention and value norms and keeps a count of its own",
           optim_noun="a sampling student", loss=ToMeLoss, token_record="tokens_per_stage"),
    Method("avit", "VisionTransformerAViT", "an", "A-ViT", True, "avit",
           has_none="adaptive depth has none", no_predictor="adaptive depth has no predictor", block="a ragged block",
           no_graph="every block reads its row counts on the host, which a captured step cannot",
           cli="--method avit", cli_bf16=("training through a ragged block is built on the fp32 data path; exact and split run, "
                                          "--eval-only runs in all three", True),
           cli_selection="every token halts by its own cumulative score: there is no selection stage",
           optim_noun="an adaptive-depth student", loss=AViTLoss, loss_extras=lambda s: (s.ponder_loss, s.prior_loss, s.avg_depth),
           token_record="tokens_per_layer",
           flags=(("avit_gate_scale", "--avit-gate-scale", 10.0), ("avit_gate_center", "--avit-gate-center", 30.0),
                  ("avit_ponder_scale", "--avit-ponder-scale", 5e-4), ("avit_prior_alpha", "--avit-prior-alpha", 0.01),
                  ("avit_target_depth", "--avit-target-depth", 7.0)),
           config_keys=("avit_gate_scale", "avit_gate_center", "avit_eps_halt"),
           config=lambda s, args: (float(s.gate_scale), float(s.gate_center), float(s.eps_halt)),
           eval_extras=(("avg_depth", "val_avg_depth"),)),
    Method("evo", "VisionTransformerEvo", "an", "Evo-ViT", True, "evo",
           has_none="the slow-fast update has none", no_predictor="the slow-fast update has no predictor", block="a slow-fast block",
           cli="--method evo", cli_selection="the slow-fast update ranks tokens by its own global score: there is no selection stage",
           optim_noun="a slow-fast student", loss=ToMeLoss,
           flags=(("evo_start", "--evo-start", 4), ("evo_keep", "--evo-keep", 0.5), ("evo_tradeoff", "--evo-tradeoff", 0.5)),
           config_keys=("evo_start", "evo_keep", "evo_tradeoff"),
           config=lambda s, args: (int(s.evo_start), float(s.evo_keep), float(s.evo_tradeoff))),
    Method("ltp", "VisionTransformerLTP", "an", "LTP", True, "ltp",
           has_none="learned thresholds have none", no_predictor="learned thresholds have no predictor",
           block="a ragged block or a block with a learnt policy",
           no_graph="a hard stage reads its row counts on the host, which a captured step cannot, and a captured soft step is not built",
           bf16_refusal=_ltp_bf16_refusal,
           cli="--method ltp", cli_bf16=("the score is recomputed from the fp32 attention's log-sum-exp, and both phases train on the fp32 "
                                         "data path; exact and split run", False),
           cli_selection="a token stays while the attention it receives reaches its block's learned threshold: there is no other "
                         "selection stage",
           optim_noun="a learned-threshold student", loss=LTPLoss, loss_extras=lambda s: (s.ltp_reg, s.avg_tokens),
           flags=(("ltp_phase", "--ltp-phase", "soft"), ("ltp_temperature", "--ltp-temperature", 1e-3), ("ltp_lambda", "--ltp-lambda", 0.01),
                  ("ltp_init_threshold", "--ltp-init-threshold", 0.005)),
           config_keys=("ltp_phase", "ltp_temperature", "ltp_lambda", "ltp_init_threshold"),
           config=lambda s, args: (str(s.ltp_phase), float(s.ltp_temperature), float(flag_values(by_name("ltp"), args)["ltp_lambda"]),
                                   float(s.ltp_init_threshold)),
           eval_extras=(("avg_tokens", "val_avg_tokens"),)),
)
_BY_NAME = {m.name: m for m in METHODS}
_BY_CLASS = {m.cls: m for m in METHODS}


def by_name(cli_name):
    return _BY_NAME[cli_name]


def of(student):
    """The family a student trains as, by its class name; any other class takes the dense-to-sparse route, and so does an ATS model
    without stages: it is the dense trunk."""
    m = _BY_CLASS.get(type(student).__name__, D2S)
    if m.name == "ats" and not len(getattr(student, "ats_locs", [])) > 0:
        return D2S
    return m


def eval_returns_logits_alone(model):
    """In eval mode the six baseline classes return logits alone, whatever they train as; the dense-to-sparse student returns its tuple."""
    return _BY_CLASS.get(type(model).__name__, D2S) is not D2S
