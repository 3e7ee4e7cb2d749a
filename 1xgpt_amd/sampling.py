"""The sampling law of the MaskGIT decoder: logit temperature, top-k, top-p, and the "confidence" unmasking mode's
choice temperature (genie_sampling in include/genie_hip.h, which states the semantics).

A departure from the reference: its ``temperature`` only switches arg-max to sampling (st_mask_git.py:184-186 builds
``Categorical(probs=probs / temperature)``, which renormalises) and it has no filter.  ``sampling=None`` everywhere means the
reference's behaviour, bit for bit.
"""
import math
from dataclasses import dataclass

UNMASK_MODES = ("random", "greedy", "confidence")


@dataclass
class SamplingConfig:
    logit_temperature: float = 1.0   # tau > 0: z = logit / tau (1 = off)
    top_k: int = 0                   # keep the k best entries of each factored vocabulary (0 = off)
    top_p: float = 1.0               # ... then the smallest prefix of them whose mass reaches top_p (>= 1 or <= 0 = off)
    choice_temperature: float = 4.5  # c >= 0 of unmask_mode="confidence": key = log(conf) + c * (1 - (step+1)/steps) * gumbel

    def __post_init__(self):
        self.validate()

    def validate(self):
        tau, k, p, c = self.logit_temperature, self.top_k, self.top_p, self.choice_temperature
        if isinstance(k, bool) or int(k) != k:
            raise ValueError(f"top_k must be an integer, got {k!r}")
        if not (isinstance(tau, (int, float)) and math.isfinite(tau) and tau > 0):
            raise ValueError(f"logit_temperature must be positive and finite, got {tau!r}")
        if k < 0:
            raise ValueError(f"top_k must be >= 0, got {k!r}")
        if not isinstance(p, (int, float)) or math.isnan(p):
            raise ValueError(f"top_p must be a number, got {p!r}")
        if not (isinstance(c, (int, float)) and c >= 0):
            raise ValueError(f"choice_temperature must be >= 0, got {c!r}")
        return self

    def is_neutral(self, factored_vocab_size=None):
        """True when the law filters and tempers nothing (the library then runs the reference's kernels)."""
        k_off = self.top_k == 0 or (factored_vocab_size is not None and self.top_k >= factored_vocab_size)
        return self.logit_temperature == 1.0 and k_off and not (0.0 < self.top_p < 1.0)

    def to_struct(self):
        """The ctypes genie_sampling of this law."""
        from . import _lib
        self.validate()
        return _lib.Sampling(logit_temperature=float(self.logit_temperature), top_k=int(self.top_k), top_p=float(self.top_p),
                             choice_temperature=float(self.choice_temperature))

    @classmethod
    def from_args(cls, args):
        """From an argparse / SimpleNamespace carrying any of the four fields (missing ones take the defaults); None when the
        namespace names none of them."""
        names = ("logit_temperature", "top_k", "top_p", "choice_temperature")
        given = {n: getattr(args, n) for n in names if getattr(args, n, None) is not None}
        return cls(**given) if given else None


class _ModelNull:
    """Default of Guidance.null_action: "the model's own null row" (a model conditioned on action vectors has exactly one)."""

    def __repr__(self):
        return "MODEL_NULL"


MODEL_NULL = _ModelNull()


@dataclass
class Guidance:
    """Classifier-free guidance of an action-conditioned model (genie_guidance in include/genie_hip.h, which states the arithmetic):
    logits = scale * conditional + (1 - scale) * null, the null stream being the same tokens under ``null_action`` at every frame."""
    scale: float          # w, finite: 1 = plain conditional sampling, 0 = the null stream alone, > 1 = guidance
    # row of the action table that stands for "no action" (learned through action dropout: data.maskgit_collate).  A model with
    # config.action_dim > 0 (continuous actions) supplies the index of its learned null row itself: Guidance(scale) is enough there.
    null_action: int = MODEL_NULL

    def __post_init__(self):
        self.validate()

    def validate(self, action_vocab_size=None):
        w, a = self.scale, self.null_action
        if isinstance(w, bool) or not (isinstance(w, (int, float)) and math.isfinite(w)):
            raise ValueError(f"guidance scale must be a finite number, got {w!r}")
        if a is not MODEL_NULL and (isinstance(a, bool) or not isinstance(a, int) or a < 0):
            raise ValueError(f"null_action must be a non-negative integer, got {a!r}")
        if action_vocab_size is not None:
            if not action_vocab_size:
                raise ValueError("guidance given to a model without actions (config.action_vocab_size == 0)")
            if a is MODEL_NULL:
                raise ValueError("guidance of a model conditioned on action ids needs null_action (the table row trained as 'no action')")
            if a >= action_vocab_size:
                raise IndexError(f"null_action {a} out of range [0, {action_vocab_size})")
        return self

    def to_struct(self):
        """The ctypes genie_guidance."""
        from . import _lib
        self.validate()
        if self.null_action is MODEL_NULL:
            raise ValueError("Guidance without null_action has no struct of its own: the model supplies the row (guidance_struct)")
        return _lib.Guidance(scale=float(self.scale), null_action=int(self.null_action))

    @classmethod
    def from_args(cls, args):
        """From a namespace carrying guidance_scale / null_action; None when guidance_scale is absent or None."""
        w = getattr(args, "guidance_scale", None)
        if w is None:
            return None
        a = getattr(args, "null_action", None)
        if a is None:
            raise ValueError("--guidance_scale needs --null_action (the action-table row trained as 'no action')")
        return cls(float(w), int(a))


def guidance_struct(guidance, action_vocab_size=None, null_row=None):
    """None -> None (the unchanged entry points); a Guidance -> its genie_guidance, checked against the model's action table
    (scale 1 -> None as well, once checked: the library would dispatch to the unguided entry point anyway).
    null_row: the fixed index of the learned null row in the per-call row table of a model conditioned on action vectors
    (config.action_dim > 0); the Guidance then needs no null_action, and one that names another row is refused."""
    if guidance is None:
        return None
    if not isinstance(guidance, Guidance):
        raise ValueError(f"guidance must be a Guidance or None, got {type(guidance).__name__}")
    if null_row is not None:
        from . import _lib
        guidance.validate()
        if guidance.null_action is not MODEL_NULL and guidance.null_action != null_row:
            raise ValueError(f"this model is conditioned on action vectors: its null row is row {null_row} of the per-call table, "
                             f"not null_action={guidance.null_action} (pass Guidance(scale))")
        return None if float(guidance.scale) == 1.0 else _lib.Guidance(scale=float(guidance.scale), null_action=int(null_row))
    guidance.validate(action_vocab_size)
    if float(guidance.scale) == 1.0:   # g = c: the unguided entry points, sizes and launches
        return None
    return guidance.to_struct()


def add_guidance_arguments(parser):
    """--guidance_scale / --null_action for tools/generate.py and tools/bench_generate.py."""
    parser.add_argument("--guidance_scale", type=float, default=None,
                        help="Classifier-free guidance scale w of an action-conditioned model: logits = w * conditional + (1 - w) * null "
                             "(1 = off, > 1 pushes away from the null-action stream). Needs --null_action.")
    parser.add_argument("--null_action", type=int, default=None,
                        help="Row of the action table trained as 'no action' (tools/train.py --action_dropout --null_action).")
    return parser


def as_struct(sampling):
    """None -> None (the unchanged entry points); a SamplingConfig -> its genie_sampling."""
    if sampling is None:
        return None
    if not isinstance(sampling, SamplingConfig):
        raise ValueError(f"sampling must be a SamplingConfig or None, got {type(sampling).__name__}")
    return sampling.to_struct()


def unmask_code(unmask_mode):
    from . import _lib
    if unmask_mode not in UNMASK_MODES:
        raise NotImplementedError(f"Expected `unmask_mode` to be one of ['greedy', 'random', 'confidence'], got {unmask_mode}")
    return {"random": _lib.UNMASK_RANDOM, "greedy": _lib.UNMASK_GREEDY, "confidence": _lib.UNMASK_CONFIDENCE}[unmask_mode]


def add_cli_arguments(parser):
    """--logit_temperature / --top_k / --top_p / --unmask_mode / --choice_temperature for tools/generate.py and tools/evaluate.py."""
    parser.add_argument("--logit_temperature", type=float, default=None,
                        help="Divide the logits by this before the softmax (> 0). This is the flag that tempers; "
                             "--temperature is the reference's switch between arg-max and sampling and does not.")
    parser.add_argument("--top_k", type=int, default=None, help="Sample among the k most likely entries of each factored vocabulary.")
    parser.add_argument("--top_p", type=float, default=None,
                        help="Nucleus sampling: the smallest set of most likely entries whose mass reaches this.")
    parser.add_argument("--unmask_mode", default="random", choices=list(UNMASK_MODES),
                        help="Which tokens a MaskGIT step re-masks: random draws, lowest confidence (greedy), or confidence plus "
                             "annealed Gumbel noise (confidence).")
    parser.add_argument("--choice_temperature", type=float, default=None,
                        help="Scale of the annealed Gumbel noise of --unmask_mode confidence (default 4.5).")
    return parser
