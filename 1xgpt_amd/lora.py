"""LoRA adapters on the attention, MLP and readout Linears (include/genie_hip.h, "LoRA adapters"; Hu et al. 2021).

An adapted Linear keeps its base weight W0 and gains A (rank, in) and B (out, rank); everything that computes -- training step, inference,
generation -- runs on the effective weight W = W0 + (alpha / rank) B A, merged by genie_lora_merge.  What is here is shared by the trainer
(1xgpt_amd/train.py: the adapters live in its flat buffers, dW of the untouched step is projected onto them by genie_lora_project) and by
the model (STMaskGIT.load_adapter: the in-place merge): the settings, target selection, the initial draw, the item tables of the two
library calls and the adapter files.  No model math: there is no CPU fallback for the kernels.
"""
import fnmatch
import json
import math
import os
import zlib
from dataclasses import dataclass

import numpy as np

from . import _lib

SUFFIX_A, SUFFIX_B = ".lora_A", ".lora_B"
LINEAR_WEIGHTS = ("spatial_attn.qkv", "spatial_attn.proj", "temporal_attn.qkv", "temporal_attn.proj", "mlp.fc1", "mlp.fc2")
# the fields of the base model's config that fix the shapes of its Linears: an adapter is refused on a base that differs in one
BASE_FIELDS = ("num_layers", "d_model", "num_heads", "mlp_ratio", "factored_vocab_size", "num_factored_vocabs")


def linear_weight_names(config):
    """The nn.Linear weights an adapter may target: six per layer and the readout."""
    out = [f"decoder.layers.{i}.{n}.weight" for i in range(config.num_layers) for n in LINEAR_WEIGHTS]
    return out + ["out_x_proj.weight"]


@dataclass
class LoraConfig:
    """rank: 1 .. 64; alpha: finite, the scale is alpha / rank; targets: fnmatch patterns over `linear_weight_names(config)` (a list or one
    comma-separated string; "decoder.layers.*" = the six Linears of every layer); seed: of the initial draw of A."""
    rank: int = 8
    alpha: float = 16.0
    targets: object = "decoder.layers.*"
    seed: int = 0

    def __post_init__(self):
        if isinstance(self.rank, bool) or not isinstance(self.rank, (int, np.integer)) or not 1 <= int(self.rank) <= _lib.LORA_MAX_RANK:
            raise ValueError(f"LoraConfig.rank must be an integer in 1 .. {_lib.LORA_MAX_RANK}, got {self.rank!r}")
        self.rank = int(self.rank)
        self.alpha = float(self.alpha)
        if not math.isfinite(self.alpha) or abs(self.alpha / self.rank) > float(np.finfo(np.float32).max):   # the library's scale is a float
            raise ValueError(f"LoraConfig.alpha must be finite, got {self.alpha!r}")
        pats = [q for q in self.targets.split(",") if q] if isinstance(self.targets, str) else list(self.targets or ())
        if not pats or not all(isinstance(q, str) for q in pats):
            raise ValueError(f"LoraConfig.targets needs at least one pattern, got {self.targets!r}")
        self.targets = pats
        self.seed = int(self.seed)

    @property
    def scale(self):
        return self.alpha / self.rank


def select_targets(config, patterns):
    """The adapted Linear weight names, in `linear_weight_names` order.  ValueError for a pattern that matches none of them."""
    names = linear_weight_names(config)
    hit = set()
    for p in patterns:
        m = [n for n in names if fnmatch.fnmatchcase(n, p)]
        if not m:
            raise ValueError(f"lora target pattern {p!r} matches no Linear weight (linear_weight_names)")
        hit.update(m)
    return [n for n in names if n in hit]


def adapter_names(weight_name):
    """(<linear>.lora_A, <linear>.lora_B) of <linear>.weight."""
    stem = weight_name[:-len(".weight")]
    return stem + SUFFIX_A, stem + SUFFIX_B


def adapter_shapes(targets, weight_shapes, rank):
    """{adapter tensor name: shape} for the targets, from {weight name: (out, in)}."""
    out = {}
    for n in targets:
        o, i = weight_shapes[n]
        a, b = adapter_names(n)
        out[a], out[b] = (rank, i), (o, rank)
    return out


def draw_a(name, shape, seed):
    """The initial A: U(-1/sqrt(in), 1/sqrt(in)) in f32 from a generator seeded by (seed, tensor name); B starts at zero."""
    rng = np.random.Generator(np.random.PCG64([int(seed) & (2 ** 64 - 1), zlib.crc32(name.encode())]))
    bound = 1.0 / math.sqrt(shape[1])
    return ((rng.random(shape, dtype=np.float64) * 2.0 - 1.0) * bound).astype(np.float32)


def item(scale, out, in_, rank, a, b, w=None, w0=None, dw=None, da=None, db=None):
    """One genie_lora_item from device pointers (integers; None = unused by the call)."""
    return _lib.LoraItem(w=w, w0=w0, a=a, b=b, dw=dw, da=da, db=db, out=out, in_=in_, rank=rank, scale=scale)


def table(items):
    """(ctypes array, n) of a list of LoraItem, at most GENIE_LORA_MAX_ITEMS."""
    assert 1 <= len(items) <= _lib.LORA_MAX_ITEMS, len(items)
    return (_lib.LoraItem * len(items))(*items), len(items)


def chunks(items, n=_lib.LORA_MAX_ITEMS):
    return [items[i:i + n] for i in range(0, len(items), n)]


def merge(lib, items, stream):
    """genie_lora_merge over any number of items, GENIE_LORA_MAX_ITEMS per launch."""
    for part in chunks(items):
        arr, n = table(part)
        _lib.check(lib.genie_lora_merge(arr, n, stream), "genie_lora_merge")


# ------------------------------------------------------------------ adapter files
def base_geometry(config):
    return {k: getattr(config, k) for k in BASE_FIELDS}


def adapter_config(lora, targets, config):
    """What adapter_config.json holds."""
    return {"rank": lora.rank, "alpha": lora.alpha, "targets": list(targets), "base": base_geometry(config)}


def check_adapter(cfg, tensors, config, weight_shapes):
    """(rank, scale, targets) of an adapter (its config dict and {name: tensor with .shape}) for a base model.  ValueError for a base that
    differs in a BASE_FIELDS value, a target that is no Linear of it, a missing or surplus tensor, or a wrong shape."""
    try:
        rank, alpha, targets, base = int(cfg["rank"]), float(cfg["alpha"]), list(cfg["targets"]), dict(cfg["base"])
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"adapter config is incomplete: {e!r}") from None
    lc = LoraConfig(rank=rank, alpha=alpha, targets=targets)
    mine = base_geometry(config)
    diff = {k: (base.get(k), v) for k, v in mine.items() if base.get(k) != v}
    if diff:
        raise ValueError("the adapter was trained on another base model (adapter, this model): "
                         + ", ".join(f"{k}={a}->{b}" for k, (a, b) in diff.items()))
    known = set(linear_weight_names(config))
    bad = [n for n in targets if n not in known]
    if bad or not targets:
        raise ValueError(f"adapter targets {bad} are not Linear weights of this model" if bad else "the adapter has no target")
    want = adapter_shapes(targets, weight_shapes, rank)
    if set(tensors) != set(want):
        raise ValueError(f"adapter tensors do not match its targets: missing {sorted(set(want) - set(tensors))[:4]}, "
                         f"unexpected {sorted(set(tensors) - set(want))[:4]}")
    for n, shp in want.items():
        if tuple(tensors[n].shape) != tuple(shp):
            raise ValueError(f"adapter tensor {n} has shape {tuple(tensors[n].shape)}, this model needs {tuple(shp)}")
    return rank, lc.scale, targets


def save_adapter(save_directory, cfg, tensors):
    """adapter_config.json + adapter.safetensors ({name: torch tensor})."""
    from safetensors.torch import save_file
    os.makedirs(save_directory, exist_ok=True)
    with open(os.path.join(save_directory, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.detach().cpu().contiguous() for k, v in tensors.items()}, os.path.join(save_directory, "adapter.safetensors"))


def load_adapter_files(directory):
    """(config dict, {name: CPU tensor}) of a directory `save_adapter` wrote."""
    from safetensors.torch import load_file
    d = str(directory)
    if not os.path.isfile(os.path.join(d, "adapter_config.json")):
        raise FileNotFoundError(f"{d} holds no adapter_config.json")
    with open(os.path.join(d, "adapter_config.json")) as f:
        cfg = json.load(f)
    return cfg, load_file(os.path.join(d, "adapter.safetensors"))
