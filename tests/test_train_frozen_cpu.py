"""Training a subset of the weights, the part that runs anywhere (1xgpt_amd/train.py: select_trainable, lr_factors, FlatLayout; the
bucketed gradient exchange over a trainable prefix; the C ABI of genie_train_pack_weights_some).  tests/test_hip_train_frozen.py holds
the GPU side."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO, pkg
from test_distributed_gloo import _free_port


def cfg3(**kw):
    args = dict(num_layers=3, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False, num_prompt_frames=2)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


def numels(cfg):
    return {k: int(np.prod(shape)) for k, shape, *_ in pkg("synthetic").state_dict_spec(cfg)
            if k not in ("action_mean", "action_std")}   # buffers, not parameters


NAMES = sorted(numels(cfg3()))


# ---------------------------------------------------------------------------------------------- select_trainable
def test_select_trainable_patterns():
    S = pkg("train").select_trainable
    assert S(NAMES) == set(NAMES)
    assert S(NAMES, train_only="out_x_proj.*") == {"out_x_proj.weight", "out_x_proj.bias"}
    assert S(NAMES, train_only=["out_x_proj.*"]) == S(NAMES, train_only="out_x_proj.*")
    last = S(NAMES, train_only="decoder.layers.2.*,out_x_proj.*")
    assert last == {n for n in NAMES if n.startswith(("decoder.layers.2.", "out_x_proj."))}
    assert S(NAMES, train_only="decoder.layers.[12].*") == {n for n in NAMES if n.startswith(("decoder.layers.1.", "decoder.layers.2."))}
    assert S(NAMES, train_only="*.bias,*norm*.weight") == {n for n in NAMES if n.endswith(".bias") or ("norm" in n and n.endswith(".weight"))}
    assert S(NAMES, freeze="decoder.*") == {n for n in NAMES if not n.startswith("decoder.")}
    # freeze applies after train_only; an exact name is a pattern; matching is case-sensitive and over the whole name
    assert S(NAMES, train_only="decoder.layers.0.*", freeze="*.bias") == {n for n in NAMES if n.startswith("decoder.layers.0.") and not n.endswith(".bias")}
    assert S(NAMES, train_only="pos_embed_TSC") == {"pos_embed_TSC"}
    assert S(NAMES, train_only="token_embed.*") == {n for n in NAMES if n.startswith("token_embed.")}
    with pytest.raises(ValueError, match="matches no parameter"):
        S(NAMES, train_only="pos_embed_tsc")
    with pytest.raises(ValueError, match="matches no parameter"):
        S(NAMES, train_only="decoder.layers.0")          # a prefix is not a match
    an = sorted(numels(cfg3(action_dim=3)))
    assert S(an, train_only="action_*") == {"action_proj.weight", "action_proj.bias", "action_null"}
    assert S(sorted(numels(cfg3(action_vocab_size=5))), train_only="action_*") == {"action_embed.weight"}


def test_select_trainable_refuses_a_typo_and_an_empty_selection():
    S = pkg("train").select_trainable
    with pytest.raises(ValueError, match="train_only pattern 'decoder.layers.7.*' matches no parameter"):
        S(NAMES, train_only="out_x_proj.*,decoder.layers.7.*")
    with pytest.raises(ValueError, match="freeze pattern 'nope' matches no parameter"):
        S(NAMES, freeze=["nope"])
    with pytest.raises(ValueError, match="no trainable parameter is left"):
        S(NAMES, train_only="out_x_proj.*", freeze="out_x_proj.*")
    with pytest.raises(ValueError, match="no trainable parameter is left"):
        S(NAMES, freeze="*")


def test_lr_factors():
    F = pkg("train").lr_factors
    assert set(F(NAMES).values()) == {1.0} and F(NAMES, {}) == F(NAMES)
    f = F(NAMES, {"out_x_proj.bias": 3.0, "out_x_proj.*": 10.0, "*.bias": 0.5})   # the first pattern that matches
    assert f["out_x_proj.bias"] == 3.0 and f["out_x_proj.weight"] == 10.0
    assert f["decoder.layers.0.mlp.fc1.bias"] == 0.5 and f["decoder.layers.0.mlp.fc1.weight"] == 1.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="finite and > 0"):
            F(NAMES, {"*.bias": bad})
    with pytest.raises(ValueError, match="matches no parameter"):
        F(NAMES, {"out_proj.*": 2.0})


# ---------------------------------------------------------------------------------------------- the flat layout
def layout(sel=None, lr_scale=None, cfg=None, **kw):
    T = pkg("train")
    cfg = cfg or cfg3()
    n = numels(cfg)
    chosen = None if sel is None and not kw else T.select_trainable(n, sel, **kw)
    return cfg, n, T.FlatLayout(cfg, n, chosen, lr_scale)


def check_layout(cfg, n, lay):
    """What holds for every selection: the prefix is the trainable names in ready order, then the frozen ones in ready order; tensors are
    256-byte aligned and do not overlap; runs and segments tile the prefix in order; runs break exactly where (decay flag, lr factor)
    changes; stop / embed are the documented ones."""
    T = pkg("train")
    ro = T.ready_order(cfg, n)
    k = len(lay.trainable)
    assert lay.order[:k] == [x for x in ro if x in lay.trainable] and lay.order[k:] == [x for x in ro if x not in lay.trainable]
    o = 0
    for name in lay.order:
        assert lay.offsets[name] == (o, o + n[name]) and o % 64 == 0
        o += (n[name] + 63) // 64 * 64
    assert lay.n_flat == o and lay.n_train == (lay.offsets[lay.order[k]][0] if k < len(lay.order) else o)
    # AdamW runs: contiguous, cover [0, n_train), one per maximal stretch of equal (decay flag, factor)
    assert lay.adam_runs[0][0] == 0 and lay.adam_runs[-1][1] == lay.n_train
    assert all(a[1] == b[0] for a, b in zip(lay.adam_runs, lay.adam_runs[1:]))
    assert all((a[2], a[3]) != (b[2], b[3]) for a, b in zip(lay.adam_runs, lay.adam_runs[1:]))
    for name in lay.order[:k]:
        (run,) = [r for r in lay.adam_runs if r[0] <= lay.offsets[name][0] and lay.offsets[name][1] <= r[1]]
        assert (run[2], run[3]) == (T.decays(name), lay.lr_factor[name]), name
    # segments: the groups that hold a trainable tensor, in ready order, tiling the prefix
    def group(x):
        return "head" if x.startswith("out_x_proj.") else (int(x.split(".")[2]) if x.startswith("decoder.layers.") else "embed")
    want = []
    for x in lay.order[:k]:
        if group(x) not in want:
            want.append(group(x))
    assert [g for g, _, _ in lay.groups] == want
    assert lay.segments == [(lo, hi) for _, lo, hi in lay.groups]
    assert lay.segments[0][0] == 0 and lay.segments[-1][1] == lay.n_train
    assert all(a[1] == b[0] for a, b in zip(lay.segments, lay.segments[1:]))
    emb = any(group(x) == "embed" for x in lay.trainable)
    layers = [group(x) for x in lay.trainable if isinstance(group(x), int)]
    assert lay.embed == emb
    assert lay.stop == (0 if emb else min(layers) if layers else cfg.num_layers)
    assert lay.all == (k == len(n))


def test_layout_all_trainable_is_the_layout_of_before():
    """trainable=None: ready order, one segment per group (head, layers L-1 .. 0, embeddings), runs that break at decay-flag changes only."""
    cfg, n, lay = layout()
    check_layout(cfg, n, lay)
    T = pkg("train")
    assert lay.all and lay.order == T.ready_order(cfg, n) and lay.n_train == lay.n_flat
    assert [g for g, _, _ in lay.groups] == ["head", 2, 1, 0, "embed"] and lay.stop == 0 and lay.embed
    runs, o = [], 0
    for name in lay.order:   # the loop the trainer ran before layouts could be partial
        pad = (n[name] + 63) // 64 * 64
        if runs and runs[-1][2] == T.decays(name):
            runs[-1][1] = o + pad
        else:
            runs.append([o, o + pad, T.decays(name)])
        o += pad
    assert [r[:3] for r in lay.adam_runs] == [tuple(r) for r in runs] and {r[3] for r in lay.adam_runs} == {1.0}


SELECTIONS = {
    "head": ("out_x_proj.*", ["head"], 3, False),
    "last+head": ("decoder.layers.2.*,out_x_proj.*", ["head", 2], 2, False),
    "biases+norms": ("*.bias,*norm*.weight", ["head", 2, 1, 0], 0, False),
    "scattered": ("decoder.layers.1.mlp.fc1.weight,decoder.layers.0.spatial_attn.qkv.weight,pos_embed_TSC", [1, 0, "embed"], 0, True),
    "embeddings": ("token_embed.*", ["embed"], 0, True),
    "middle": ("decoder.layers.1.*", [1], 1, False),
}


@pytest.mark.parametrize("tag", list(SELECTIONS))
def test_layout_of_a_selection(tag):
    sel, groups, stop, embed = SELECTIONS[tag]
    cfg, n, lay = layout(sel)
    check_layout(cfg, n, lay)
    assert [g for g, _, _ in lay.groups] == groups and lay.stop == stop and lay.embed == embed and not lay.all
    assert lay.n_train < lay.n_flat


def test_layout_runs_break_at_lr_factor_changes():
    cfg, n, lay = layout("decoder.layers.2.*,out_x_proj.*", {"out_x_proj.*": 10.0, "decoder.layers.2.mlp.*": 2.0})
    check_layout(cfg, n, lay)
    # head: weight (decays) | bias: one factor, two decay flags; layer 2: decaying tensors first, the MLP's among them at factor 2
    assert [(r[2], r[3]) for r in lay.adam_runs[:2]] == [(True, 10.0), (False, 10.0)]
    assert {r[3] for r in lay.adam_runs} == {10.0, 2.0, 1.0}
    _, _, same = layout("decoder.layers.2.*,out_x_proj.*")
    assert len(lay.adam_runs) > len(same.adam_runs) == 4
    # a factor on a frozen tensor changes nothing
    _, _, frozen = layout("out_x_proj.*", {"decoder.*": 5.0})
    assert [(r[2], r[3]) for r in frozen.adam_runs] == [(True, 1.0), (False, 1.0)]


def test_layout_of_action_models():
    for kw, new in ((dict(action_dim=3), {"action_proj.weight", "action_proj.bias", "action_null"}), (dict(action_vocab_size=5), {"action_embed.weight"})):
        cfg, n, lay = layout("action_*", cfg=cfg3(**kw))
        check_layout(cfg, n, lay)
        assert lay.trainable == new and lay.stop == 0 and lay.embed and [g for g, _, _ in lay.groups] == ["embed"]
    cfg, n, lay = layout("action_proj.bias", cfg=cfg3(action_dim=3))   # one of the three on its own
    check_layout(cfg, n, lay)
    assert lay.order[0] == "action_proj.bias" and lay.n_train == 64


def test_layout_refuses_unknown_names():
    T = pkg("train")
    with pytest.raises(ValueError):
        T.FlatLayout(cfg3(), numels(cfg3()), {"out_x_proj.weight", "nope"})
    with pytest.raises(ValueError):
        T.FlatLayout(cfg3(), numels(cfg3()), set())


# ---------------------------------------------------------------------------------------------- the exchange over a prefix
def _prefix_case(rank):
    """A partial layout and this rank's values for its gradient buffer (the trainable prefix alone)."""
    T = pkg("train")
    cfg = cfg3()
    n = numels(cfg)
    lay = T.FlatLayout(cfg, n, T.select_trainable(n, "decoder.layers.1.mlp.fc1.weight,decoder.layers.0.spatial_attn.qkv.*,pos_embed_TSC,out_x_proj.bias"))
    g = np.random.default_rng(100 + rank).standard_normal(lay.n_train).astype(np.float32)
    return lay, g


def _prefix_worker(rank, world, port, q):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from conftest import pkg as _pkg
    D, T = _pkg("distributed"), _pkg("train")
    D.init_distributed(backend="gloo")
    lay, g = _prefix_case(rank)
    flat = torch.from_numpy(g.copy())
    red = T.BucketReducer(flat, T.bucket_bounds(lay.segments, 4096))   # small buckets: several in flight
    assert red.world == world and len(red.bounds) > 1 and red.bounds[-1][1] == lay.n_train
    hi = {k: h for k, _, h in lay.groups}
    for key in ["head"] + list(reversed(range(lay.stop, 3))) + ["embed"]:   # the trainer's calls; a group without a segment says nothing
        if key in hi:
            red.ready(hi[key])
    red.finish()
    q.put((rank, flat.numpy().copy()))
    torch.distributed.destroy_process_group()


def test_gloo_world2_buckets_over_a_trainable_prefix():
    """BucketReducer over the segments of a partial layout (head bias, one weight of layer 1, two tensors of layer 0, pos_embed; layer 2
    absent): every element of the prefix is summed exactly once on both ranks."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_prefix_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    lay, g0 = _prefix_case(0)
    assert [k for k, _, _ in lay.groups] == ["head", 1, 0, "embed"] and lay.n_train < lay.n_flat
    want = g0 + _prefix_case(1)[1]
    for r in range(world):
        assert np.array_equal(res[r], want)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_is_c99_and_exports_pack_weights_some(tmp_path):
    """include/genie_hip.h with the "Frozen tensors" section still compiles as C99, and a C program links genie_train_pack_weights_some and
    gets its host-side refusals (no GPU needed): NULL arguments and the exact precision, GENIE_E_ARG like genie_train_pack_weights."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    assert "genie_train_pack_weights_some" in lib_mod.SIGNATURES
    assert hasattr(lib_mod.load(), "genie_train_pack_weights_some") and lib_mod.load().genie_version() == 3
    assert "Frozen tensors" in open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = tmp_path / "frozen.c"
    src.write_text('#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_cfg c; genie_weights w; genie_layer_weights l[2];\n"
                   "    memset(&c, 0, sizeof c); memset(&w, 0, sizeof w); memset(l, 0, sizeof l);\n"
                   "    c.num_layers = 2; c.num_heads = 2; c.head_dim = 32; c.d_model = 64; c.T = 4; c.S = 16; c.hidden = 256;\n"
                   "    c.factored_vocab = 512; c.num_factored = 2; c.image_vocab_size = 262144; c.attn_scale = 0.17f; c.readout_mult = 1.0f;\n"
                   "    w.layers_host = l;\n"
                   "    c.precision = GENIE_PREC_BF16;\n"
                   "    if (genie_version() != GENIE_ABI_VERSION || GENIE_ABI_VERSION != 3) return 1;\n"
                   "    if (genie_train_pack_weights_some(&c, &w, &w, 0, 0, 0) != GENIE_E_ARG) return 2;      /* a NULL table */\n"
                   "    if (genie_train_pack_weights_some(0, &w, &w, &w, &w, 0) != GENIE_E_ARG) return 3;\n"
                   "    c.precision = GENIE_PREC_EXACT;\n"
                   "    if (genie_train_pack_weights_some(&c, &w, &w, &w, 0, 0) != GENIE_E_ARG) return 4;     /* no 16-bit copies to make */\n"
                   "    if (genie_train_pack_weights(&c, &w, &w, &w, 0) != GENIE_E_ARG) return 5;             /* ... like its sibling */\n"
                   "    if (strstr(genie_last_error(), \"exact\") == 0) return 6;\n"
                   "    c.precision = GENIE_PREC_F16X3;\n"
                   "    if (genie_train_pack_weights_some(&c, &w, &w, &w, &w, 0) != GENIE_OK) return 7;       /* nothing selected: nothing to do */\n"
                   "    return 0;\n}\n")
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "frozen.o")], check=True)
    exe = tmp_path / "frozen"
    subprocess.run([gcc, str(tmp_path / "frozen.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
