"""CPU-only tests of fan-out generation (genie_generate_fanout, generate.fanout_frames): the C ABI additions (exported, bound, argument
errors before any HIP call, the size functions), the Python shape checks, and the compiled flavours of the two decode attention
kernels (csrc/kernels_attn_temporal.hip, csrc/kernels_frame.hip: no scratch, no LDS)."""
import os
import subprocess
import sys

import pytest

from conftest import REPO, pkg

torch = pytest.importorskip("torch")


def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def small_cfg(**kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=8, S=16, num_factored_vocabs=2, qk_norm=False)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


NEW = ("genie_generate_fanout", "genie_fanout_branch_bytes", "genie_fanout_workspace_bytes", "genie_temporal_attention_decode_fanout")


def test_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    assert "GENIE_ABI_VERSION 3" in header
    G = pkg("generate")
    for n in ("fanout_frames", "fanout_call", "fanout_cond"):
        assert hasattr(G, n), n
    assert hasattr(pkg("st_mask_git").STMaskGIT, "fanout")


def test_generate_fanout_rejects_bad_arguments_before_any_hip_call():
    """GENIE_E_ARG from host code with NULL or fake device pointers: nothing is enqueued, and the message names the argument."""
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())           # T = 8
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    E = lib_mod.E_ARG
    fake = 1 << 20
    big = 1 << 40

    def call(B=2, K=3, P=3, n_new=4, steps=2, temperature=0.0, mode=1, uniforms=None, cond=None, guide=None, ids=fake, gen=fake,
             trunk=fake, trunk_bytes=big, branch=fake, branch_bytes=big, ws=fake, ws_bytes=big, wt=w):
        return L.genie_generate_fanout(cfg, wt, ids, B, K, P, n_new, steps, temperature, mode, None, uniforms, 1, gen, trunk, trunk_bytes,
                                       branch, branch_bytes, ws, ws_bytes, None, cond, None, guide)

    for kw, word in ((dict(K=0), b"K=0"), (dict(K=-1), b"K=-1"), (dict(B=0), b"B=0"), (dict(P=0), b"prompt"), (dict(P=5, n_new=4), b"of at most 8"),
                     (dict(P=8, n_new=1), b"of at most 8"), (dict(n_new=0), b"new frames"), (dict(steps=0), b"steps"),
                     (dict(temperature=1.0), b"uniforms"), (dict(mode=0), b"draws"), (dict(mode=7), b"unmask_mode"),
                     (dict(B=1 << 20, K=1 << 20), b"too many"), (dict(B=1 << 15, K=1 << 15), b"too many"),
                     (dict(ids=None), b"NULL pointer"), (dict(gen=None), b"NULL pointer"), (dict(trunk=None), b"NULL pointer"),
                     (dict(branch=None), b"NULL pointer"), (dict(ws=None), b"NULL pointer"), (dict(wt=None), b"NULL pointer"),
                     (dict(trunk_bytes=L.genie_prefix_cache_bytes(cfg, 2) - 1), b"trunk cache too small"),
                     (dict(branch_bytes=L.genie_fanout_branch_bytes(cfg, 2, 3, 4) - 1), b"branch cache too small"),
                     (dict(ws_bytes=L.genie_fanout_workspace_bytes(cfg, 2, 3, 3, 0) - 1), b"workspace too small")):
        rc = call(**kw)
        assert rc == (lib_mod.E_UNSUPPORTED if kw == dict(mode=7) else E), (kw, rc, L.genie_last_error())
        assert word in L.genie_last_error(), (kw, L.genie_last_error())
    # guidance needs a usable action condition; under it the buffers are those of 2 B clips
    cond = lib_mod.FrameCond(table=fake, ids=fake, n_actions=5)
    for c, g in ((None, lib_mod.Guidance(3.0, 0)), (cond, lib_mod.Guidance(3.0, 5))):
        assert call(cond=c, guide=g) == E and b"guidance" in L.genie_last_error()
    assert call(cond=cond, guide=lib_mod.Guidance(3.0, 4), trunk_bytes=L.genie_prefix_cache_bytes(cfg, 4) - 1) == E
    assert b"trunk cache too small" in L.genie_last_error()
    assert call(cond=cond, guide=lib_mod.Guidance(3.0, 4), ws_bytes=L.genie_fanout_workspace_bytes(cfg, 2, 3, 3, 1) - 1) == E
    assert b"workspace too small" in L.genie_last_error()


def test_decode_fanout_kernel_entry_rejects_bad_arguments_before_any_hip_call():
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())           # T = 8
    aw = lib_mod.AttnWeights()
    fake = 1 << 20

    def call(NBK=6, K=3, P0=3, Tb=4, t=4, trunk=fake, branch=fake, out=fake, c=cfg):
        return L.genie_temporal_attention_decode_fanout(c, aw, trunk, branch, out, NBK, K, P0, Tb, t, 0, None)

    for kw in (dict(K=0), dict(NBK=7), dict(NBK=0), dict(P0=5), dict(P0=-1), dict(t=8), dict(Tb=1, t=4), dict(Tb=0), dict(trunk=None),
               dict(branch=None), dict(out=None), dict(c=None)):
        assert call(**kw) == lib_mod.E_ARG, kw
    bad = lib_mod.make_cfg(small_cfg())
    bad.head_dim = 12
    assert call(c=bad) == lib_mod.E_SHAPE


def test_size_functions():
    lib_mod, L = _lib()
    for cfg in (lib_mod.make_cfg(small_cfg()), lib_mod.make_cfg(small_cfg(T=16, S=64, d_model=64, num_layers=3))):
        T, slot = cfg.T, cfg.S * 3 * cfg.d_model * 4
        for NB in (1, 2, 6):
            for K in (1, 3, 16):
                for n_new in (1, 2, T - 1):
                    assert L.genie_fanout_branch_bytes(cfg, NB, K, n_new) == cfg.num_layers * NB * K * n_new * slot
        # half the window as context, 5 branches: trunk + branches hold 2 T + 10 T / 2 slots, the replicated batch's cache 10 T
        assert 10 * (L.genie_prefix_cache_bytes(cfg, 2) + L.genie_fanout_branch_bytes(cfg, 2, 5, T // 2)) == 7 * L.genie_prefix_cache_bytes(cfg, 10)
        for guided in (0, 1):
            for B in (1, 3):
                for P in (1, 2, T - 1):
                    sizes = [L.genie_fanout_workspace_bytes(cfg, B, K, P, guided) for K in (1, 2, 3, 8, 64)]
                    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
                    # K = 1 decodes what generate does: no less room than that loop's own passes need
                    assert sizes[0] >= L.genie_workspace_bytes(cfg, 2 * B if guided else B)
                    # ... and it does not grow as the K-times replicated batch's full-window workspace would
                    assert sizes[-1] < L.genie_workspace_bytes(cfg, 64 * B * (2 if guided else 1))
                assert L.genie_fanout_workspace_bytes(cfg, B, 4, 2, 1) >= L.genie_fanout_workspace_bytes(cfg, B, 4, 2, 0)
        for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, T), (-1, 2, 2), (1 << 20, 1 << 20, 1)):
            assert L.genie_fanout_branch_bytes(cfg, *bad) == 0, bad
        for bad in ((0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, T, 0), (1 << 20, 1 << 20, 1, 0), (1 << 15, 1 << 14, 1, 1)):
            assert L.genie_fanout_workspace_bytes(cfg, *bad) == 0, bad
    assert L.genie_fanout_branch_bytes(None, 1, 1, 1) == 0 and L.genie_fanout_workspace_bytes(None, 1, 1, 1, 0) == 0


def test_python_shape_checks_raise_before_the_library_is_called(monkeypatch):
    G = pkg("generate")
    M = pkg("st_mask_git").STMaskGIT
    monkeypatch.setattr(M, "_device", lambda self: torch.device("cpu"))          # (checked vectors are moved to the model's device)
    m = M(small_cfg())
    prompt = torch.zeros(2, 3, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        G.fanout_frames(m, prompt, 4)                                            # an unconditioned model takes K explicitly
    for kw in (dict(n_new=0, K=2), dict(n_new=6, K=2), dict(n_new=4, K=0), dict(n_new=4, K=-2)):
        with pytest.raises(ValueError):
            G.fanout_frames(m, prompt, **kw)
    with pytest.raises(ValueError):
        G.fanout_frames(m, torch.zeros(2, 8, 4, 4, dtype=torch.long), 1, K=2)    # P = T
    with pytest.raises(RuntimeError):
        G.fanout_frames(m, torch.zeros(2, 3, 16, dtype=torch.long), 4, K=2)      # not (B, P, H, W)
    with pytest.raises(ValueError):
        m.fanout(prompt, 4, action_ids=torch.zeros(2, 3, 4, dtype=torch.long))   # a model without actions
    ma = M(small_cfg(action_vocab_size=5))
    good = torch.zeros(2, 3, 4, dtype=torch.long)
    pa = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        ma.fanout(prompt, 4, K=3)                                                # actions missing
    with pytest.raises(ValueError):
        ma.fanout(prompt, 4, action_ids=good)                                    # prompt_actions missing
    with pytest.raises(ValueError):
        ma.fanout(prompt, 4, K=2, action_ids=good, prompt_actions=pa)            # K disagrees with the actions
    for bad in (torch.zeros(2, 3, 5, dtype=torch.long), torch.zeros(3, 3, 4, dtype=torch.long), torch.zeros(2, 12, dtype=torch.long)):
        with pytest.raises(RuntimeError):
            ma.fanout(prompt, 4, action_ids=bad, prompt_actions=pa)
    with pytest.raises(RuntimeError):
        ma.fanout(prompt, 4, action_ids=good, prompt_actions=torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(RuntimeError):
        ma.fanout(prompt, 4, action_ids=good.float(), prompt_actions=pa)
    with pytest.raises(IndexError):
        ma.fanout(prompt, 4, action_ids=torch.full((2, 3, 4), 5), prompt_actions=pa)
    with pytest.raises(ValueError):
        ma.fanout(prompt, 4, action_ids=good, prompt_actions=pa, action_vectors=torch.zeros(2, 3, 4, 6))
    mv = M(small_cfg(action_dim=6))
    vec, pv = torch.zeros(2, 3, 4, 6), torch.zeros(2, 3, 6)
    with pytest.raises(ValueError):
        mv.fanout(prompt, 4, action_ids=good, prompt_actions=pa)                 # ids given to a model of action vectors
    with pytest.raises(ValueError):
        mv.fanout(prompt, 4, action_vectors=vec)                                 # prompt_action_vectors missing
    for bad in (torch.zeros(2, 3, 4, 5), torch.zeros(2, 3, 5, 6), torch.zeros(2, 12, 6)):
        with pytest.raises(RuntimeError):
            mv.fanout(prompt, 4, action_vectors=bad, prompt_action_vectors=pv)
    with pytest.raises(RuntimeError):
        mv.fanout(prompt, 4, action_vectors=vec, prompt_action_vectors=torch.zeros(2, 2, 6))
    with pytest.raises(RuntimeError):
        mv.fanout(prompt, 4, action_vectors=vec.long(), prompt_action_vectors=pv)
    with pytest.raises(ValueError):
        mv.fanout(prompt, 4, action_vectors=torch.full((2, 3, 4, 6), float("nan")), prompt_action_vectors=pv)
    # what the checks hand on: K from the actions, branch-major rows
    B, P, K, a_p, a_b, v_p, v_b = G._fanout_inputs(ma, prompt, 4, None, torch.arange(24).view(2, 3, 4) % 5, None, pa, None)
    assert (B, P, K) == (2, 3, 3) and a_b.shape == (6, 4) and a_p.shape == (2, 3) and v_p is None and v_b is None
    assert a_b[4].tolist() == [(16 + j) % 5 for j in range(4)]                   # row b * K + k = branch k of clip b


def test_fanout_kernel_flavours_use_no_scratch_and_no_lds():
    """The built code object: every instantiation of the two decode attention kernels (csrc/kernels_attn_temporal.hip, csrc/kernels_frame.hip),
    ordinary and fan-out, keeps its scores in registers (the `single` kernel's t >= 16 path keeps score j in lane j: no indexed array in
    scratch), and none uses LDS."""
    LLVM = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod, _ = _lib()
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(REPO, "tools", "isa_audit.py"))
    audit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audit)
    rows = {r[0]: r for r in audit.audit(lib_mod.LIB_PATH, all_kernels=True)}
    single = {k: v for k, v in rows.items() if "attn_temporal_single_kernel<" in k}
    fr = {k: v for k, v in rows.items() if "attn_temporal_fr_kernel<" in k and k.rstrip().endswith("true>")}
    assert len(single) == 16 and len(fr) == 2, (sorted(single), sorted(fr))     # head_dim 8 / 16 / 32 / 64 x f32 / bf16 x ordinary / fan-out; 64 / 32
    assert sum(k.rstrip().endswith("true>") for k in single) == 8, sorted(single)
    for name, r in {**single, **fr}.items():
        assert r[6] == 0, f"{name}: {r[6]} bytes of scratch per lane"
        assert r[7] <= 80, f"{name}: {r[7]} registers (79 at most before the fan-out flavour existed)"
    # no LDS: the group segment size in the kernels' own metadata
    import re
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        meta = "".join(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
                       for co in audit.code_objects(lib_mod.LIB_PATH, tmp))
    lds = {}
    for block in re.split(r"\n\s*- \.agpr_count:", meta):
        name, size = re.search(r"\.name:\s+(\S+)", block), re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        if name and size and re.search(r"attn_temporal_single_kernel|attn_temporal_fr_kernel.*Lb1E", name.group(1)):
            lds[name.group(1)] = int(size.group(1))
    assert len(lds) == 18 and not any(lds.values()), lds


def test_tools_list_the_fanout_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "generate.py"), "--help"], capture_output=True, text=True, check=True)
    assert "--fanout" in out.stdout and "--fanout_actions" in out.stdout
    assert "--fanout" in open(os.path.join(REPO, "tools", "bench_generate.py")).read()
