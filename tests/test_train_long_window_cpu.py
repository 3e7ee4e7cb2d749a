"""Training at T = 32 and 64 frames, the part that needs no GPU: the new entry point's argument checks, the yardstick itself (the NumPy
training oracle against float64 torch autograd at these lengths -- it had only been pinned at T <= 16), the conditions under which
the cases of tests/test_hip_train_long_window.py run, and the compiled tiled temporal attention backward."""
import importlib.util
import os

import numpy as np
import pytest

import test_hip_train_long_window as LW
from conftest import REPO, pkg
from oracle import genie_train_oracle as TO

LLVM = "/opt/rocm/lib/llvm/bin"
MASKED = {"t32": 29, "t64qk": 666, "t64b3": 391, "t32s64qk": 1364}


def test_entry_point_is_exported_and_checks_its_arguments():
    """genie_temporal_attention_backward: NULL pointers and B <= 0 are argument errors; T > 64, a T that is no power of two,
    head_dim * num_heads != d_model and a qk_ld other than 2 d / 3 d are shape errors -- all before the device or the stream is
    touched (this machine may have neither; the pointers are never dereferenced)."""
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    L = lib_mod.load()
    assert hasattr(L, "genie_temporal_attention_backward") and "genie_temporal_attention_backward" in lib_mod.SIGNATURES
    f = L.genie_temporal_attention_backward
    p = 4096   # never dereferenced
    good = dict(qkv=p, qk=p, ld=3 * 64, do=p, dqkv=p, B=2, T=32, S=3, d=64, H=2, Dh=32)

    def call(**kw):
        a = {**good, **kw}
        return f(a["qkv"], a["qk"], a["ld"], a["do"], a["dqkv"], a["B"], a["T"], a["S"], a["d"], a["H"], a["Dh"], 0.125, 0)

    for k in ("qkv", "qk", "do", "dqkv"):
        assert call(**{k: 0}) == lib_mod.E_ARG, k
    assert call(B=0) == lib_mod.E_ARG and call(B=-1) == lib_mod.E_ARG
    assert call(T=128) == lib_mod.E_SHAPE and b"T=128" in L.genie_last_error()
    for T in (24, 48, 12, 3):
        assert call(T=T) == lib_mod.E_SHAPE, T
    assert call(H=3) == lib_mod.E_SHAPE and b"d_model" in L.genie_last_error()
    assert call(Dh=16) == lib_mod.E_SHAPE
    for ld in (64, 4 * 64, 2 * 64 + 1, 0):
        assert call(ld=ld) == lib_mod.E_SHAPE, ld
    assert b"qk_ld" in L.genie_last_error()
    assert L.genie_version() == 3


def torch_autograd_step(cfg, sd, ids, labels):
    """(loss, {name: gradient}) of the training objective in float64 torch autograd: the embedding, genie_torch_port._block per
    layer, the readout, and the masked factored CE through logsumexp / gather."""
    torch = pytest.importorskip("torch")
    from oracle import genie_oracle as go
    from oracle import genie_torch_port as tp
    F = torch.nn.functional
    with torch.enable_grad():   # the package switches autograd off when it is imported
        t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for k, v in sd.items()}
        B = ids.shape[0]
        T, S, Vf, nv = cfg.T, cfg.S, cfg.factored_vocab_size, cfg.num_factored_vocabs
        x_in = torch.from_numpy(np.asarray(ids, dtype=np.int64)).reshape(B, T, S)
        is_mask = x_in == cfg.image_vocab_size
        safe = torch.where(is_mask, torch.zeros_like(x_in), x_in)
        e = None
        for j in range(nv):
            ej = t[f"token_embed.factored_embeds.{j}.weight"][(safe // Vf ** j) % Vf]
            e = ej if e is None else e + ej
        x = torch.where(is_mask[..., None], t["token_embed.mask_token_embed"][0], e) + t["pos_embed_TSC"]
        for i in range(cfg.num_layers):
            x = tp._block(x, t, i, cfg)
        if cfg.use_mup:
            x = x * cfg.readout_mult
        fl = F.linear(x, t["out_x_proj.weight"], t["out_x_proj.bias"])[:, 1:].reshape(B, T - 1, S, nv, Vf)
        ft = torch.from_numpy(go.factorize_token_ids(np.asarray(labels, dtype=np.int64).reshape(B, T, S)[:, 1:], nv, Vf))
        ce = (torch.logsumexp(fl, -1) - torch.gather(fl, -1, ft[..., None])[..., 0]).sum(-1)
        relevant = is_mask[:, 1:]
        loss = (ce * relevant).sum() / relevant.sum()
        loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}


@pytest.mark.parametrize("name", ["t32", "t64qk"])
def test_float64_oracle_matches_torch_autograd(name):
    """The yardstick of the GPU tests at T = 32 / 64: loss and every gradient tensor of the float64 NumPy oracle within 1e-12 of the
    tensor's largest element of float64 torch autograd (measured: t32 1.5e-15, t64qk 2.2e-15), and no gradient key missing."""
    cfg, sd, ids, labels, loss_o, _, g_o = LW.case(name)
    loss_t, g_t = torch_autograd_step(cfg, sd, ids, labels)
    assert abs(loss_t - loss_o) <= 1e-12 * abs(loss_t)
    assert set(g_o) <= set(g_t), set(g_o) - set(g_t)
    assert all(not np.abs(g).max() > 0 for k, g in g_t.items() if k not in g_o)    # what the oracle leaves out has no gradient
    worst = {k: LW.rel_err(g_o[k], g_t[k]) for k in g_o}
    print(name, max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= 1e-12, max(worst.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("name", LW.F16X3_CASES)
def test_f16x3_number_model_leaves_half_the_bar(name):
    """The rule of tests/test_hip_train_geometry.py: a case runs in f16x3 only where F16X3_TRAIN itself is within GRAD_TOL / 2 =
    5e-5 of the float64 oracle.  Measured: t32 9.5e-6, t64qk 3.4e-5, t64b3 3.4e-5 (t32s64qk, not run in f16x3: 6.1e-5)."""
    cfg, sd, ids, labels, loss, _, grads = LW.case(name)
    loss_m, _, g_m = TO.forward_backward(ids, labels, sd, cfg, nm=TO.F16X3_TRAIN)
    worst = {k: LW.rel_err(g_m[k], grads[k]) for k in grads}
    print(name, max(worst.items(), key=lambda kv: kv[1]))
    assert max(worst.values()) <= 0.5 * LW.GRAD_TOL, max(worst.items(), key=lambda kv: kv[1])
    assert abs(loss_m - loss) < 0.1 * LW.LOSS_TOL * abs(loss)


@pytest.mark.parametrize("name", list(LW.CASES))
def test_cases_have_the_geometry_they_claim(name):
    cfg, _, ids, labels, loss, _, grads = LW.case(name)
    H, d, T, S, B, *_ = LW.CASES[name]
    assert ids.shape == labels.shape == (B, T * S) and B * T * S == LW.TOKENS[name]
    assert T in (32, 64) and cfg.head_dim == d // H and cfg.head_dim in (32, 64) and not cfg.use_mup
    assert S % 16 == 0 and (T * S) % 64 == 0                       # what train_check admits, 16-bit precisions included
    masked = int((ids.reshape(B, T, S)[:, 1:] == cfg.image_vocab_size).sum())
    assert masked >= 8 and masked == MASKED[name], masked
    assert np.isfinite(loss) and 13.0 < loss < 16.0                 # an unsaturated readout (2 ln 512 = 12.5 for a uniform one)
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in grads.values())


def test_compiled_tiled_backward_has_no_scratch():
    """Every instantiation of attn_temporal_bwd_tiled_kernel (head_dim 32 / 64 x T 32 / 64) in the built library: no scratch, MFMAs
    present, and no more registers than one wave per SIMD has (512: the kernel runs one wave per SIMD by design).  The T = 16 kernel
    beside it (attn_temporal_bwd_mfma_kernel) keeps its occupancy: registers are allocated in blocks of 8, and 128 at head_dim 64 / 72
    at head_dim 32 are 4 / 7 waves per SIMD."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(REPO, "tools", "isa_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    audit = mod.audit(lib_mod.LIB_PATH, all_kernels=True)
    rows = {r[0]: r for r in audit if "attn_temporal_bwd_tiled_kernel<" in r[0]}
    for dh, allocated in ((64, 128), (32, 72)):
        (row,) = [r for r in audit if f"attn_temporal_bwd_mfma_kernel<{dh}>" in r[0]]
        assert row[6] == 0 and row[5] > 0 and (row[7] + 7) // 8 * 8 <= allocated, row
    assert len(rows) == 4, sorted(rows)
    for name, (_, _, _, _, _, mfma, scratch, vgpr) in rows.items():
        print(name, "mfma", mfma, "scratch", scratch, "vgpr", vgpr)
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
        assert mfma > 0 and 0 < vgpr <= 512, (name, mfma, vgpr)
