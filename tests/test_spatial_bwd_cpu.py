"""The spatial attention backward and qk-norm kernels one by one, the part that needs no GPU: the references of
tests/spatial_bwd_model.py against float64 torch autograd of the plain formulas, the new entry points' argument checks, a table of
wrong variants that every acceptance function of tests/test_hip_spatial_bwd.py must reject on that file's own inputs, and the
conditions on those inputs."""
import os

import numpy as np
import pytest

import spatial_bwd_model as M
from conftest import pkg

# the S = 256 inputs of the fused and bf16 GPU cases the mutants are applied to: (head_dim, ld3, q_mul), both head_dims, both
# sources of q | k and both row regimes
MUTANT_INPUTS = [(32, True, 1.0), (32, False, 4.0), (64, False, 1.0), (64, True, 4.0)]
ALL_S256 = [(Dh, ld3, q) for Dh in (32, 64) for ld3 in (True, False) for q in (1.0, 4.0)]


# ---------------------------------------------------------------------------------------------- references vs torch autograd
@pytest.mark.parametrize("S,Dh,ld3,q_mul", [(16, 16, False, 4.0), (16, 128, True, 1.0), (144, 32, False, 1.0), (256, 64, True, 4.0)])
def test_attention_restatement_matches_torch_autograd(S, Dh, ld3, q_mul):
    """dq, dk, dv of the float64 restatement within 1e-12 of the block's largest element of float64 torch autograd of
    softmax(scale q k^T) v -- a derivation that is not the project's."""
    torch = pytest.importorskip("torch")
    (qkv, qk, dO, H, scale), ref, _ = M.attn_case(S, Dh, ld3, q_mul)
    n, _, d3 = qkv.shape
    d = d3 // 3
    with torch.enable_grad():   # the package switches autograd off when it is imported
        t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).reshape(n, S, H, Dh).transpose(1, 2).requires_grad_(True)  # noqa: E731
        q, k, v = t(qk[..., :d]), t(qk[..., d:2 * d]), t(qkv[..., 2 * d:])
        out = torch.softmax(scale * q @ k.transpose(-1, -2), -1) @ v                       # (n, H, S, Dh)
        out.backward(torch.from_numpy(dO.astype(np.float64)).reshape(n, S, H, Dh).transpose(1, 2))
    for name, mine, theirs in zip(("dq", "dk", "dv"), ref, (q.grad, k.grad, v.grad)):
        err = M.rel_err(mine, theirs.transpose(1, 2).reshape(n, S, d).numpy())
        print(name, err)
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("Dh,rows,H", [(32, 37, 3), (64, 3, 1), (128, 37, 3)])
def test_qk_norm_restatement_matches_torch_autograd(Dh, rows, H):
    """Forward and the three gradients of the float64 qk-norm restatement within 1e-12 of float64 F.layer_norm and its autograd."""
    torch = pytest.importorskip("torch")
    (qkv, dy, nw, nb), fwd, _, bwd, _ = M.qk_norm_case(Dh, rows, H)
    d = H * Dh
    with torch.enable_grad():
        x = torch.from_numpy(qkv[:, :2 * d].astype(np.float64)).requires_grad_(True)
        w = torch.from_numpy(nw.astype(np.float64)).requires_grad_(True)
        b = torch.from_numpy(nb.astype(np.float64)).requires_grad_(True)
        y = torch.nn.functional.layer_norm(x.reshape(rows, 2, H, Dh), (Dh,), w, b, eps=1e-5).reshape(rows, 2 * d)
        y.backward(torch.from_numpy(dy.astype(np.float64)))
    for name, mine, theirs in zip(("qkn", "d_qk", "d_norm_w", "d_norm_b"), (fwd,) + bwd, (y.detach(), x.grad, w.grad, b.grad)):
        err = M.rel_err(mine, theirs.numpy())
        print(name, err)
        assert err <= 1e-12, (name, err)


def test_bf16_rounding_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 1e-30, 0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0.0, 0.0], np.float32)
    got = M.bf16(x)
    assert np.array_equal(got[:5], want[:5]) and got[6] == 0.0 and abs(got[5] - 1e-30) < 1e-32
    assert M.bf16(x.astype(np.float64)).dtype == np.float64 and np.array_equal(M.bf16(x.astype(np.float64)), got.astype(np.float64))


# ---------------------------------------------------------------------------------------------- the entry points refuse bad input
def test_entry_points_are_exported_and_check_their_arguments():
    """Every argument, shape and unsupported-path answer of genie_spatial_attention_backward, genie_qk_norm_forward and
    genie_qk_norm_backward, before the device or the stream is touched (this machine may have neither; the pointers are never
    dereferenced)."""
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    L = lib_mod.load()
    for name in ("genie_spatial_attention_backward", "genie_spatial_attention_backward_workspace_bytes", "genie_qk_norm_forward",
                 "genie_qk_norm_backward", "genie_qk_norm_backward_scratch_bytes"):
        assert hasattr(L, name) and name in lib_mod.SIGNATURES, name
    AUTO, FUSED, MAT, BF16 = (lib_mod.SPATIAL_BWD_AUTO, lib_mod.SPATIAL_BWD_FUSED, lib_mod.SPATIAL_BWD_MATERIALISED,
                              lib_mod.SPATIAL_BWD_BF16)
    p = 4096   # never dereferenced
    size = L.genie_spatial_attention_backward_workspace_bytes
    assert size(FUSED, 3, 256, 2) == 0
    assert size(MAT, 3, 144, 2) == 2 * ((3 * 2 * 144 * 144 * 4 + 255) // 256 * 256) == size(AUTO, 3, 144, 2)
    assert size(BF16, 3, 256, 2) == 3 * 2 * 256 * 4 * 4
    assert size(7, 3, 256, 2) == 0 and size(MAT, 0, 256, 2) == 0 and size(MAT, 3, 0, 2) == 0 and size(MAT, 3, 256, 0) == 0

    good = dict(qkv=p, qk=p, ld=3 * 64, do=p, dqkv=p, n=3, S=144, d=64, H=2, Dh=32, path=MAT, ws=p, wsb=1 << 30)

    def call(**kw):
        a = {**good, **kw}
        return L.genie_spatial_attention_backward(a["qkv"], a["qk"], a["ld"], a["do"], a["dqkv"], a["n"], a["S"], a["d"], a["H"],
                                                  a["Dh"], 0.125, a["path"], a["ws"], a["wsb"], 0)

    for k in ("qkv", "qk", "do", "dqkv"):
        assert call(**{k: 0}) == lib_mod.E_ARG, k
    assert call(n=0) == lib_mod.E_ARG and call(n=-1) == lib_mod.E_ARG
    for path in (-1, 4):
        assert call(path=path) == lib_mod.E_ARG and b"path" in L.genie_last_error()
    for S in (8, 24, 250):
        assert call(S=S) == lib_mod.E_SHAPE, S
    assert call(Dh=24, d=48) == lib_mod.E_SHAPE and b"multiples of 16" in L.genie_last_error()
    assert call(H=3) == lib_mod.E_SHAPE and b"d_model" in L.genie_last_error()
    assert call(Dh=16) == lib_mod.E_SHAPE
    for ld in (64, 4 * 64, 2 * 64 + 1, 0):
        assert call(ld=ld) == lib_mod.E_SHAPE, ld
    assert b"qk_ld" in L.genie_last_error()
    # a forced path outside its geometry: S != 256, or head_dim outside {32, 64}
    for path in (FUSED, BF16):
        assert call(path=path) == lib_mod.E_UNSUPPORTED, path
        assert call(path=path, S=16) == lib_mod.E_UNSUPPORTED
        assert call(path=path, S=256, Dh=16, d=32, ld=96) == lib_mod.E_UNSUPPORTED
        assert call(path=path, S=256, Dh=128, d=256, ld=512) == lib_mod.E_UNSUPPORTED
        assert b"does not take" in L.genie_last_error()
    # the workspace: too small, or NULL where the path needs one -- for the path AUTO resolves to as well
    need = size(MAT, 3, 144, 2)
    assert call(wsb=need - 1) == lib_mod.E_ARG and b"workspace" in L.genie_last_error()
    assert call(ws=0) == lib_mod.E_ARG
    assert call(path=AUTO, wsb=need - 1) == lib_mod.E_ARG                                   # S = 144: materialised
    assert call(path=AUTO, S=256, Dh=128, d=256, ld=768, wsb=size(MAT, 3, 256, 2) - 1) == lib_mod.E_ARG   # head_dim 128: materialised
    assert call(path=BF16, S=256, wsb=size(BF16, 3, 256, 2) - 1) == lib_mod.E_ARG
    assert call(path=BF16, S=256, ws=0) == lib_mod.E_ARG

    def fwd(qkv=p, qkn=p, nw=p, nb=p, rows=5, H=2, Dh=32):
        return L.genie_qk_norm_forward(qkv, qkn, nw, nb, rows, H, Dh, 0)

    for k in ("qkv", "qkn", "nw", "nb"):
        assert fwd(**{k: 0}) == lib_mod.E_ARG, k
    assert fwd(rows=0) == lib_mod.E_ARG and fwd(H=0) == lib_mod.E_ARG and fwd(Dh=0) == lib_mod.E_ARG
    for Dh in (16, 48, 256):
        assert fwd(Dh=Dh) == lib_mod.E_UNSUPPORTED and b"head_dim" in L.genie_last_error()

    scratch = L.genie_qk_norm_backward_scratch_bytes
    assert [scratch(Dh) for Dh in (32, 64, 128, 16, 48)] == [513 * 2 * 32 * 4, 513 * 2 * 64 * 4, 513 * 2 * 128 * 4, 0, 0]

    def bwd(qkv=p, dqkv=p, nw=p, dnw=p, dnb=p, rows=5, H=2, Dh=32, sc=p, scb=1 << 20):
        return L.genie_qk_norm_backward(qkv, dqkv, nw, dnw, dnb, rows, H, Dh, 0, sc, scb, 0)

    for k in ("qkv", "dqkv", "nw"):
        assert bwd(**{k: 0}) == lib_mod.E_ARG, k
    assert bwd(rows=0) == lib_mod.E_ARG and bwd(H=-1) == lib_mod.E_ARG and bwd(Dh=0) == lib_mod.E_ARG
    for frozen in (dict(), dict(dnw=0), dict(dnb=0)):
        assert bwd(scb=scratch(32) - 1, **frozen) == lib_mod.E_ARG and b"scratch" in L.genie_last_error()
        assert bwd(sc=0, **frozen) == lib_mod.E_ARG
    for Dh in (16, 48):
        assert bwd(Dh=Dh) == lib_mod.E_UNSUPPORTED and bwd(Dh=Dh, dnw=0, dnb=0, sc=0, scb=0) == lib_mod.E_UNSUPPORTED
    assert L.genie_version() == 3


# ---------------------------------------------------------------------------------------------- the bars can fail
@pytest.mark.parametrize("Dh,ld3,q_mul", MUTANT_INPUTS)
def test_f32_bar_rejects_every_mutant(Dh, ld3, q_mul):
    """Each wrong variant of the restatement, run in f32 on a fused case's inputs, is over KERNEL_FACTOR x the floor in at least
    one block -- and the unchanged f32 restatement is not."""
    inp, ref, f32 = M.attn_case(256, Dh, ld3, q_mul)
    assert not M.accept_f32(f32, ref, f32)[1]
    mutants = M.MUTANTS_F32 + (() if ld3 else ("qk_from_qkv",))
    for mutant in mutants:
        seen, bad = M.accept_f32(M.attn_bwd_restated(*inp, np.float32, mutant=mutant), ref, f32)
        print(mutant, {k: f"{e / fl:.1f}x" for k, (e, fl) in seen.items()})
        assert bad, (mutant, seen)
    # each mutant fails where it should: D feeds dq and dk, not dv; the lost query block is in dk and dv, not dq
    assert set(M.accept_f32(M.attn_bwd_restated(*inp, np.float32, mutant="D_without_last_64_keys"), ref, f32)[1]) == {"dq", "dk"}
    assert set(M.accept_f32(M.attn_bwd_restated(*inp, np.float32, mutant="dkdv_without_last_query_block"), ref, f32)[1]) == {"dk", "dv"}


def test_f32_bar_rejects_the_mutants_at_a_materialised_shape():
    """The same on S = 144 inputs (qk_ld = 2 d), where the forced and the automatic materialised path are judged."""
    inp, ref, f32 = M.attn_case(144, 32, False, 4.0)
    for mutant in M.MUTANTS_F32 + ("qk_from_qkv",):
        assert M.accept_f32(M.attn_bwd_restated(*inp, np.float32, mutant=mutant), ref, f32)[1], mutant


@pytest.mark.parametrize("Dh,ld3,q_mul", MUTANT_INPUTS)
def test_bf16_bars_reject_every_mutant(Dh, ld3, q_mul):
    """The f32-accumulating number model stands in for the bf16 pair.  Unchanged it passes both assertions; with dS left unrounded,
    P rounded through f16 first, or any of the structural mistakes, it fails."""
    inp, ref, _ = M.attn_case(256, Dh, ld3, q_mul)
    model = M.bf16_model(256, Dh, ld3, q_mul)
    stand_in = M.attn_bwd_restated(*inp, np.float32, round=M.bf16)
    seen, bad = M.accept_bf16(stand_in, ref, model)
    print("stand-in", seen)
    assert not bad, bad
    for mutant in M.MUTANTS_BF16 + (() if ld3 else ("qk_from_qkv",)):
        seen, bad = M.accept_bf16(M.attn_bwd_restated(*inp, np.float32, round=M.bf16, mutant=mutant), ref, model)
        print(mutant, {k: f"{r:.3f}" for k, (_, _, r) in seen.items()})
        assert bad, (mutant, seen)


@pytest.mark.parametrize("Dh,rows,H", [(32, 37, 3), (64, 2100, 2), (128, 3, 1)])
def test_qk_norm_bar_rejects_every_mutant(Dh, rows, H):
    (qkv, dy, nw, nb), _, _, bwd, bwd32 = M.qk_norm_case(Dh, rows, H)
    names = ("d_qk", "d_norm_w", "d_norm_b")
    assert not M.accept_blocks(names, bwd32, bwd, bwd32)[1]
    for mutant, where in zip(M.MUTANTS_QKNORM, ({"d_qk"}, {"d_norm_w", "d_norm_b"})):
        seen, bad = M.accept_blocks(names, M.qk_norm_bwd_restated(qkv, dy, nw, H, np.float32, mutant=mutant), bwd, bwd32)
        assert set(bad) == where, (mutant, seen)


# ---------------------------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("S,Dh,ld3", [(256, 32, True), (256, 32, False), (256, 64, True), (256, 64, False), (144, 32, False),
                                      (144, 64, True), (16, 16, False), (16, 64, True), (16, 128, False)])
def test_sharp_inputs_are_sharp_and_no_block_is_degenerate(S, Dh, ld3):
    """q x 4: the float64 reference has no degenerate block (largest |dq| and |dk| at least 1e-3 of the largest |dv|), the rows are
    sharp (in the median row ONE key holds at least a quarter of the mass, and more than the q x 1 inputs' median row gives its
    largest) but not one-hot (in at most a tenth of the rows the largest probability exceeds 0.999, where dS would vanish)."""
    (qkv, qk, dO, H, scale), (dq, dk, dv), _ = M.attn_case(S, Dh, ld3, 4.0)
    assert np.abs(dq).max() >= 1e-3 * np.abs(dv).max() and np.abs(dk).max() >= 1e-3 * np.abs(dv).max()
    top = M.row_max_probability(qk, H, scale)
    flat = M.row_max_probability(M.attn_case(S, Dh, ld3, 1.0)[0][1], H, scale)
    print(S, Dh, ld3, "median top p", np.median(top), "flat", np.median(flat), "one-hot share", (top > 0.999).mean())
    assert np.median(top) >= 0.25 and np.median(top) > np.median(flat)
    assert (top > 0.999).mean() <= 0.1


def test_qk_ld_2d_inputs_differ_from_the_columns_of_qkv():
    for S, Dh in ((256, 32), (144, 64), (16, 16)):
        qkv, qk, *_ = M.kernel_inputs(S, Dh, False, 1.0)
        assert qk.shape[-1] == 2 * qkv.shape[-1] // 3 and qkv.shape[0] == 3
        assert np.abs(qk - qkv[..., :qk.shape[-1]]).min() > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("Dh,q_mul", [(32, 1.0), (32, 4.0), (64, 1.0), (64, 4.0)])
def test_f32_accumulating_bf16_model_sits_within_the_cap(Dh, q_mul, seed):
    """What stands in for the bf16 pair on the CPU -- the number model accumulating in f32 -- is within BF16_MODEL_SHARE_CAP of the
    float64-accumulating model, as a share of that model's Frobenius distance from float64.  Measured here at S = 256 over head_dim
    32 / 64, q x 1 / x 4 and three seeds: share 0.0000 .. 0.0171, the model's distance from float64 3.4e-3 .. 8.2e-3 of the block's norm."""
    inp, ref, _ = M.attn_case(256, Dh, True, q_mul, seed)
    model = M.bf16_model(256, Dh, True, q_mul, seed)
    stand_in = M.attn_bwd_restated(*inp, np.float32, round=M.bf16)
    for name, s, m, r in zip(("dq", "dk", "dv"), stand_in, model, ref):
        share, dist = M.fro(s.astype(np.float64) - m) / M.fro(m - r), M.fro(m - r) / M.fro(r)
        print(name, f"share {share:.4f} model distance {dist:.2e}")
        assert share <= M.BF16_MODEL_SHARE_CAP, (name, share)
        assert 1e-3 <= dist <= 2e-2, (name, dist)    # a bf16 operand rounding (2^-9) per product, averaged -- not 0, not f16-like


@pytest.mark.parametrize("Dh,rows,H", M.QKNORM_CASES)
def test_qk_norm_cases_have_the_item_counts_they_claim(Dh, rows, H):
    """Less than a block, no multiple of a block, or one full grid of the backward (512 blocks) plus at most a tenth; and the
    near-constant rows are there: eps is at least a hundred times their variance."""
    items, per_block = rows * 2 * H, 1024 // Dh
    grid = 512 * per_block
    assert items < per_block or items % per_block or grid < items <= 1.1 * grid
    kinds = {(d, "small" if r * 2 * h < 1024 // d else "ragged" if r * 2 * h < 512 * (1024 // d) else "second trip")
             for d, r, h in M.QKNORM_CASES}
    assert len(kinds) == 9
    qkv, *_ = M.qk_norm_inputs(Dh, rows, H)
    var = qkv[:, :2 * H * Dh].astype(np.float64).reshape(rows, 2 * H, Dh).var(-1)
    assert 3 <= int((var * 100 <= M.EPS).sum()) <= 5 and (var > 0).all()
