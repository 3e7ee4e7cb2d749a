"""CPU-only tests of the sampling law (temperature, top-k, top-p, "confidence" unmasking): the f64 model against itself, the C ABI
additions (exported, struct layout as the compiler sees it, argument errors before any HIP call), the built kernels' scratch,
SamplingConfig validation and the CLI flags."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest

import sampling_model as SM
from conftest import REPO, pkg

VF = 512


def _inputs(rows=6, S=32, seed=17):
    g = np.random.default_rng(seed)
    logits = (g.standard_normal((rows, S, 2 * VF)) * 2.5).astype(np.float32)
    uni = g.random((2, rows, S), dtype=np.float32)
    return logits, uni


# ------------------------------------------------------------------ the f64 model against itself
def test_model_top_k_1_and_tiny_top_p_equal_argmax():
    logits, uni = _inputs()
    logits[0, :, 100] = logits[0, :, 300] = 20.0          # ties: the first maximum wins
    want = logits[..., VF:].argmax(-1) * VF + logits[..., :VF].argmax(-1)
    for kw in (dict(top_k=1), dict(top_p=1e-9), dict(tau=0.7, top_k=1, top_p=0.5)):
        got = SM.sample(logits, uni, VF, **kw)
        assert np.array_equal(got["ids"], want), kw
    assert np.array_equal(SM.sample(logits, uni, VF, tau=1.3, top_k=50, top_p=0.9, temperature=0.0)["ids"], want)


def test_model_kept_sets_nest():
    logits, _ = _inputs(rows=3)
    l = logits[..., :VF]
    prev = None
    for k in (1, 2, 8, 50, 511, 512, 0):
        kept = SM.factor_law(l, 0.7, k, 1.0)["kept"]
        assert (kept.sum(-1) == (k if 0 < k < VF else VF)).all()
        if prev is not None:
            assert (kept | ~prev).all(), k
        prev = kept
    prev = None
    for p in (1e-6, 0.1, 0.5, 0.9, 0.999, 1.0):
        kept = SM.factor_law(l, 1.3, 50, p)["kept"]
        assert kept.any(-1).all() and (kept.sum(-1) <= 50).all()
        if prev is not None:
            assert (kept | ~prev).all(), p
        prev = kept
    # the kept mass reaches top_p, and dropping the worst kept entry would fall short of it
    law = SM.factor_law(l, 1.0, 0, 0.9)
    p = law["e"] / law["e"].sum(-1, keepdims=True)
    mass = np.where(law["kept"], p, 0).sum(-1)
    worst = np.where(law["kept"], p, np.inf).min(-1)
    assert (mass >= 0.9 - 1e-12).all() and (mass - worst < 0.9).all()


def test_model_all_off_equals_the_plain_inverse_cdf():
    logits, uni = _inputs()
    ids, amb = SM.plain_inverse_cdf(logits, uni, VF)
    for kw in (dict(), dict(top_k=VF), dict(top_k=4096, top_p=1.5), dict(top_p=0.0), dict(top_p=-1.0)):
        got = SM.sample(logits, uni, VF, **kw)
        assert np.array_equal(got["ids"], ids), kw
        assert np.array_equal(got["ambiguous"], amb), kw


def test_model_ambiguous_shares_are_small():
    """The shares the GPU test caps at 1 %, on its own inputs (a smaller slice of them here)."""
    g = np.random.default_rng(17)
    logits = (g.standard_normal((24, 256, 1024)) * 2.5).astype(np.float32)[:4]
    uni = g.random((2, 24, 256), dtype=np.float32)[:, :4]
    for tau, k, p in [(0.7, 0, 1.0), (1.3, 50, 1.0), (1.0, 0, 0.9), (0.7, 8, 0.5), (1.3, 50, 0.95), (1.0, 1, 1.0), (2.0, 0, 0.3)]:
        r = SM.sample(logits, uni, VF, tau, k, p)
        assert r["ambiguous"].mean() < 0.01, (tau, k, p, r["ambiguous"].mean())
        for pick, law in zip(r["picks"], r["laws"]):
            assert np.take_along_axis(law["kept"], pick[..., None], -1).all()


def test_model_confidence_keys():
    conf = np.array([0.5, 0.25, 1e-30])
    u = np.array([0.0, 0.5, 1.0])
    k0 = SM.confidence_keys(conf, u, 0.0, 0, 4)
    assert np.array_equal(k0, np.log(conf)) and np.array_equal(np.argsort(k0), np.argsort(conf))
    k = SM.confidence_keys(conf, u, 4.5, 0, 4)
    assert np.isfinite(k).all()
    assert np.array_equal(SM.confidence_keys(conf, u, 4.5, 3, 4), np.log(conf))    # the last step's anneal factor is 0


# ------------------------------------------------------------------ SamplingConfig and the CLI
def test_sampling_config_validation():
    S = pkg("sampling")
    c = S.SamplingConfig()
    assert (c.logit_temperature, c.top_k, c.top_p, c.choice_temperature) == (1.0, 0, 1.0, 4.5)
    assert c.is_neutral() and S.SamplingConfig(top_k=512).is_neutral(512) and S.SamplingConfig(top_p=0.0).is_neutral()
    assert not S.SamplingConfig(top_k=5).is_neutral(512) and not S.SamplingConfig(logit_temperature=0.7).is_neutral()
    for bad in (dict(logit_temperature=0.0), dict(logit_temperature=-1.0), dict(logit_temperature=float("inf")),
                dict(logit_temperature=float("nan")), dict(top_k=-1), dict(top_k=1.5), dict(top_p=float("nan")),
                dict(choice_temperature=-0.1), dict(choice_temperature=float("nan"))):
        with pytest.raises(ValueError):
            S.SamplingConfig(**bad)
    with pytest.raises(ValueError):
        S.as_struct("top_k=5")
    with pytest.raises(NotImplementedError):
        S.unmask_code("sorted")
    assert S.as_struct(None) is None
    st = S.as_struct(S.SamplingConfig(0.7, 50, 0.9, 2.0))
    assert (round(st.logit_temperature, 6), st.top_k, round(st.top_p, 6), st.choice_temperature) == (0.7, 50, 0.9, 2.0)
    # namespaces that predate the fields
    assert S.SamplingConfig.from_args(SimpleNamespace(maskgit_steps=2, temperature=0)) is None
    assert S.SamplingConfig.from_args(SimpleNamespace(top_k=None, top_p=None)) is None
    assert S.SamplingConfig.from_args(SimpleNamespace(top_k=8)) == S.SamplingConfig(top_k=8)


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tool", ["generate", "evaluate"])
def test_cli_flags_parse(tool):
    S = pkg("sampling")
    ap = _tool(tool).build_parser()
    a = ap.parse_args(["--top_k", "50", "--top_p", "0.9", "--logit_temperature", "0.7", "--unmask_mode", "confidence",
                       "--choice_temperature", "3", "--temperature", "1"])
    assert S.SamplingConfig.from_args(a) == S.SamplingConfig(0.7, 50, 0.9, 3.0) and a.unmask_mode == "confidence"
    a = ap.parse_args([])
    assert S.SamplingConfig.from_args(a) is None and a.unmask_mode == "random" and a.temperature == 0
    with pytest.raises(SystemExit):
        ap.parse_args(["--unmask_mode", "sorted"])
    help_text = ap.format_help()
    assert "does NOT temper" in " ".join(help_text.split())


def test_evaluator_reads_the_law_with_defaults():
    E = pkg("evaluate").GenieEvaluator
    S = pkg("sampling")
    ev = E.__new__(E)
    ev.args = SimpleNamespace(maskgit_steps=2, temperature=0)
    assert ev._sampling() == (None, "random")
    ev.args = SimpleNamespace(maskgit_steps=2, temperature=1.0, top_k=50, logit_temperature=0.7, unmask_mode="confidence")
    assert ev._sampling() == (S.SamplingConfig(logit_temperature=0.7, top_k=50), "confidence")


# ------------------------------------------------------------------ C ABI
def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def small_cfg(**kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    for n in ("genie_sample_ex", "genie_maskgit_generate_ex", "genie_generate_cached_ex", "genie_sampling_layout"):
        assert hasattr(L, n) and n in lib_mod.SIGNATURES, n
    for base in ("genie_maskgit_generate", "genie_generate_cached"):
        assert lib_mod.SIGNATURES[base + "_ex"][1][:-1] == lib_mod.SIGNATURES[base + "_cond"][1]
        assert lib_mod.SIGNATURES[base + "_ex"][1][-1] is ctypes.POINTER(lib_mod.Sampling)
    assert lib_mod.SIGNATURES["genie_sample_ex"][1][:9] == lib_mod.SIGNATURES["genie_sample"][1]
    assert L.genie_abi_layout(None, 0) == 12
    assert lib_mod.UNMASK_CONFIDENCE == 2


def test_sampling_layout_matches_the_ctypes_struct():
    lib_mod, L = _lib()
    out = (ctypes.c_size_t * 5)()
    assert L.genie_sampling_layout(out, 5) == 5
    F = lib_mod.Sampling
    assert list(out) == [ctypes.sizeof(F), F.logit_temperature.offset, F.top_k.offset, F.top_p.offset, F.choice_temperature.offset]
    assert list(out) == [16, 0, 4, 8, 12]


def test_ex_entry_points_reject_bad_arguments_before_any_hip_call():
    """Every check below returns GENIE_E_ARG from host code: the fake device pointers are never dereferenced."""
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    fake = 1 << 20   # never read
    E = lib_mod.E_ARG
    nan, inf = float("nan"), float("inf")
    bad_laws = [lib_mod.Sampling(0.0, 0, 1.0, 4.5), lib_mod.Sampling(-1.0, 0, 1.0, 4.5), lib_mod.Sampling(inf, 0, 1.0, 4.5),
                lib_mod.Sampling(nan, 0, 1.0, 4.5), lib_mod.Sampling(1.0, -1, 1.0, 4.5), lib_mod.Sampling(1.0, 0, nan, 4.5),
                lib_mod.Sampling(1.0, 0, 1.0, -0.5), lib_mod.Sampling(1.0, 0, 1.0, nan)]
    good = lib_mod.Sampling(0.7, 50, 0.9, 4.5)

    def sample(law, keys=None, noise=None):
        return L.genie_sample_ex(cfg, fake, 0, 1, 1.0, fake, fake, fake, None, law, keys, noise, 0.5)

    def maskgit(law, mode, steps, noise):
        return L.genie_maskgit_generate_ex(cfg, w, fake, 1, 1, steps, 1.0, mode, noise, fake, fake, None, 0, None, fake, 1 << 30,
                                           None, None, law)

    def cached(law, mode, steps, noise):
        return L.genie_generate_cached_ex(cfg, w, fake, 1, 2, 1, steps, 1.0, mode, noise, fake, 0, 1, fake, None, fake, 1 << 30,
                                          fake, 1 << 30, None, None, law)

    for law in bad_laws:
        assert sample(law) == E
        assert b"sampling" in L.genie_last_error()
        assert maskgit(law, 0, 1, None) == E
        assert cached(law, 0, 1, None) == E
    # keys without the draws they are made from
    assert sample(good, keys=fake, noise=None) == E
    # "confidence" with steps > 1 and no noise
    assert maskgit(good, lib_mod.UNMASK_CONFIDENCE, 2, None) == E and b"confidence" in L.genie_last_error()
    assert cached(good, lib_mod.UNMASK_CONFIDENCE, 2, None) == E and b"confidence" in L.genie_last_error()
    assert maskgit(None, lib_mod.UNMASK_CONFIDENCE, 2, None) == E
    # the entry points of before do not know the new mode
    assert L.genie_maskgit_generate_cond(cfg, w, fake, 1, 1, 2, 0.0, lib_mod.UNMASK_CONFIDENCE, fake, None, fake, None, 0, None, fake,
                                         1 << 30, None, None) == lib_mod.E_UNSUPPORTED
    assert L.genie_generate_cached_cond(cfg, w, fake, 1, 2, 1, 2, 0.0, lib_mod.UNMASK_CONFIDENCE, fake, None, 0, 1, fake, None, fake,
                                        1 << 30, fake, 1 << 30, None, None) == lib_mod.E_UNSUPPORTED


def test_python_raises_value_error_on_a_bad_law():
    """The module-level entry points validate the law on the host (no GPU needed to reach the check)."""
    M = pkg("st_mask_git").STMaskGIT
    m = M(small_cfg())
    import torch
    prompt = torch.zeros(1, 4, 4, 4, dtype=torch.long)
    with pytest.raises(ValueError):
        m.maskgit_generate(prompt, 1, sampling={"top_k": 5})
    with pytest.raises(NotImplementedError):
        m.maskgit_generate(prompt, 1, unmask_mode="sorted")
    with pytest.raises(ValueError):
        m.generate(prompt.view(1, -1)[:, :32], max_new_tokens=16, sampling=3)


# ------------------------------------------------------------------ the built kernels
def test_filtered_sample_kernels_use_no_scratch():
    """The built code object: the row kernel keeps a factor's 512 values in registers through every pass (a loop left rolled would
    index them dynamically and spill), the strided one re-reads them; neither uses scratch."""
    LLVM = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    lib_mod, _ = _lib()
    audit = _tool("isa_audit")
    rows = {r[0]: r for r in audit.audit(lib_mod.LIB_PATH, all_kernels=True)}
    got = {k: v for k, v in rows.items() if "sample_filtered" in k}
    assert any("sample_filtered_rows_kernel<8>" in k for k in got) and any("sample_filtered_kernel" in k for k in got), list(got)
    for name, r in got.items():
        assert r[6] == 0, f"{name}: {r[6]} bytes of scratch per lane"
        assert r[7] <= 128, f"{name}: {r[7]} registers (4 waves per SIMD need <= 128)"
