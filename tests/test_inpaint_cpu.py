"""CPU-only tests of decoding with known tokens (inpainting): the NumPy model (tests/inpaint_model.py) against the oracle where there are
no known tokens and its invariants where there are, and the C ABI additions -- exported and bound, the struct layout as the compiler sees
it, genie_mask_fraction bit for bit, the header as C99, the refusals before any HIP call, and every size function unchanged."""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO, pkg

torch = pytest.importorskip("torch")

import inpaint_model as M
from oracle import genie_oracle as O


def _lib():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    return lib_mod, lib_mod.load()


def small_cfg(**kw):
    args = dict(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    args.update(kw)
    return pkg("config").GenieConfig(**args)


def fake_logits_fn(cfg, seed):
    """logits (B, V, T, H, W) that depend on every token of the prompt, so a differing intermediate frame shows in the next step"""
    V = cfg.factored_vocab_size * cfg.num_factored_vocabs

    def fn(p):
        rng = np.random.default_rng([seed, int(p.sum() % (1 << 31)), int((p * np.arange(p.size).reshape(p.shape) % 977).sum() % (1 << 31))])
        return rng.standard_normal((p.shape[0], V) + p.shape[1:]).astype(np.float32)
    return fn


def draws(cfg, steps, B, seed):
    rng = np.random.default_rng(seed)
    noise = rng.random((max(steps - 1, 1), B, cfg.S), dtype=np.float32)
    uniforms = rng.random((steps, cfg.num_factored_vocabs, B, 4, 4), dtype=np.float32)
    return noise, uniforms


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("steps", [1, 2, 3, 4, 8])
def test_counts_without_known_tokens_are_the_oracles(steps):
    for S in (1, 16, 100, 256, 1024):
        assert M.counts(steps, S) == O.mask_counts(steps, S)
    assert M.counts(steps, 0) == [0] * (steps - 1)
    for m in range(1, 40):   # every non-final step leaves at least one and at most M tokens masked
        assert all(1 <= n <= m for n in M.counts(steps, m))


@pytest.mark.parametrize("mode,temperature", [("random", 0.0), ("greedy", 0.0), ("random", 1.0)])
@pytest.mark.parametrize("steps", [1, 2, 4])
def test_loop_without_known_tokens_is_the_oracles(steps, mode, temperature):
    cfg = small_cfg()
    B, T, mask = 3, cfg.T, cfg.image_vocab_size
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, mask, (B, T, 4, 4))
    prompt[:, 2:] = mask
    noise, uniforms = draws(cfg, steps, B, 7)
    seen_o, seen_m = [], []

    def recording(fn, log):
        def g(p):
            log.append(p[:, 2].copy())
            return fn(p)
        return g
    po, pm = prompt.copy(), prompt.copy()
    so, _ = O.maskgit_generate(po, 2, None, cfg, steps, temperature, mode, noise=noise, uniforms=uniforms if temperature else None,
                               logits_fn=recording(fake_logits_fn(cfg, 3), seen_o))
    for known in (None, np.full((B, 4, 4), mask), np.full((B, 4, 4), -1)):
        pm = prompt.copy()
        del seen_m[:]
        sm, unmasked, masked = M.generate_frame(pm, 2, known, cfg, steps, recording(fake_logits_fn(cfg, 3), seen_m), temperature, mode,
                                                noise, uniforms if temperature else None)
        assert np.array_equal(sm, so) and np.array_equal(pm, po)
        # the frame every pass saw is the oracle's: so `unmasked`, the complement of its masked positions, is too
        assert len(seen_m) == len(seen_o) and all(np.array_equal(a, b) for a, b in zip(seen_m, seen_o))
        if steps > 1:
            assert np.array_equal(unmasked, seen_o[-1].reshape(B, -1) != mask)
        assert [int(m[0]) for m in masked[:-1]] == O.mask_counts(steps, cfg.S)


def mixed_known(rng, B, S, mask):
    """(B, S) known tokens with K_b = 0, 1, S/2, S-1, S, ... per clip, at random positions"""
    kn = np.full((B, S), mask, dtype=np.int64)
    Ks = [0, 1, S // 2, S - 1, S]
    for b in range(B):
        pos = rng.permutation(S)[:Ks[b % len(Ks)]]
        kn[b, pos] = rng.integers(0, mask, len(pos))
    return kn


@pytest.mark.parametrize("mode,temperature", [("random", 0.0), ("greedy", 0.0), ("random", 1.0)])
@pytest.mark.parametrize("steps", [1, 2, 4, 8])
def test_invariants_with_known_tokens(steps, mode, temperature):
    cfg = small_cfg()
    B, S, mask = 5, cfg.S, cfg.image_vocab_size
    rng = np.random.default_rng(11)
    kn = mixed_known(rng, B, S, mask)
    k = M.is_known(kn, mask)
    prompt = rng.integers(0, mask, (B, cfg.T, 4, 4))
    prompt[:, 1:] = mask
    noise, uniforms = draws(cfg, steps, B, 13)
    s, unmasked, masked = M.generate_frame(prompt, 1, kn.reshape(B, 4, 4), cfg, steps, fake_logits_fn(cfg, 17), temperature, mode, noise,
                                           uniforms if temperature else None)
    s = s.reshape(B, S)
    assert np.array_equal(s[k], kn[k])                       # known positions are preserved
    assert not (s == mask).any() and s.min() >= 0            # no mask id in the output
    assert np.array_equal(prompt[:, 1].reshape(B, S), s)
    for b in range(B):                                       # each clip follows the schedule of ITS count
        assert [int(m[b]) for m in masked] == M.counts(steps, S - int(k[b].sum())) + [0]
    assert np.array_equal(s[4], kn[4])                       # the fully known clip is a fixed point
    if steps > 1:
        assert unmasked[k].all()


def test_start_state_and_schedule_independence():
    cfg = small_cfg()
    mask = cfg.image_vocab_size
    kn = np.array([[3, mask, -1, mask + 5, 0, mask - 1]])
    tokens, unmasked = M.start_state(kn, mask)
    assert tokens.tolist() == [[3, mask, mask, mask, 0, mask - 1]] and unmasked.tolist() == [[True, False, False, False, True, True]]
    # a clip decodes the same whatever shares its batch
    rng = np.random.default_rng(2)
    B, S = 5, cfg.S
    knb = mixed_known(rng, B, S, mask)
    samples = rng.integers(0, mask, (B, S))
    keys = rng.random((B, S), dtype=np.float32)
    frame, um = M.start_state(knb, mask)
    s_all, f_all, u_all = samples.copy(), frame.copy(), um.copy()
    M.mask_step(s_all, keys, u_all, knb, 0, 3, mask, f_all)
    for b in range(B):
        s1, f1, u1 = samples[b:b + 1].copy(), frame[b:b + 1].copy(), um[b:b + 1].copy()
        M.mask_step(s1, keys[b:b + 1], u1, knb[b:b + 1], 0, 3, mask, f1)
        assert np.array_equal(f1[0], f_all[b]) and np.array_equal(u1[0], u_all[b])


# ------------------------------------------------------------------ C ABI
NEW = ("genie_known_layout", "genie_mask_fraction", "genie_known_begin", "genie_mask_step_known", "genie_maskgit_generate_known",
       "genie_generate_cached_known", "genie_rollout_cached_known", "genie_generate_fanout_known")


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    assert "#define GENIE_ABI_VERSION 3" in header
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    for base, widest in (("genie_maskgit_generate", "genie_maskgit_generate_guided"), ("genie_generate_cached", "genie_generate_cached_guided"),
                         ("genie_rollout_cached", "genie_rollout_cached"), ("genie_generate_fanout", "genie_generate_fanout")):
        assert lib_mod.SIGNATURES[base + "_known"][1][:-1] == lib_mod.SIGNATURES[widest][1]
        assert lib_mod.SIGNATURES[base + "_known"][1][-1] is ctypes.POINTER(lib_mod.Known)
    assert "kernels_known.hip" in pkg("build").SOURCES


def test_known_layout_matches_the_ctypes_struct():
    lib_mod, L = _lib()
    out = (ctypes.c_size_t * 3)()
    assert L.genie_known_layout(out, 3) == 3
    F = lib_mod.Known
    assert list(out) == [ctypes.sizeof(F), F.ids.offset, F.clip_stride.offset] == [16, 0, 8]
    assert L.genie_known_layout(None, 0) == 3


def test_mask_fraction_is_pythons_bit_for_bit():
    _, L = _lib()
    for steps in range(1, 9):
        for s in range(steps):
            want = math.cos((s + 1) / steps * math.pi / 2)
            assert struct.pack("<d", L.genie_mask_fraction(s, steps)) == struct.pack("<d", want), (s, steps)
            assert want == M.fraction(s, steps)
    assert L.genie_mask_fraction(0, 0) == 0.0


def test_header_with_the_known_additions_compiles_as_c99(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if not gcc:
        pytest.skip("no C compiler")
    lib_mod, _ = _lib()
    src = tmp_path / "known.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_known k = {0, 32};\n"
                   "    int (*b)(const int64_t*, int64_t, int64_t, int64_t*, int64_t, uint8_t*, int, int, int, void*) = genie_known_begin;\n"
                   "    int (*m)(const float*, double, int, int64_t, const int64_t*, int64_t, uint8_t*, int64_t*, int64_t*, int64_t, int, int,\n"
                   "             void*) = genie_mask_step_known;\n"
                   "    int (*r)(const genie_cfg*, const genie_weights*, int64_t*, int, int, int, int, int, int, int, int, float, int,\n"
                   "             const float*, const float*, int, float*, size_t, void*, size_t, void*, const genie_frame_cond*,\n"
                   "             const genie_sampling*, const genie_guidance*, const genie_known*) = genie_rollout_cached_known;\n"
                   '    printf("%zu %zu %zu %d %.17g\\n", sizeof(genie_known), offsetof(genie_known, ids), offsetof(genie_known, clip_stride),\n'
                   "           (int)k.clip_stride + (b != 0) + (m != 0) + (r != 0), genie_mask_fraction(0, 2));\n"
                   "    return genie_known_layout(0, 0) != 3;\n}\n")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(REPO, "include"), "-c", str(src),
                    "-o", str(tmp_path / "known.o")], check=True)
    subprocess.run([gcc, str(tmp_path / "known.o"), lib_mod.LIB_PATH, f"-Wl,-rpath,{os.path.dirname(lib_mod.LIB_PATH)}", "-o",
                    str(tmp_path / "known")], check=True)
    out = subprocess.run([str(tmp_path / "known")], capture_output=True, text=True, check=True).stdout.split()
    F = lib_mod.Known
    assert [int(v) for v in out[:4]] == [ctypes.sizeof(F), F.ids.offset, F.clip_stride.offset, 35]
    assert float(out[4]) == math.cos(0.5 * math.pi / 2)


def test_known_entry_points_refuse_bad_arguments_before_any_hip_call():
    """ids == NULL and a clip_stride below frames x S: GENIE_E_ARG from host code, with a message that names the entry point and `known`
    (the fake device pointers are never dereferenced: nothing is enqueued)."""
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())   # T = 4, S = 16
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    fake, big = 1 << 20, 1 << 30
    K = lib_mod.Known

    def maskgit(k):
        return L.genie_maskgit_generate_known(cfg, w, fake, 1, 1, 1, 0.0, 0, None, None, fake, None, 0, None, fake, big, None, None, None,
                                              None, k)

    def cached(k):   # 2 new frames
        return L.genie_generate_cached_known(cfg, w, fake, 1, 2, 2, 1, 0.0, 0, None, None, 0, 1, fake, None, fake, big, fake, big, None,
                                             None, None, None, k)

    def rollout(k):   # frames [2, 5): 3 frames
        return L.genie_rollout_cached_known(cfg, w, fake, 1, 2, 2, 8, 2, 5, 0, 1, 0.0, 0, None, None, 1, fake, big, fake, big, None, None,
                                            None, None, k)

    def fanout(k):   # 2 new frames
        return L.genie_generate_fanout_known(cfg, w, fake, 1, 2, 2, 2, 1, 0.0, 0, None, None, 1, fake, fake, big, fake, big, fake, big,
                                             None, None, None, None, k)

    for call, name, frames in ((maskgit, b"maskgit_generate", 1), (cached, b"generate_cached", 2), (rollout, b"rollout_cached", 3),
                               (fanout, b"generate_fanout", 2)):
        for k in (K(0, frames * 16), K(fake, frames * 16 - 1), K(fake, 0), K(fake, -5)):
            assert call(k) == lib_mod.E_ARG, (name, k.ids, k.clip_stride)
            msg = L.genie_last_error()
            assert name in msg and b"known" in msg, msg
    E = lib_mod.E_ARG
    assert L.genie_known_begin(None, 16, 100, fake, 16, None, 1, 16, 1, None) == E
    assert L.genie_known_begin(fake, 16, 100, None, 16, None, 1, 16, 1, None) == E
    assert L.genie_known_begin(fake, 16, 100, fake, 16, None, 1, 16, 3, None) == E
    assert L.genie_known_begin(fake, 16, 100, fake, 16, None, 0, 16, 1, None) == E
    assert L.genie_mask_step_known(None, 0.5, 0, 100, fake, 16, fake, fake, fake, 16, 1, 16, None) == E     # keys required
    assert L.genie_mask_step_known(fake, 1.5, 0, 100, fake, 16, fake, fake, fake, 16, 1, 16, None) == E     # frac outside [0, 1]
    assert L.genie_mask_step_known(fake, float("nan"), 0, 100, fake, 16, fake, fake, fake, 16, 1, 16, None) == E
    assert L.genie_mask_step_known(fake, 0.5, 0, 100, fake, 16, None, fake, fake, 16, 1, 16, None) == E


def size_grid(L, c, T):
    """Every size function of the inference side on a grid of (B, P, K) (x guided), in one fixed order"""
    out = []
    for B in (1, 3):
        out += [L.genie_workspace_bytes(c, B), L.genie_prefix_cache_bytes(c, B)]
        for P in (1, T // 2, T - 1):
            out += [L.genie_generate_workspace_bytes(c, B, P), L.genie_generate_guided_workspace_bytes(c, B, P),
                    L.genie_rollout_workspace_bytes(c, B, P, 0), L.genie_rollout_workspace_bytes(c, B, P, 1)]
            for K in (1, 3):
                out += [L.genie_fanout_workspace_bytes(c, B, K, P, 0), L.genie_fanout_workspace_bytes(c, B, K, P, 1),
                        L.genie_fanout_branch_bytes(c, B, K, P), L.genie_score_workspace_bytes(c, B, K, P)]
    return out


def size_cases():
    C = pkg("config")

    def small(H, d, T, S, qk_norm, layers):
        return C.GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm, use_mup=False)
    return {"d64": small(2, 64, 8, 16, False, 2), "s144qk": small(2, 128, 4, 144, True, 2), "t8s256": small(2, 128, 8, 256, False, 1),
            "c35": C.c35()}


# size_grid of the four configs (the same in exact, bf16 and f16x3), read from the library of the commit before known tokens: known tokens add no buffer to any workspace
# (the mask step re-reads the clip's known row instead), so no size function may move
SIZES = {
    "d64": [
        754432, 196608, 754432, 1510400, 754432, 1510400, 754432, 1508096, 24576, 754432, 766464, 1530368, 73728, 766464,
        754432, 1510400, 754432, 1510400, 754432, 1508096, 98304, 754432, 766720, 1531136, 294912, 766720, 754432, 1510400,
        754432, 1510400, 754432, 1508096, 172032, 754432, 861184, 1719552, 516096, 861184, 2262016, 589824, 2262016, 4530176,
        2262016, 4530176, 2262016, 4523520, 73728, 2262016, 2296576, 4589312, 221184, 2296576, 2262016, 4530176, 2262016,
        4530176, 2262016, 4523520, 294912, 2262016, 2297600, 4591616, 884736, 2297600, 2262016, 4530176, 2262016, 4530176,
        2262016, 4523520, 516096, 2262016, 2580224, 5156608, 1548288, 2580224],
    "s144qk": [
        4425984, 1769472, 4425984, 8860928, 4425984, 8860928, 4425984, 8851456, 442368, 4425984, 8432640, 16857856, 1327104,
        8432640, 4425984, 8860928, 4425984, 8860928, 4425984, 8851456, 884736, 4425984, 8433664, 16860160, 2654208, 8433664,
        4425984, 8860928, 4425984, 8860928, 4425984, 8851456, 1327104, 4425984, 8434944, 16862464, 3981312, 8434944, 13276928,
        5308416, 13276928, 26581504, 13276928, 26581504, 13276928, 26553600, 1327104, 13276928, 25295872, 50572288, 3981312,
        25295872, 13276928, 26581504, 13276928, 26581504, 13276928, 26553600, 2654208, 13276928, 25299200, 50579200, 7962624,
        25299200, 13276928, 26581504, 13276928, 26581504, 13276928, 26553600, 3981312, 13276928, 25302784, 50586112, 11943936,
        25302784],
    "t8s256": [
        15731968, 3145728, 15731968, 31496960, 15731968, 31496960, 15731968, 31463936, 393216, 15731968, 15731968, 31463936,
        1179648, 15731968, 15731968, 31496960, 15731968, 31496960, 15731968, 31463936, 1572864, 15731968, 15731968, 31463936,
        4718592, 15731968, 15731968, 31496960, 15731968, 31496960, 15731968, 31463936, 2752512, 15731968, 16961024, 33911808,
        8257536, 16961024, 47195904, 9437184, 47195904, 94490624, 47195904, 94490624, 47195904, 94391808, 1179648, 47195904,
        47195904, 94391808, 3538944, 47195904, 47195904, 94490624, 47195904, 94490624, 47195904, 94391808, 4718592, 47195904,
        47195904, 94391808, 14155776, 47195904, 47195904, 94490624, 47195904, 94490624, 47195904, 94391808, 8257536, 47195904,
        50882560, 101734912, 24772608, 50882560],
    "c35": [
        46140672, 402653184, 46140672, 92347136, 46140672, 92347136, 46140672, 92281344, 25165824, 46140672, 46140672, 92281344,
        75497472, 46140672, 46140672, 92347136, 46140672, 92347136, 46140672, 92281344, 201326592, 46140672, 46140672, 92281344,
        603979776, 46140672, 46140672, 92347136, 46140672, 92347136, 46140672, 92281344, 377487360, 46140672, 46468864,
        92927232, 1132462080, 46468864, 138422016, 1207959552, 138422016, 277041408, 138422016, 277041408, 138422016, 276844032,
        75497472, 138422016, 138422016, 276844032, 226492416, 138422016, 138422016, 277041408, 138422016, 277041408, 138422016,
        276844032, 603979776, 138422016, 138422016, 276844032, 1811939328, 138422016, 138422016, 277041408, 138422016,
        277041408, 138422016, 276844032, 1132462080, 138422016, 139406080, 278781696, 3397386240, 139406080],
}


def test_every_size_function_is_unchanged():
    lib_mod, L = _lib()
    cases = size_cases()
    assert sorted(cases) == sorted(SIZES)
    for name, cfg in cases.items():
        for prec in (lib_mod.PREC_EXACT, lib_mod.PREC_BF16, lib_mod.PREC_F16X3):
            got = size_grid(L, lib_mod.make_cfg(cfg, prec), cfg.T)
            assert len(got) == len(SIZES[name]) == 2 * (2 + 3 * (4 + 2 * 4)) and all(v > 0 for v in got), name
            assert got == SIZES[name], (name, prec)


# ------------------------------------------------------------------ the Python helpers and the CLI flag
def test_known_tokens_and_check_known():
    G = pkg("generate")
    frames = torch.arange(2 * 3 * 4 * 4).view(2, 3, 4, 4)
    keep = torch.zeros(4, 4, dtype=torch.bool)
    keep[1:3, 0:3] = True
    kn = G.known_tokens(frames, keep, 1000)
    assert kn.dtype == torch.int64 and kn.is_contiguous() and torch.equal(kn[..., 1:3, 0:3], frames[..., 1:3, 0:3])
    assert int((kn == 1000).sum()) == 2 * 3 * 10
    full = torch.zeros(2, 3, 4, 4, dtype=torch.bool)
    full[1, 2] = True
    kn = G.known_tokens(frames.to(torch.int32), full, 1000)
    assert kn.dtype == torch.int64 and torch.equal(kn[1, 2], frames[1, 2]) and int((kn != 1000).sum()) == 16
    for bad in (keep.to(torch.uint8), torch.zeros(3, 4, 4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match="keep"):
            G.known_tokens(frames, bad, 1000)
    assert G.check_known(None, (1,), "cpu") is None
    assert G.check_known(kn, (2, 3, 4, 4), "cpu") is kn
    for bad, shape in ((kn.to(torch.int32), (2, 3, 4, 4)), (kn, (2, 3, 16)), (kn.numpy(), (2, 3, 4, 4))):
        with pytest.raises(RuntimeError, match="known"):
            G.check_known(bad, shape, "cpu")
    with pytest.raises(RuntimeError, match="known"):
        G.check_known(kn, (2, 3, 4, 4), "cuda:0")


def test_known_box_flag():
    import importlib.util
    from types import SimpleNamespace
    spec = importlib.util.spec_from_file_location("tool_generate", os.path.join(REPO, "tools", "generate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    G = pkg("generate")
    model = SimpleNamespace(h=4, w=4, mask_token_id=1000)
    ex = torch.arange(8 * 16).view(1, 8, 4, 4)

    def box(text, N=5):
        args = tool.build_parser().parse_args(["--known_box", text, "--num_prompt_frames", "3", "--window_size", "8"])
        return tool.known_box(args, model, ex, G, N)
    kn = box("1,0,2,3")
    assert kn.shape == (1, 5, 4, 4) and torch.equal(kn[..., 1:3, 0:3], ex[:, 3:, 1:3, 0:3]) and int((kn == 1000).sum()) == 5 * 10
    assert torch.equal(box("0,0,4,4"), ex[:, 3:])
    assert tool.known_box(tool.build_parser().parse_args([]), model, ex, G, 5) is None
    for bad in ("1,0,2", "a,b,c,d", "3,0,2,3", "0,0,0,1", "-1,0,2,2", "0,2,1,3"):
        with pytest.raises(SystemExit):
            box(bad)
    with pytest.raises(SystemExit):      # no ground truth behind the example's frames
        box("1,0,2,3", N=6)
