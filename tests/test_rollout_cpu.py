"""CPU-only tests of the rollout past the context window: the window schedule, the C ABI additions (exported, bound, argument errors
before any HIP call, the workspace size) and the CLI flags."""
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


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("T,P,keep,N", [(8, 3, 2, 15), (8, 3, 7, 4), (16, 8, 8, 40), (8, 7, 1, 9)])
def test_window_schedule_follows_the_formulas(T, P, keep, N):
    """Every generated frame f gets j = 0 below T, else 1 + (f - T) // hop, start = j * hop, slot = f - start; its context is
    [start, f); the windows tile [P, P + N) without gap or overlap."""
    G = pkg("generate")
    hop = T - keep
    wins = G.window_schedule(P, keep, T, N)
    covered = []
    for n, (j, start, fb, fe) in enumerate(wins):
        assert fb < fe and start == j * hop
        assert fe - fb <= (T - P if j == 0 else hop)
        assert fb - start == (P if j == 0 else keep)          # the context the window runs before its first frame
        covered += list(range(fb, fe))
        if n:
            assert j == wins[n - 1][0] + 1 and fb == wins[n - 1][3]
        if n + 1 < len(wins):
            assert fe == start + T                            # only the last window is partial
    assert covered == list(range(P, P + N))
    for f in range(P, P + N):
        j = 0 if f < T else 1 + (f - T) // hop
        slot = f - j * hop
        assert G.frame_window(f, P, keep, T) == (j, j * hop, slot)
        assert (P if j == 0 else keep) <= slot < T
        win = [w for w in wins if w[2] <= f < w[3]]
        assert len(win) == 1 and win[0][:2] == (j, j * hop)   # context range [start, f) = slots 0 .. slot - 1
    sizes = [fe - fb for _, _, fb, fe in wins]
    if (T, P, keep, N) == (8, 3, 2, 15):
        assert sizes == [5, 6, 4]
    if (T, P, keep, N) == (8, 3, 7, 4):
        assert sizes == [4]
    if (T, P, keep, N) == (8, 7, 1, 9):
        assert sizes == [1, 7, 1]


def test_window_schedule_hop_one_and_bad_arguments():
    G = pkg("generate")
    assert [w[2:] for w in G.window_schedule(7, 7, 8, 4)] == [(7, 8), (8, 9), (9, 10), (10, 11)]     # every frame its own window
    assert G.window_schedule(3, 2, 8, 0) == []
    for P, keep in ((0, 2), (8, 2), (3, 0), (3, 8)):
        with pytest.raises(ValueError):
            G.window_schedule(P, keep, 8, 4)


# ------------------------------------------------------------------ C ABI
NEW = ("genie_rollout_cached", "genie_rollout_workspace_bytes")


def test_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib_mod, L = _lib()
    assert L.genie_version() == 3 and lib_mod.ABI_VERSION == 3
    header = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    for n in NEW:
        assert hasattr(L, n) and n in lib_mod.SIGNATURES and n + "(" in header, n
    assert "GENIE_ABI_VERSION 3" in header
    G = pkg("generate")
    for n in ("rollout_frames", "Rollout", "window_schedule"):
        assert hasattr(G, n), n
    assert hasattr(pkg("st_mask_git").STMaskGIT, "rollout")


def test_rollout_rejects_bad_arguments_before_any_hip_call():
    """GENIE_E_ARG from host code with NULL device pointers: the range checks come before the pointers are looked at, and the message
    names the argument."""
    lib_mod, L = _lib()
    cfg = lib_mod.make_cfg(small_cfg())           # T = 8
    w = lib_mod.Weights()
    layers = (lib_mod.LayerWeights * 1)()
    w.layers_host = layers
    E = lib_mod.E_ARG
    fake = 1 << 20

    def call(P=3, keep=2, cap=20, f0=3, f1=10, resume=0, steps=2, temperature=0.0, mode=1, uniforms=None, cond=None, guide=None,
             frames=None, cache=None, ws=None):
        return L.genie_rollout_cached(cfg, w, frames, 3, P, keep, cap, f0, f1, resume, steps, temperature, mode, None, uniforms, 1, cache,
                                      1 << 40, ws, 1 << 40, None, cond, None, guide)

    for kw, word in ((dict(keep=0), b"keep"), (dict(keep=8), b"keep"), (dict(P=8, f0=8), b"prompt"), (dict(P=9, f0=9), b"prompt"),
                     (dict(P=0, f0=1), b"prompt"), (dict(f0=2), b"frames ["), (dict(f1=21), b"frames ["), (dict(f0=10, f1=10), b"frames ["),
                     (dict(f0=11, f1=10), b"frames ["), (dict(resume=2), b"resume"), (dict(temperature=1.0), b"uniforms"),
                     (dict(mode=0), b"draws"), (dict(steps=0), b"steps")):
        assert call(**kw) == E, kw
        assert word in L.genie_last_error(), (kw, L.genie_last_error())
    uncond = lib_mod.FrameCond(table=0, ids=0, n_actions=0)
    no_table = lib_mod.FrameCond(table=0, ids=fake, n_actions=5)
    cond = lib_mod.FrameCond(table=fake, ids=fake, n_actions=5)
    for c, g in ((None, lib_mod.Guidance(3.0, 0)), (uncond, lib_mod.Guidance(3.0, 0)), (cond, lib_mod.Guidance(3.0, 5))):
        assert call(cond=c, guide=g) == E
        assert b"guidance" in L.genie_last_error()
    assert call(cond=no_table, guide=lib_mod.Guidance(3.0, 0)) == E and b"table" in L.genie_last_error()
    # everything in range: the NULL device pointers are what is refused next -- still before any HIP call
    assert call() == E and b"NULL pointer" in L.genie_last_error()
    assert call(frames=fake, cache=fake) == E and b"workspace" in L.genie_last_error()


def test_rollout_workspace_covers_the_generate_loops():
    lib_mod, L = _lib()
    for cfg in (lib_mod.make_cfg(small_cfg()), lib_mod.make_cfg(small_cfg(T=16, S=64, d_model=64))):
        T = cfg.T
        for B in (1, 3, 16):
            for ctx in (1, 2, 5, T - 1):
                n = L.genie_rollout_workspace_bytes(cfg, B, ctx, 0)
                assert n >= L.genie_generate_workspace_bytes(cfg, B, ctx) > 0
                assert n >= L.genie_workspace_bytes(cfg, B)
                g = L.genie_rollout_workspace_bytes(cfg, B, ctx, 1)
                assert g >= L.genie_generate_guided_workspace_bytes(cfg, B, ctx) > 0
                assert g >= n
        for bad in ((0, 1, 0), (1, 0, 0), (1, T, 0), (1, -1, 1), (-2, 3, 1)):
            assert L.genie_rollout_workspace_bytes(cfg, *bad) == 0, bad
    assert L.genie_rollout_workspace_bytes(None, 1, 1, 0) == 0


# ------------------------------------------------------------------ Python surface and the CLI
def test_rollout_arguments_are_checked_on_the_host():
    """Before the device is touched: keep and the prompt length against the window, actions against the model."""
    G = pkg("generate")
    m = pkg("st_mask_git").STMaskGIT(small_cfg())
    prompt = torch.zeros(2, 3, 4, 4, dtype=torch.long)
    for kw in (dict(keep=0), dict(keep=8)):
        with pytest.raises(ValueError):
            G.rollout_frames(m, prompt, 4, **kw)
    with pytest.raises(ValueError):
        G.rollout_frames(m, torch.zeros(2, 8, 4, 4, dtype=torch.long), 4)          # P = T
    with pytest.raises(ValueError):
        G.rollout_frames(m, prompt, 0)
    with pytest.raises(ValueError):
        G.rollout_frames(m, prompt, 4, action_ids=torch.zeros(2, 7, dtype=torch.long))   # a model without actions
    ma = pkg("st_mask_git").STMaskGIT(small_cfg(action_vocab_size=5))
    with pytest.raises(ValueError):
        ma.rollout(prompt, 4)
    with pytest.raises(RuntimeError):
        ma.rollout(prompt, 4, action_ids=torch.zeros(2, 8, dtype=torch.long))      # (B, T) is not (B, P + n_new)
    with pytest.raises(IndexError):
        ma.rollout(prompt, 4, action_ids=torch.full((2, 7), 5))
    with pytest.raises(ValueError):
        G.Rollout(m, prompt, keep=8)


def test_generate_tool_lists_the_rollout_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "generate.py"), "--help"], capture_output=True, text=True, check=True)
    assert "--num_new_frames" in out.stdout and "--keep" in out.stdout
    text = open(os.path.join(REPO, "tools", "bench_generate.py")).read()
    assert "--rollout" in text
