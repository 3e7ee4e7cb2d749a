"""CPU-only: the C-ABI library loads and exports every symbol include/genie_hip.h declares; argument checks
that need no GPU; host-side logic (config, synthetic weights, sharding)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, pkg


def declared_symbols():
    src = open(os.path.join(REPO, "include", "genie_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(genie_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib_mod = pkg("_lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        pkg("build").build()
    L = lib_mod.load()
    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"{n} declared in genie_hip.h but not exported"
        assert n in lib_mod.SIGNATURES, f"{n} has no ctypes signature in _lib.py"
    assert sorted(lib_mod.SIGNATURES) == names
    assert L.genie_version() == 3


def test_struct_layout_matches_header():
    """The ctypes declarations of _lib.py against the COMPILER's layout of include/genie_hip.h (genie_abi_layout): sizes of the
    four POD structs and the offsets of the fields ABI versions 2 and 3 added (fused streams, f16x3 range flags, frame streams)."""
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    out = (ctypes.c_size_t * 12)()
    assert L.genie_abi_layout(out, 12) == 12
    A, LW, W = lib_mod.AttnWeights, lib_mod.LayerWeights, lib_mod.Weights
    mine = [ctypes.sizeof(lib_mod.GenieCfg), ctypes.sizeof(A), A.fused_w16.offset, A.w16_wide.offset, ctypes.sizeof(LW),
            LW.mlp_fused_w16.offset, LW.w16_wide.offset, ctypes.sizeof(W), W.out_w16_wide.offset, A.frame_w16.offset,
            LW.mlp_frame_w16.offset, W.out_frame_w16.offset]
    assert list(out) == mine, (list(out), mine)
    assert ctypes.sizeof(lib_mod.GenieCfg) == 18 * 4


def test_config_checks_without_gpu():
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    C = pkg("config")
    ok = lib_mod.make_cfg(C.c138())
    assert L.genie_check_config(ok) == 0
    assert L.genie_workspace_bytes(ok, 1) > 4096 * 512 * 4 * 2
    assert L.genie_workspace_bytes(ok, 2) > L.genie_workspace_bytes(ok, 1)
    bad = lib_mod.make_cfg(C.GenieConfig(num_layers=1, num_heads=3, d_model=96 * 3, num_factored_vocabs=2))
    assert L.genie_check_config(bad) == lib_mod.E_SHAPE  # head_dim 96 unsupported
    assert b"head_dim" in L.genie_last_error()
    assert L.genie_workspace_bytes(bad, 1) == 0
    # NULL / range checks fire before any HIP call
    assert L.genie_layer_norm(0, 0, 0, 0, 4, 64, 1e-5, 0) == lib_mod.E_ARG
    assert L.genie_mask_step(0, 3, 0, 262144, 0, 0, 0, 0, 1, 256, 0) == lib_mod.E_ARG
    with pytest.raises(lib_mod.GenieHipError):
        lib_mod.check(L.genie_linear(0, 0, 0, 0, 1, 1, 16, 0, 0, 0), "genie_linear")


def test_config_check_refuses_inconsistent_vocabulary():
    """genie_check_config: image_vocab_size (the mask id) must be factored_vocab ^ num_factored -- else a sampled id hi * vf + lo
    can reach or pass the mask id.  The power is formed without overflow (factored_vocab up to 2^31 - 1, four factors)."""
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    C = pkg("config")
    for iv, nv in [(262144, 1), (262144, 2), (262144, 3), (65536, 4), (10000, 2), (4096, 1), (1, 4)]:
        c = lib_mod.make_cfg(C.GenieConfig(num_layers=1, num_heads=2, d_model=64, T=4, S=16, image_vocab_size=iv,
                                           num_factored_vocabs=nv))
        assert L.genie_check_config(c) == 0, (iv, nv, L.genie_last_error())
        assert L.genie_workspace_bytes(c, 1) > 0
    ok = lib_mod.make_cfg(C.c35())
    for vf, nv, iv in [(512, 2, 262143), (512, 2, 262145), (512, 2, 512), (512, 1, 262144), (64, 3, 262144 * 64),
                       (100, 2, 10001), (2 ** 31 - 1, 2, 2 ** 31 - 1), (2 ** 31 - 1, 4, 1), (65536, 2, 0), (46341, 2, 2 ** 31 - 1)]:
        bad = lib_mod.make_cfg(C.c35())
        bad.factored_vocab, bad.num_factored, bad.image_vocab_size = vf, nv, iv
        assert L.genie_check_config(bad) == lib_mod.E_SHAPE, (vf, nv, iv)
        assert b"image_vocab_size" in L.genie_last_error()
        assert L.genie_workspace_bytes(bad, 1) == 0
        assert L.genie_generate_workspace_bytes(bad, 1, 2) == 0
    assert L.genie_check_config(ok) == 0


def test_workspace_holds_the_16bit_scratch_when_the_vocabulary_is_narrower_than_d():
    """The 16-bit blocks' generic attention kernels write an (M, d) f32 scratch into the logits region of the workspace: with
    V < d that region (and hence the workspace) must grow to M * d floats, while V >= d keeps its size."""
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    C = pkg("config")

    def ws(**kw):
        c = lib_mod.make_cfg(C.GenieConfig(num_layers=1, num_heads=kw["d_model"] // 64, T=4, S=64, **kw))
        c.precision = lib_mod.PREC_BF16
        assert L.genie_check_config(c) == 0, L.genie_last_error()
        return L.genie_workspace_bytes(c, 1), L.genie_generate_workspace_bytes(c, 1, 2)

    M = 4 * 64
    for d in (256, 1536):
        narrow, gen_narrow = ws(d_model=d, image_vocab_size=64 ** 3, num_factored_vocabs=3)   # V = 192 < d
        assert gen_narrow >= narrow
        assert ws(d_model=d, image_vocab_size=16, num_factored_vocabs=1)[0] == narrow      # any V <= d: M * d floats
        assert ws(d_model=d, image_vocab_size=d, num_factored_vocabs=1)[0] == narrow       # V = d
        assert ws(d_model=d, image_vocab_size=4 * d, num_factored_vocabs=1)[0] == narrow + M * 3 * d * 4   # V = 4d: M * V floats


# (genie_train_activation_bytes, genie_train_workspace_bytes) in exact, bf16, f16x3.  Read from the library of the commit before the
# training step's layer was stated once for the three precisions (one layout function for the saved activations): the buffers are
# opaque to the caller, their sizes are not.
TRAIN_BUFFER_BYTES = {
    "d64": [(966656, 18211328), (860160, 18604544), (1015808, 18997760)],                    # tests/test_hip_train_bf16.py
    "s144qk": [(15040512, 38822912), (13123584, 42361856), (15925248, 45900800)],             # tests/test_hip_train_geometry.py
    "t8s256": [(31457280, 49816576), (28311552, 62399488), (33554432, 74982400)],
    "c35/B1": [(2839543808, 161490944), (2371878912, 186656768), (2977955840, 211822592)],
    "c35/B8": [(22716350464, 808462336), (18975031296, 1009788928), (23823646720, 1211115520)],
    "c138/B1": [(5662310400, 390082560), (4726980608, 440414208), (5939134464, 490745856)],
    "c138/B8": [(45298483200, 1214263296), (37815844864, 1616916480), (47513075712, 2019569664)],
}


def test_training_buffer_sizes_are_unchanged():
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    C = pkg("config")

    def small(H, d, T, S, qk_norm, layers):
        return C.GenieConfig(num_layers=layers, num_heads=H, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                             num_prompt_frames=max(1, T // 2), use_mup=False)
    cases = {"d64": (small(2, 64, 4, 16, False, 2), 1), "s144qk": (small(2, 128, 4, 144, True, 2), 1),
             "t8s256": (small(2, 128, 8, 256, False, 1), 1), "c35/B1": (C.c35(), 1), "c35/B8": (C.c35(), 8),
             "c138/B1": (C.c138(), 1), "c138/B8": (C.c138(), 8)}
    assert sorted(cases) == sorted(TRAIN_BUFFER_BYTES)
    for name, (cfg, B) in cases.items():
        for prec, want in zip((lib_mod.PREC_EXACT, lib_mod.PREC_BF16, lib_mod.PREC_F16X3), TRAIN_BUFFER_BYTES[name]):
            c = lib_mod.make_cfg(cfg, prec)
            got = (L.genie_train_activation_bytes(c, B), L.genie_train_workspace_bytes(c, B))
            assert got == want, (name, prec, got, want)


def loop_workspace_sizes(L, c, T):
    """The size functions of the generate loops on the grid B x P (x guided) (x K), in one fixed order:
    [generate, generate_guided, rollout, fanout, fanout_branch]"""
    Bs, Ks, Ps = (1, 3, 16), (1, 3, 64), (1, T // 2, T - 1)
    return [[L.genie_generate_workspace_bytes(c, B, P) for B in Bs for P in Ps],
            [L.genie_generate_guided_workspace_bytes(c, B, P) for B in Bs for P in Ps],
            [L.genie_rollout_workspace_bytes(c, B, P, g) for g in (0, 1) for B in Bs for P in Ps],
            [L.genie_fanout_workspace_bytes(c, B, K, P, g) for g in (0, 1) for B in Bs for K in Ks for P in Ps],
            [L.genie_fanout_branch_bytes(c, B, K, P) for B in Bs for K in Ks for P in Ps]]


# loop_workspace_sizes of four configs, the same in exact, bf16 and f16x3.  Read from the library of the commit before the generate loops
# moved into a driver file of their own (one Decode, one PassCtx, one MaskGIT step, one commit rule): what a caller allocates stays.
LOOP_WORKSPACE_BYTES = {
    "d64": [
        [377600, 377600, 377600, 1131520, 1131520, 1131520, 6032640, 6032640, 6032640],
        [755712, 755712, 755712, 2265856, 2265856, 2265856, 12082688, 12082688, 12082688],
        [377600, 377600, 377600, 1131520, 1131520, 1131520, 6032640, 6032640, 6032640, 755712, 755712, 755712, 2265856, 2265856,
         2265856, 12082688, 12082688, 12082688],
        [377600, 377600, 377600, 766464, 766464, 766720, 16314880, 16314880, 16315136, 1131520, 1131520, 1131520, 2296320, 2296576,
         2297088, 48943872, 48944128, 48944640, 6032640, 6032640, 6032640, 12238336, 12240384, 12242432, 261032448, 261034496,
         261036544, 754432, 754432, 754432, 1530112, 1530368, 1530624, 32615936, 32616192, 32616448, 2262528, 2262528, 2262528,
         4588544, 4589312, 4590080, 97847296, 97848064, 97848832, 12065280, 12065280, 12065280, 24466688, 24470784, 24474880,
         521851904, 521856000, 521860096],
        [24576, 49152, 73728, 73728, 147456, 221184, 1572864, 3145728, 4718592, 73728, 147456, 221184, 221184, 442368, 663552,
         4718592, 9437184, 14155776, 393216, 786432, 1179648, 1179648, 2359296, 3538944, 25165824, 50331648, 75497472],
    ],
    "d256": [
        [46140672, 46140672, 46140672, 138422016, 138422016, 138422016, 738250752, 738250752, 738250752],
        [92347136, 92347136, 92347136, 277041408, 277041408, 277041408, 1477554176, 1477554176, 1477554176],
        [46140672, 46140672, 46140672, 138422016, 138422016, 138422016, 738250752, 738250752, 738250752, 92347136, 92347136,
         92347136, 277041408, 277041408, 277041408, 1477554176, 1477554176, 1477554176],
        [46140672, 46140672, 46140672, 46140672, 46140672, 46468864, 437168384, 437182720, 437197056, 138422016, 138422016,
         138422016, 138422016, 138422016, 139406080, 1311504896, 1311547904, 1311590912, 738250752, 738250752, 738250752,
         738250752, 738250752, 743497728, 6994692096, 6994921472, 6995150848, 92281344, 92281344, 92281344, 92281344, 92281344,
         92927232, 874123520, 874152192, 874180864, 276844032, 276844032, 276844032, 276844032, 276844032, 278781696, 2622370560,
         2622456576, 2622542592, 1476501504, 1476501504, 1476501504, 1476501504, 1476501504, 1486835712, 13985976320, 13986435072,
         13986893824],
        [1572864, 12582912, 23592960, 4718592, 37748736, 70778880, 100663296, 805306368, 1509949440, 4718592, 37748736, 70778880,
         14155776, 113246208, 212336640, 301989888, 2415919104, 4529848320, 25165824, 201326592, 377487360, 75497472, 603979776,
         1132462080, 1610612736, 12884901888, 24159191040],
    ],
    "d512": [
        [75500800, 75500800, 75500800, 226502400, 226502400, 226502400, 1208012800, 1208012800, 1208012800],
        [151067392, 151067392, 151067392, 453202176, 453202176, 453202176, 2417078272, 2417078272, 2417078272],
        [75500800, 75500800, 75500800, 226502400, 226502400, 226502400, 1208012800, 1208012800, 1208012800, 151067392, 151067392,
         151067392, 453202176, 453202176, 453202176, 2417078272, 2417078272, 2417078272],
        [75500800, 75500800, 75500800, 75500800, 75500800, 75500800, 672049408, 672063744, 672078080, 226502400, 226502400,
         226502400, 226502400, 226502400, 226502400, 2016147968, 2016190976, 2016233984, 1208012800, 1208012800, 1208012800,
         1208012800, 1208012800, 1208012800, 10752788480, 10753017856, 10753247232, 151001600, 151001600, 151001600, 151001600,
         151001600, 151001600, 1343885568, 1343914240, 1343942912, 453004800, 453004800, 453004800, 453004800, 453004800,
         453004800, 4031656704, 4031742720, 4031828736, 2416025600, 2416025600, 2416025600, 2416025600, 2416025600, 2416025600,
         21502169088, 21502627840, 21503086592],
        [3145728, 25165824, 47185920, 9437184, 75497472, 141557760, 201326592, 1610612736, 3019898880, 9437184, 75497472,
         141557760, 28311552, 226492416, 424673280, 603979776, 4831838208, 9059696640, 50331648, 402653184, 754974720, 150994944,
         1207959552, 2264924160, 3221225472, 25769803776, 48318382080],
    ],
    "v3x64": [
        [164608, 164608, 164608, 492544, 492544, 492544, 2624768, 2624768, 2624768],
        [329728, 329728, 329728, 987904, 987904, 987904, 5266944, 5266944, 5266944],
        [164608, 164608, 164608, 492544, 492544, 492544, 2624768, 2624768, 2624768, 329728, 329728, 329728, 987904, 987904, 987904,
         5266944, 5266944, 5266944],
        [164608, 164608, 164608, 287232, 287232, 287488, 6091264, 6091264, 6091520, 492544, 492544, 492544, 858624, 858880, 859392,
         18273024, 18273280, 18273792, 2624768, 2624768, 2624768, 4570624, 4572672, 4574720, 97454592, 97456640, 97458688, 328448,
         328448, 328448, 571648, 571904, 572160, 12168704, 12168960, 12169216, 984576, 984576, 984576, 1713152, 1713920, 1714688,
         36505600, 36506368, 36507136, 5249536, 5249536, 5249536, 9131264, 9135360, 9139456, 194696192, 194700288, 194704384],
        [24576, 49152, 73728, 73728, 147456, 221184, 1572864, 3145728, 4718592, 73728, 147456, 221184, 221184, 442368, 663552,
         4718592, 9437184, 14155776, 393216, 786432, 1179648, 1179648, 2359296, 3538944, 25165824, 50331648, 75497472],
    ],
}


def test_loop_workspace_sizes_are_unchanged():
    lib_mod = pkg("_lib")
    L = lib_mod.load()
    C = pkg("config")

    def model(H, d, T, S, **kw):
        return C.GenieConfig(num_layers=2, num_heads=H, d_model=d, T=T, S=S, qk_norm=False, use_mup=False, **kw)
    cases = {"d64": model(2, 64, 4, 16, num_factored_vocabs=2), "d256": model(8, 256, 16, 256, num_factored_vocabs=2),
             "d512": model(8, 512, 16, 256, num_factored_vocabs=2),
             "v3x64": model(2, 64, 4, 16, image_vocab_size=64 ** 3, num_factored_vocabs=3)}
    assert sorted(cases) == sorted(LOOP_WORKSPACE_BYTES)
    names = ["generate", "generate_guided", "rollout", "fanout", "fanout_branch"]
    for name, cfg in cases.items():
        T = cfg.T
        for prec in (lib_mod.PREC_EXACT, lib_mod.PREC_BF16, lib_mod.PREC_F16X3):
            c = lib_mod.make_cfg(cfg, prec)
            for fn, got, want in zip(names, loop_workspace_sizes(L, c, T), LOOP_WORKSPACE_BYTES[name]):
                assert got == want, (name, prec, fn, got, want)
            # scoring allocates what an unguided fan-out call does
            for B, K, P in [(1, 1, 1), (3, 3, T // 2), (16, 64, T - 1), (1, 64, T - 1)]:
                assert L.genie_score_workspace_bytes(c, B, K, P) == L.genie_fanout_workspace_bytes(c, B, K, P, 0) > 0
            # ... and every size function answers a bad argument with 0
            big = 0x40000000   # clips no guided pass (2 B) or fan-out pass (B * K) can count
            zero = [L.genie_generate_workspace_bytes(None, 1, 1), L.genie_generate_workspace_bytes(c, 0, 1),
                    L.genie_generate_workspace_bytes(c, 1, 0), L.genie_generate_workspace_bytes(c, 1, T + 1),
                    L.genie_generate_guided_workspace_bytes(None, 1, 1), L.genie_generate_guided_workspace_bytes(c, 0, 1),
                    L.genie_generate_guided_workspace_bytes(c, big, 1), L.genie_generate_guided_workspace_bytes(c, 1, 0),
                    L.genie_generate_guided_workspace_bytes(c, 1, T + 1),
                    L.genie_rollout_workspace_bytes(None, 1, 1, 0), L.genie_rollout_workspace_bytes(c, 0, 1, 0),
                    L.genie_rollout_workspace_bytes(c, big, 1, 1), L.genie_rollout_workspace_bytes(c, 1, 0, 0),
                    L.genie_rollout_workspace_bytes(c, 1, T, 1),
                    L.genie_fanout_workspace_bytes(None, 1, 1, 1, 0), L.genie_fanout_workspace_bytes(c, 0, 1, 1, 0),
                    L.genie_fanout_workspace_bytes(c, 1, 0, 1, 0), L.genie_fanout_workspace_bytes(c, big // 2, 2, 1, 0),
                    L.genie_fanout_workspace_bytes(c, big // 4, 2, 1, 1), L.genie_fanout_workspace_bytes(c, 1, 1, 0, 0),
                    L.genie_fanout_workspace_bytes(c, 1, 1, T, 1),
                    L.genie_score_workspace_bytes(None, 1, 1, 1), L.genie_score_workspace_bytes(c, 0, 1, 1),
                    L.genie_score_workspace_bytes(c, 1, 0, 1), L.genie_score_workspace_bytes(c, big // 2, 2, 1),
                    L.genie_score_workspace_bytes(c, 1, 1, 0), L.genie_score_workspace_bytes(c, 1, 1, T),
                    L.genie_fanout_branch_bytes(None, 1, 1, 1), L.genie_fanout_branch_bytes(c, 0, 1, 1),
                    L.genie_fanout_branch_bytes(c, 1, 0, 1), L.genie_fanout_branch_bytes(c, big // 2, 2, 1),
                    L.genie_fanout_branch_bytes(c, 1, 1, 0), L.genie_fanout_branch_bytes(c, 1, 1, T)]
            assert zero == [0] * len(zero), (name, prec, zero)


def test_config_roundtrip_and_derived(tmp_path):
    C = pkg("config")
    c = C.c35()
    assert c.factored_vocab_size == 512 and c.mask_token_id == 262144 and c.head_dim == 32
    assert abs(c.attn_scale - 32 ** -0.5) < 1e-12 and c.readout_mult == 1.0
    m = C.GenieConfig(num_layers=2, num_heads=8, d_model=512, use_mup=True, num_factored_vocabs=2)
    assert m.attn_scale == 8 / 64 and m.readout_mult == 0.5
    p = tmp_path / "config.json"
    c.save_pretrained(p)
    assert C.GenieConfig.from_pretrained(p) == c
    # the reference's shipped JSON loads unchanged (same field names)
    import json
    shipped = {"num_layers": 32, "num_heads": 8, "d_model": 256, "T": 16, "S": 256, "image_vocab_size": 262144,
               "use_mup": False, "num_factored_vocabs": 2, "qkv_bias": False, "proj_bias": True, "attn_drop": 0.0,
               "qk_norm": False, "mlp_ratio": 4.0, "mlp_drop": 0.0, "mlp_bias": True}
    p.write_text(json.dumps(shipped))
    assert C.GenieConfig.from_pretrained(p) == c


def test_synthetic_is_deterministic_and_complete():
    C, S = pkg("config"), pkg("synthetic")
    cfg = C.GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    a, b = S.make_state_dict(cfg, seed=5), S.make_state_dict(cfg, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["out_x_proj.weight"], S.make_state_dict(cfg, seed=6)["out_x_proj.weight"])
    n_params = sum(v.size for v in S.make_state_dict(C.c35(), seed=0, law="init").values())
    assert n_params == 35_218_688  # the shipped config is GENIE_35M
    assert sum(int(np.prod(s)) for _, s, _, _ in S.state_dict_spec(C.c138())) == 137_545_216
    # the module's state dict has exactly these keys
    import torch  # noqa: F401
    m = pkg("st_mask_git").STMaskGIT(cfg)
    assert sorted(m.state_dict()) == sorted(a)
    q = C.GenieConfig(num_layers=1, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=True)
    assert sorted(pkg("st_mask_git").STMaskGIT(q).state_dict()) == sorted(S.make_state_dict(q))


def test_checkpoint_roundtrip(tmp_path):
    import torch
    C, S = pkg("config"), pkg("synthetic")
    cfg = C.GenieConfig(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    M = pkg("st_mask_git").STMaskGIT
    m = M(cfg).load_numpy_state_dict(S.make_state_dict(cfg, seed=1))
    m.save_pretrained(tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["config.json", "model.safetensors"]
    m2 = M.from_pretrained(tmp_path)
    assert m2.config == cfg
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())


def test_no_cpu_fallback():
    import torch
    C = pkg("config")
    cfg = C.GenieConfig(num_layers=1, num_heads=2, d_model=32, T=4, S=16, num_factored_vocabs=2, qk_norm=False)
    m = pkg("st_mask_git").STMaskGIT(cfg)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.compute_logits(torch.zeros(1, 4, 4, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU only"):
        pkg("attention").SelfAttention(2, 32, qk_norm=False)(torch.zeros(1, 4, 32))


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(REPO, "1xgpt_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "genie_oracle" not in src, f


def test_shard_range_and_means():
    D = pkg("distributed")
    for n, w in [(512, 8), (10, 3), (3, 8), (64, 1)]:
        parts = [D.shard_range(n, r, w) for r in range(w)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(parts[i][1] == parts[i + 1][0] for i in range(w - 1))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1
    m = D.means_from_sums([20.0, 2.0, 3.0, 12.0, 30.0, 2.0])
    assert m == dict(loss=10.0, acc=0.25, frames=30, clips=2)


def test_header_is_plain_c_and_the_library_links_from_c(tmp_path):
    """The drop-in boundary is a C ABI: include/genie_hip.h must compile as plain C99 (no C++-isms, no torch / HIP types in the
    signatures) and a C program must link against libgenie_hip.so and call it -- what a cgo / JNI / FFI binding of the reference's
    maintainer would do.  No GPU: genie_version / genie_workspace_bytes / genie_check_config are host-only."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lib = pkg("_lib").LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("library not built")
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "genie_hip.h"\n'
                   "int main(void) {\n"
                   "    genie_cfg c; memset(&c, 0, sizeof c);\n"
                   "    c.num_layers = 2; c.num_heads = 8; c.head_dim = 64; c.d_model = 512; c.T = 16; c.S = 256; c.hidden = 2048;\n"
                   "    c.factored_vocab = 512; c.num_factored = 2; c.image_vocab_size = 262144; c.attn_scale = 0.125f; c.readout_mult = 1.0f;\n"
                   "    c.precision = GENIE_PREC_F16X3;\n"
                   "    if (genie_version() != GENIE_ABI_VERSION) return 1;\n"
                   "    if (genie_check_config(&c) != GENIE_OK) { puts(genie_last_error()); return 2; }\n"
                   "    if (genie_workspace_bytes(&c, 4) == 0 || genie_generate_workspace_bytes(&c, 4, 8) < genie_workspace_bytes(&c, 4)) return 3;\n"
                   "    c.head_dim = 48;\n"
                   "    if (genie_check_config(&c) == GENIE_OK || strlen(genie_last_error()) == 0) return 4;   /* errors are codes + text, never aborts */\n"
                   '    printf("%zu\\n", genie_prefix_cache_bytes(&c, 1));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "abi"
    inc = os.path.join(REPO, "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-c", str(src), "-o", str(tmp_path / "abi.o")], check=True)
    subprocess.run([gcc, str(tmp_path / "abi.o"), lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
