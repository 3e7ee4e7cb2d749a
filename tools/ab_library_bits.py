#!/usr/bin/env python3
"""Do two builds of libgenie_hip.so compute the same bits with the same launches?  (The check of a host-code-only change.)

    python 1xgpt_amd/build.py --variant parent          # at the commit to compare against
    python tools/ab_library_bits.py 1xgpt_amd/lib_ab_parent.so 1xgpt_amd/libgenie_hip.so

One battery runs in two fresh child processes, one per library (GENIE_HIP_LIBRARY), each under its own time limit; the second is not
started when the first fails.  Per case a child records the return code, the SHA-256 of every output tensor's bytes (equal digests =
zero differing bits) and, per kernel class, the name / launch-count table of genie_profile_kernels.  The parent process compares the two
records and exits non-zero on any difference.

The battery: every pass kind (full forward, clean pass + masked-frames pass at frame0 0 and 1, a half-length clean pass into a full-length
cache at 1 and 2 clips, one- and two-frame decode passes, the cached generate loop with 2 MaskGIT steps and the merged commit, one
STBlock) in all three precisions, for a LayerNorm and a qk-norm model, at four geometries; then BRANCH_CASES, one model each for the
branches of the 16-bit layer driver (csrc/st_block.hip) that those models do not reach.  A case the library refuses (e.g. two frames
per pass outside f16x3) counts through its return code.  WATCHED names the kernels whose dispatch depends on the pass kind: the battery
as a whole must reach each of them in the first library, else the battery itself has failed.  Two kernels of that kind carry no name a
table could show: the launches of attn_spatial_dma are profiled unnamed (they are counted, and compared, as "(unnamed)" of the spatial
attention class behind the 16-bit gemm16_pp qkv GEMMs), and splitk2_residual_kernel is launched outside any profiler scope (the d 512
bf16 decode passes at 8 clips are inside the shape window of fc2_splitk2; its two-slab GEMM in front is counted).  For both a proxy
is printed with the watched lines, and the first one is required.

The training battery (--battery train; the default runs both, each in its own pair of child processes): per case a GenieTrainer, one
forward_backward, a second one with accumulate=True, one optimizer_step.  Recorded: the loss sums and every gradient tensor after each
call, the flat parameters after the step, genie_train_activation_bytes / genie_train_workspace_bytes, and the kernel tables around the
whole case (the trainer's weight packing included).  TRAIN_CASES are geometries tests/test_hip_train*.py pin, in all three precisions;
s144 (T*S = 288) is refused by the 16-bit step and counts through its return code."""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, d_model, heads, T, S, clips of the main cases)
GEOMETRIES = [("d64", 64, 2, 4, 16, 3),        # generic attention kernels, ragged GEMM tiles
              ("d256", 256, 8, 16, 256, 8),    # the shipped geometry: 8 clips = every fused bf16 kernel, chip-filling GEMMs
              ("d512", 512, 8, 16, 256, 8),    # heads of 64
              ("d64h16", 64, 4, 4, 16, 3)]     # heads of 16: the bf16 temporal qkv and KV cache stay f32 (temporal_qkv16 false)
# Branches of the 16-bit layer driver that no model above reaches: (tag, precision, clips, the cases to run, (d, heads, T, S, qk_norm,
# qkv_bias), edit of the weights / of how they are packed)
BRANCH_CASES = [
    # |w| >= 32 in a row of every Linear: each leaves gemm16_pp for a two-accumulator kernel (8 clips: gemm16_pp would take them all) and
    # the spatial sub-block its fused qkv + DMA attention for the f32 qkv
    ("d256wide/ln/f16x3", "f16x3", 8, ("compute_logits", "clean_pass", "masked_frames_logits"), (256, 8, 16, 256, False, True), "wide"),
    # ... at d 512, where no fused kernel takes the temporal qkv Linear
    ("d512wide/ln/f16x3", "f16x3", 8, ("compute_logits",), (512, 8, 16, 256, False, True), "wide"),
    # no qkv bias: the fused MLP kernel of block 0 also writes block 1's spatial operand planes (BlockCarry::qkv_planes_done); block 1 reads
    # them with the fused attention + out-projection kernel at 128 sequences (8 clips), with the stand-alone attention kernel at 32 (2 clips)
    ("d256nobias/ln/bf16", "bf16", 8, ("compute_logits",), (256, 8, 16, 256, False, False), None),
    ("d256nobias2/ln/bf16", "bf16", 2, ("compute_logits",), (256, 8, 16, 256, False, False), None),
    # fc2_splitk2 on split planes: a one-frame pass of 2,048 rows at hidden 2,048 that the fragment-order frame kernels do not take
    ("d512noframe/ln/f16x3", "f16x3", 8, ("clean_pass_into_full_cache", "frame_pass"), (512, 8, 16, 256, False, True), "no_frame_streams")]
WIDE_TENSORS = [f"decoder.layers.0.{t}.weight" for t in ("spatial_attn.qkv", "spatial_attn.proj", "temporal_attn.qkv", "temporal_attn.proj",
                                                         "mlp.fc1", "mlp.fc2")] + ["out_x_proj.weight"]
PRECISIONS = ["exact", "bf16", "f16x3"]
WATCHED = ["spatial_attn_proj_bf16_kernel", "temporal_fused_bf16_kernel", "mlp_fused_bf16_kernel", "temporal_prefix_fused_bf16_kernel",
           "temporal_qkv_attn_f16x3_kernel", "gemm16_pp_kernel", "gemm16_sm_ln_kernel"]
N_CLASSES = 6   # GENIE_KC_COUNT
# training battery: (name, heads, d_model, T, S, clips, qk_norm, layers, action_vocab_size)
TRAIN_CASES = [("d64", 2, 64, 4, 16, 1, False, 2, 0),         # transposed-copy wgrad with ns = 1; materialised spatial backward
               ("t8s64qk", 2, 64, 8, 64, 1, True, 2, 0),      # qk-norm epilogue hand-offs; short-window temporal forward; generic temporal backward
               ("d128", 2, 128, 4, 256, 2, False, 2, 0),      # fused spatial backward (exact / f16x3); attn_bwd16 + TN wgrad with slabs (bf16)
               ("d256qk", 8, 256, 4, 256, 2, True, 2, 0),     # every weight on TN (bf16); wgrad16 ns > 1 (f16x3)
               ("d384t16", 6, 384, 16, 64, 1, False, 1, 0),   # T = 16 MFMA temporal backward; TN and transposed-copy mixed in one layer
               ("s144", 1, 64, 2, 144, 1, False, 2, 0),       # exact only: the 16-bit step refuses T*S = 288
               ("d64act", 2, 64, 4, 16, 1, False, 2, 5)]      # the _cond forward and the embed backward with a table gradient
TRAIN_WATCHED = ["gemm_f32_gen_kernel", "attn_spatial_bwd_fused_kernel", "wgrad16_tn_kernel", "attn_bwd16_"]


def child(out_path, battery):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    _lib = importlib.import_module("1xgpt_amd._lib")
    G = importlib.import_module("1xgpt_amd.generate")
    synth = importlib.import_module("1xgpt_amd.synthetic")
    GenieConfig = importlib.import_module("1xgpt_amd.config").GenieConfig
    STMaskGIT = importlib.import_module("1xgpt_amd.st_mask_git").STMaskGIT
    lib = _lib.load()
    record = {}

    def nonzero_biases(sd, seed):   # the synthetic law leaves biases at zero: make every bias the kernels add count
        g = np.random.default_rng(seed)
        for k in sd:
            if k.endswith(".bias") and "norm" not in k:
                sd[k] = (0.05 * g.standard_normal(sd[k].shape)).astype(np.float32)

    def digest(t):
        a = t.detach().contiguous().cpu().numpy()
        return [str(a.dtype), list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]

    def record_case(name, fn):
        """fn() -> (rc, {tensor name: tensor}); the launches of all classes between reset and read are the case's table"""
        _lib.check(lib.genie_profile_enable((1 << N_CLASSES) - 1), "profile_enable")
        lib.genie_profile_reset()
        try:
            rc, outs = fn()
        except _lib.GenieHipError as e:
            rc, outs = e.code, {}
        torch.cuda.synchronize()
        table = {}
        buf = ctypes.create_string_buffer(1 << 16)
        for kc in range(N_CLASSES):
            _lib.check(lib.genie_profile_kernels(kc, buf, len(buf)), "profile_kernels")
            for ln in buf.value.decode().splitlines():
                table[f"{kc}:{ln.split(chr(9))[0]}"] = int(float(ln.split("\t")[1]))
        lib.genie_profile_enable(0)
        record[name] = {"rc": rc, "outs": {k: digest(v) for k, v in outs.items()} if rc == 0 else {}, "kernels": table}
        print(name, "rc", rc, "launches", sum(table.values()), flush=True)

    if battery == "train":
        TO = importlib.import_module("oracle.genie_train_oracle")   # its collator draws from NumPy: the same batch in both children
        GenieTrainer = importlib.import_module("1xgpt_amd.train").GenieTrainer
        for name, heads, d, T, S, B, qk_norm, layers, n_act in TRAIN_CASES:
            cfg = GenieConfig(num_layers=layers, num_heads=heads, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm,
                              use_mup=False, qkv_bias=True, num_prompt_frames=max(1, T // 2), action_vocab_size=n_act)
            sd = synth.make_state_dict(cfg, seed=5, law="conditioned")
            nonzero_biases(sd, 6)
            batches = [TO.maskgit_collate(synth.make_clips(B, cfg, seed=7 + i), cfg, TO.NumpyDraws(9 + i)) for i in range(2)]
            kw = [{"action_ids": torch.from_numpy(np.random.default_rng(11 + i).integers(0, n_act, (B, T))).cuda()} if n_act else {}
                  for i in range(2)]
            for prec in PRECISIONS:
                sizes = []

                def step():
                    tr = GenieTrainer(STMaskGIT(cfg, precision=prec).load_numpy_state_dict(sd).to("cuda"), lr=1e-3)
                    sizes[:] = [lib.genie_train_activation_bytes(tr.cfg, B), lib.genie_train_workspace_bytes(tr.cfg, B)]
                    outs = {}
                    for i, b in enumerate(batches):
                        tr.forward_backward(torch.from_numpy(b["input_ids"]).cuda(), torch.from_numpy(b["labels"]).cuda(),
                                            accumulate=i == 1, **kw[i])
                        outs[f"call{i}/sums"] = tr.sums.clone()
                        outs.update({f"call{i}/grad/{k}": g.clone() for k, g in tr.gradients().items()})
                    tr.optimizer_step()
                    outs["params"] = tr.params
                    return 0, outs
                record_case(f"{name}/{prec}", step)
                record[f"{name}/{prec}"]["sizes"] = list(sizes)
                print(f"{name}/{prec} activation / workspace bytes {sizes}", flush=True)
                torch.cuda.empty_cache()
        with open(out_path, "w") as f:
            json.dump(record, f)
        return

    def model_cases(tag, cfg, sd, prec, B, only=None):
        """Every pass kind on one model (`only`: the case names to run, None = all of them)"""
        d, T, S = cfg.d_model, cfg.T, cfg.S
        hw = int(round(S ** 0.5))
        V = cfg.factored_vocab_size * cfg.num_factored_vocabs

        def case(name, fn):
            if only is None or name[len(tag) + 1:].split("/")[0] in only:
                record_case(name, fn)
        m = STMaskGIT(cfg, precision=prec).load_numpy_state_dict(sd).to("cuda")
        c, w, layers = m._weights()[:3]
        st = torch.cuda.current_stream().cuda_stream
        ids = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, T, S)
        masked = ids.clone()
        masked[:, T // 2:, ::3] = cfg.image_vocab_size
        ws = m._workspace(B, generate_prompt_frames=T // 2)
        nbytes = lib.genie_prefix_cache_bytes(c, B)

        def full():
            logits = m.compute_logits_frames(masked.view(B, T, hw, hw), T - 2, T, "token")
            bcthw = m.compute_logits_frames(masked.view(B, T, hw, hw), T - 1, T, "bcthw")   # the readout's other layout
            hidden = m.hidden_states(masked.view(B, T, hw, hw)).clone()
            assert bool(torch.isfinite(logits).all()), tag   # (equal digests of NaNs would compare nothing)
            return 0, {"logits": logits, "logits_bcthw": bcthw, "hidden": hidden}
        case(tag + "/compute_logits", full)

        n = T - 1
        cache = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

        def clean():
            rc = lib.genie_clean_pass(c, w, ids[:, :n].contiguous().data_ptr(), B, n, n, cache.data_ptr(), nbytes, ws.data_ptr(),
                                      ws.numel(), st)
            return rc, {"cache": cache}
        case(tag + "/clean_pass", clean)
        for frame0 in (0, 1):
            def masked_pass():
                lg = torch.zeros(B, n, S, V, dtype=torch.float32, device="cuda")
                rc = lib.genie_masked_frames_logits(c, w, masked[:, frame0:frame0 + n].contiguous().data_ptr(), B, frame0, n,
                                                    cache.data_ptr(), nbytes, lg.data_ptr(), ws.data_ptr(), ws.numel(), st)
                return rc, {"logits": lg}
            case(f"{tag}/masked_frames_logits/frame0={frame0}", masked_pass)

        P = T // 2
        for Bx in (1, 2, B):   # a half-length clean pass into the full-length cache, then decode passes against it
            nb = lib.genie_prefix_cache_bytes(c, Bx)
            kv = torch.zeros(nb, dtype=torch.uint8, device="cuda")

            def strided():
                rc = lib.genie_clean_pass(c, w, ids[:Bx, :P].contiguous().data_ptr(), Bx, P, T, kv.data_ptr(), nb, ws.data_ptr(),
                                          ws.numel(), st)
                return rc, {"cache": kv}
            case(f"{tag}/clean_pass_into_full_cache/B={Bx}", strided)

            def frame():
                lg = torch.zeros(Bx, S, V, dtype=torch.float32, device="cuda")
                rc = lib.genie_frame_pass(c, w, masked[:Bx, P].contiguous().data_ptr(), Bx, P, kv.data_ptr(), nb, lg.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st)
                return rc, {"logits": lg, "cache": kv}
            case(f"{tag}/frame_pass/B={Bx}", frame)

            def frames():
                lg = torch.zeros(Bx, S, V, dtype=torch.float32, device="cuda")
                rc = lib.genie_frames_pass(c, w, masked[:Bx, P:P + 2].contiguous().data_ptr(), Bx, P, 2, kv.data_ptr(), nb,
                                           lg.data_ptr(), ws.data_ptr(), ws.numel(), st)
                return rc, {"logits": lg, "cache": kv}
            case(f"{tag}/frames_pass_nf2/B={Bx}", frames)

        noise = torch.rand(T - P, 1, B, S, generator=torch.Generator().manual_seed(3)).cuda()

        def generate():
            out = G.generate_frames_cached(m, ids.view(B, T, hw, hw), P, 2, 0.0, False, noise=noise, merge_commit=True)
            return 0, {"tokens": out}
        case(tag + "/generate_cached", generate)

        def block():
            x = (0.5 * torch.randn(B, T, S, d, generator=torch.Generator().manual_seed(4))).cuda()
            rc = lib.genie_st_block_forward(c, layers[0], x.data_ptr(), B, ws.data_ptr(), ws.numel(), st)
            return rc, {"x": x}
        case(tag + "/st_block_forward", block)
        del m, ws, cache
        torch.cuda.empty_cache()

    def make_cfg(d, heads, T, S, qk_norm, qkv_bias=True):
        return GenieConfig(num_layers=2, num_heads=heads, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm, use_mup=False,
                           qkv_bias=qkv_bias)

    for gname, d, heads, T, S, B in GEOMETRIES:
        for qk_norm in (False, True):
            cfg = make_cfg(d, heads, T, S, qk_norm)
            sd = synth.make_state_dict(cfg, seed=5, law="conditioned")
            nonzero_biases(sd, 6)
            for prec in PRECISIONS:
                model_cases(f"{gname}/{'qknorm' if qk_norm else 'ln'}/{prec}", cfg, sd, prec, B)
    for tag, prec, B, only, geometry, edit in BRANCH_CASES:
        cfg = make_cfg(*geometry)
        sd = synth.make_state_dict(cfg, seed=5, law="conditioned")
        nonzero_biases(sd, 6)
        env = {}
        if edit == "wide":   # one row of every Linear of the block and of the readout reaches |w| >= 32 (tests/test_hip_configs.py)
            for k in WIDE_TENSORS:
                sd[k][5] *= 40.0 / np.abs(sd[k][5]).max()
        elif edit == "no_frame_streams":
            env = {"GENIE_NO_FRAME_KERNELS": "1"}   # (read by the weight packer: no fragment-order streams -> the layer loop runs the pass)
        os.environ.update(env)
        try:
            model_cases(tag, cfg, sd, prec, B, only)
        finally:
            for k in env:
                del os.environ[k]
    with open(out_path, "w") as f:
        json.dump(record, f)


def run_battery(a, battery):
    """Both children of one battery and the comparison of their records -> 0, or the exit status of the failure"""
    watched = TRAIN_WATCHED if battery == "train" else WATCHED
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, path in enumerate((a.library_a, a.library_b)):
            out = os.path.join(tmp, f"record_{i}.json")
            env = dict(os.environ, GENIE_HIP_LIBRARY=os.path.abspath(path))
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, "--battery", battery], env=env,
                                    timeout=a.timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"FAIL: the {battery} battery on {path} ended with status {rc}; nothing more was started")
                return 2
            records.append(json.load(open(out)))
    ra, rb = records
    bad = 0
    if sorted(ra) != sorted(rb):
        print("FAIL: the two runs did not record the same cases")
        return 2
    n_tensors = 0
    for name in ra:
        ca, cb = ra[name], rb[name]
        if ca["rc"] != cb["rc"]:
            bad += 1
            print(f"DIFF {name}: return code {ca['rc']} != {cb['rc']}")
        if ca.get("sizes") != cb.get("sizes"):
            bad += 1
            print(f"DIFF {name}: activation / workspace bytes {ca.get('sizes')} != {cb.get('sizes')}")
        for k in sorted(set(ca["outs"]) | set(cb["outs"])):
            n_tensors += 1
            if ca["outs"].get(k) != cb["outs"].get(k):
                bad += 1
                print(f"DIFF {name}: tensor {k}: {ca['outs'].get(k)} != {cb['outs'].get(k)}")
        if ca["kernels"] != cb["kernels"]:
            bad += 1
            for k in sorted(set(ca["kernels"]) | set(cb["kernels"])):
                if ca["kernels"].get(k) != cb["kernels"].get(k):
                    print(f"DIFF {name}: launches of {k}: {ca['kernels'].get(k)} != {cb['kernels'].get(k)}")
    seen = {}
    for name, cs in ra.items():
        for k, v in cs["kernels"].items():
            for wk in watched:
                if wk in k:
                    seen.setdefault(wk, {}).setdefault(name.split("/")[0], 0)
                    seen[wk][name.split("/")[0]] += v
    for wk in watched:
        print(f"watched {wk}: launches per geometry {seen.get(wk, {})}")
    missing = [wk for wk in watched if wk not in seen]
    if battery == "inference":
        missing += inference_proxies(ra)
    refused = sorted(n for n in ra if ra[n]["rc"] != 0)
    print(f"{battery} battery: {len(ra)} cases ({len(refused)} refused by both libraries alike), {n_tensors} output tensors, "
          f"{sum(sum(c['kernels'].values()) for c in ra.values())} profiled launches in the first library")
    if missing:
        print(f"FAIL (of the {battery} battery): never reached {missing}")
        return 3
    if bad:
        print(f"FAIL: {bad} differences in the {battery} battery")
        return 1
    return 0


def inference_proxies(ra):
    """Proxies for the two kernels no table names -> what is missing.  attn_spatial_dma: the unnamed launches of the spatial attention
    class in the 16-bit cases of the S = 256 geometries (every launcher of that class the 16-bit drivers reach is profiled unnamed; the
    DMA kernel is the one behind a gemm16_pp qkv GEMM) -- each geometry must show some.  splitk2_residual: the GEMM table of the one
    case inside the shape window of fc2_splitk2 (its two-slab GEMM is one launch of the kernel the unsplit fc2 would run on, so this is
    printed, not required)."""
    missing = []
    for gname in ("d256", "d512"):
        per = {prec: sum(cs["kernels"].get("1:(unnamed)", 0) for n, cs in ra.items() if n.startswith(gname + "/") and f"/{prec}/" in n)
               for prec in ("bf16", "f16x3")}
        print(f"proxy attn_spatial_dma: unnamed spatial-attention launches at {gname}: {per}")
        if not sum(per.values()):
            missing.append(f"attn_spatial_dma (no unnamed spatial-attention launch in the 16-bit cases at {gname})")
    sk = ra.get("d512/ln/bf16/frame_pass/B=8", {"kernels": {}})["kernels"]
    print("proxy splitk2_residual: GEMM launches of d512/ln/bf16/frame_pass/B=8 (2,048 rows, hidden 2,048: inside the fc2_splitk2 window):",
          {k: v for k, v in sk.items() if k.startswith("0:")})
    for name in ("d512/ln/f16x3/frame_pass/B=8", "d512noframe/ln/f16x3/frame_pass/B=8"):   # the same pass on the frame kernels / in the layer loop
        print(f"proxy splitk2_residual on split planes: GEMM launches of {name}:",
              {k: v for k, v in ra.get(name, {"kernels": {}})["kernels"].items() if k.startswith("0:")})
    for name in ("d256nobias/ln/bf16/compute_logits", "d256nobias2/ln/bf16/compute_logits"):
        # qkv_planes_done: three forwards of two blocks run 6 spatial sub-blocks on 3 qkv GEMMs; below 128 sequences block 1 shows an unnamed
        # spatial attention launch in place of spatial_attn_proj
        print(f"proxy qkv_planes_done: launches of {name}:", ra.get(name, {"kernels": {}})["kernels"])
    return missing


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("library_a", nargs="?", help="the library to compare against (its tables decide whether the battery reached WATCHED)")
    ap.add_argument("library_b", nargs="?")
    ap.add_argument("--timeout", type=int, default=420, help="time limit of each child process, seconds")
    ap.add_argument("--battery", default="all", choices=["all", "inference", "train"],
                    help="each battery runs in its own pair of child processes; a failing one ends the run")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.battery)
    if not (a.library_a and a.library_b):
        ap.error("two libraries")
    for battery in (["inference", "train"] if a.battery == "all" else [a.battery]):
        status = run_battery(a, battery)
        if status:
            return status
    print("PASS: zero differing bits, identical return codes, identical kernel tables")
    return 0


if __name__ == "__main__":
    sys.exit(main())
