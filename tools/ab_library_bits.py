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
STBlock) in all three precisions, for a LayerNorm and a qk-norm model, at five geometries; then BRANCH_CASES, one model each for the
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
s144 (T*S = 288) is refused by the 16-bit step and counts through its return code.  Then TEMPORAL_BWD_CASES: genie_temporal_attention_backward
alone on seeded inputs, into a sentinel-filled output.  Then the loss and scoring launches of csrc/kernels_loss.hip alone (loss_cases):
genie_ce_objective without and with a struct (eps 0.1, zeta 1e-4, frame weights 1, 0, 2) and genie_ce_distill at tau 1 and 2 on T = 3,
S = 5 and 1 and 3 clips; genie_factored_ce in both layouts, with and without weight_ids, and genie_score_logits with hits and token_nll
at the smallest geometry -- each at vocabularies 2 x 512, 3 x 80 and 1 x 576.  Their f64 sums that workgroups fill with atomics depend
on arrival order and are compared within (workgroups) * 2^-52 relative; counts and every other slot exactly.

The loops battery (--battery loops): the generate loops of csrc/generate_api.hip, called through ctypes on LOOP_MODELS.  Per model and
clip count: genie_maskgit_generate_ex / _guided (3 steps; random, greedy and confidence unmasking at temperature 0 and under a
(0.7, 50, 0.9) law; the step-0 logits in both layouts; guidance of scale 3 and of scale 1), genie_generate_cached_ex / _guided (merged and
unmerged commits, teacher forcing in time, step-0 logits, a law, actions), genie_rollout_cached over three windows (in one call, and split
in mid-window with resume = 1; plain, with actions, guided), genie_generate_fanout (K = 1 and 3; P = 1, T / 2 and T - 1; per-branch
actions; guided) and genie_score_fanout (K = 1 and 3; merged and unmerged; with and without hits / token_nll / actions); then the calls
each entry point refuses (NULL pointer, frames past T, a workspace or cache one byte short, temperature > 0 without uniforms, guidance
without actions, ...).  Every output tensor starts sentinel-filled and every cache zeroed, and all are digested whether the call was
refused or not: a refused call must leave them as they were.  Before a record is kept, float outputs are checked finite and generated
tokens checked not to be one id."""
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
              ("d64h16", 64, 4, 4, 16, 3),     # heads of 16: the bf16 temporal qkv and KV cache stay f32 (temporal_qkv16 false)
              # T > 16: the generic prefix attention kernel, causal attn_generic, and the decode attention kernel's t >= 16 path (the
              # frame passes start at slot T / 2 = 16)
              ("d64t32", 64, 2, 32, 16, 2)]
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
               ("d64act", 2, 64, 4, 16, 1, False, 2, 5),      # the _cond forward and the embed backward with a table gradient
               # the tiled MFMA temporal backward at its other instantiations (d384t16 is T = 16, head_dim 64): one layer, one clip, S = 16
               ("t16h32qk", 2, 64, 16, 16, 1, True, 1, 0),
               ("t32h32", 2, 64, 32, 16, 1, False, 1, 0),
               ("t32h64", 1, 64, 32, 16, 1, False, 1, 0),
               ("t64h32", 2, 64, 64, 16, 1, False, 1, 0),
               ("t64h64", 1, 64, 64, 16, 1, False, 1, 0)]
# ... and genie_temporal_attention_backward alone: (T, head_dim, clips, S, heads, qk_ld / d_model).  B S H = 12 fills its workgroups of 4 waves,
# 3 and 5 leave idle waves in the last one; qk_ld = 3 d: qk is qkv itself, 2 d: a buffer of its own.  T = 8 and head_dim 128 are the
# scalar kernel's; the last two are refused (E_SHAPE, E_UNSUPPORTED) and must leave the output as it was.
TEMPORAL_BWD_CASES = ([(T, Dh, *g) for T in (16, 32, 64) for Dh in (32, 64) for g in ((2, 3, 2, 3), (1, 3, 1, 2), (1, 5, 1, 3))]
                      + [(8, 32, 2, 3, 2, 3), (8, 64, 1, 5, 1, 2), (16, 128, 1, 3, 1, 3), (16, 128, 1, 5, 1, 2), (4, 32, 2, 3, 2, 2),
                         (32, 128, 1, 3, 1, 3), (8, 16, 1, 3, 1, 3)])
TRAIN_WATCHED = ["gemm_f32_gen_kernel", "attn_spatial_bwd_fused_kernel", "wgrad16_tn_kernel", "attn_bwd16_", "count_frames_kernel",
                 "ce_objective_kernel", "ce_distill_kernel"]
# loops battery: (name, d_model, heads, T, S, precisions, clip counts), a LayerNorm and a qk-norm model each.  d64: the generic kernels --
# every merged commit is refused and the loops fall back, the context runs frame by frame; d256 / d512 in f16x3: the fragment-order
# passes with merged commits and the multi-frame context pass; 9 clips of 8 context frames are past its 16,384-row cut (the clean pass runs)
LOOP_MODELS = [("d64", 64, 2, 4, 16, PRECISIONS, (3,)),
               ("d256", 256, 8, 16, 256, ["f16x3"], (1, 2)),
               ("d512", 512, 8, 16, 256, ["f16x3"], (1, 2, 9))]
LOOPS_WATCHED = ["gemm16_fr(m)_kernel (readout)"]   # the fragment-order passes: without them no merged commit and no multi-frame context


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

    def record_case(name, fn, keep_refused=False):
        """fn() -> (rc, {tensor name: tensor}); the launches of all classes between reset and read are the case's table.  keep_refused:
        the outputs of a refused call are digested too (sentinel-filled by the case: a refused call must not have touched them)"""
        _lib.check(lib.genie_profile_enable((1 << N_CLASSES) - 1), "profile_enable")
        lib.genie_profile_reset()
        sums = {}
        try:
            rc, outs, *more = fn()   # (a loss case adds its f64 sums: see loss_cases)
            sums = more[0] if more else {}
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
        record[name] = {"rc": rc, "outs": {k: digest(v) for k, v in outs.items()} if rc == 0 or keep_refused else {}, "kernels": table}
        if sums:
            record[name]["sums"] = {k: {"values": [float(x).hex() for x in t.cpu().tolist()], "atomic": list(atomic), "workgroups": wg}
                                    for k, (t, atomic, wg) in sums.items()}
        print(name, "rc", rc, "launches", sum(table.values()), flush=True)

    def loss_cases():
        """The loss and scoring launches alone (csrc/kernels_loss.hip), on seeded logits into sentinel-filled outputs.  Digested: the
        gradient rows that replace the logits, nll, hits, token_nll.  The f64 sums come back apart, as (tensor, the slots that workgroups
        add to with atomics, the workgroups of the launch): those slots depend on arrival order and are compared within a bound, every
        other slot (counts, normalisers, untouched sentinels) exactly."""
        st = torch.cuda.current_stream().cuda_stream
        VOCABS = [(512, 2), (80, 3), (576, 1)]   # the register paths; a ragged lane tail on the generic path; the streaming kernels

        def seeded(seed, n_tok, vf, nfac):
            g = torch.Generator().manual_seed(seed)
            mask_id = vf ** nfac
            labels = torch.randint(0, mask_id, (n_tok,), generator=g)
            ids = torch.where(torch.rand(n_tok, generator=g) < 0.5, torch.full_like(labels, mask_id), labels)   # about half are masked
            return g, mask_id, labels.cuda(), ids.cuda()

        T, S = 3, 5   # 15 and 45 tokens: the last workgroup of four tokens is partial, frame 0 is present
        for vf, nfac in VOCABS:
            for clips in (1, 3):
                n_tok, V = clips * T * S, vf * nfac
                g, mask_id, labels, ids = seeded(100 * vf + clips, n_tok, vf, nfac)
                src = (3.0 * torch.randn(n_tok, V, generator=g)).cuda()
                teacher = (3.0 * torch.randn(n_tok, V, generator=g)).cuda()
                ob = _lib.Objective(label_smoothing=0.1, z_loss=1e-4, n_frames=T)
                ob.frame_weight[:T] = [1.0, 0.0, 2.0]
                wg = (n_tok + 3) // 4

                def training_loss(obj, tau, atomic):
                    def fn():
                        logits, sums = src.clone(), torch.full((8,), 12345.0, dtype=torch.float64, device="cuda")
                        geom = (clips, T, S, vf, nfac, mask_id)
                        if tau is None:
                            rc = lib.genie_ce_objective(logits.data_ptr(), ids.data_ptr(), labels.data_ptr(), *geom, obj, sums.data_ptr(), st)
                        else:
                            ds = _lib.Distill(alpha=0.5, temperature=tau, teacher_logits=teacher.data_ptr())
                            rc = lib.genie_ce_distill(logits.data_ptr(), teacher.data_ptr(), ids.data_ptr(), labels.data_ptr(), *geom, obj, ds,
                                                      sums.data_ptr(), st)
                        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(sums).all())
                        return rc, {"d_logits": logits}, {"sums": (sums, atomic, min(wg, 2048))}
                    return fn
                tag = f"loss/{nfac}x{vf}/clips{clips}"
                record_case(f"{tag}/objective/neutral", training_loss(None, None, (0,)))
                record_case(f"{tag}/objective/struct", training_loss(ob, None, (0, 3)))
                for tau in (1.0, 2.0):
                    record_case(f"{tag}/distill/tau{tau:g}", training_loss(ob, tau, (0, 3, 5, 6)))

        # the two entry points that take a genie_cfg: the smallest geometry of GEOMETRIES with each vocabulary
        _, d, heads, T, S, B = GEOMETRIES[0]
        for vf, nfac in VOCABS:
            cfg = GenieConfig(num_layers=2, num_heads=heads, d_model=d, T=T, S=S, num_factored_vocabs=nfac, image_vocab_size=vf ** nfac,
                              qk_norm=False, use_mup=False, qkv_bias=True)
            c = _lib.make_cfg(cfg)
            V, t0 = vf * nfac, 1
            g, mask_id, targets, ids = seeded(7 * vf, B * T * S, vf, nfac)
            src = (3.0 * torch.randn(B, T - t0, S, V, generator=g)).cuda()
            for layout, lname in ((_lib.LAYOUT_TOKEN_MAJOR, "token"), (_lib.LAYOUT_BCTHW, "bcthw")):
                logits = src if layout == _lib.LAYOUT_TOKEN_MAJOR else src.permute(0, 3, 1, 2).contiguous()
                n_tok = B * (T - t0) * S
                wg = min((n_tok + 3) // 4, 2048) if layout == _lib.LAYOUT_TOKEN_MAJOR else (n_tok + 255) // 256
                for weighted in (False, True):
                    def evaluator_ce():
                        sums = torch.full((8,), 12345.0, dtype=torch.float64, device="cuda")
                        sums[:3] = 0.0   # the entry point adds to what it finds
                        rc = lib.genie_factored_ce(c, logits.data_ptr(), layout, targets.data_ptr(), ids.data_ptr() if weighted else 0, B, t0, T,
                                                   sums.data_ptr(), st)
                        assert bool(torch.isfinite(sums).all())
                        return rc, {}, {"sums": (sums, (0,), wg)}
                    record_case(f"loss/{nfac}x{vf}/factored_ce/{lname}/{'weighted' if weighted else 'all'}", evaluator_ce)
            K, N = 3, 2 * 3   # two clips of three branches: row i is scored against the tokens of clip i / K

            def score():
                rows = (3.0 * torch.randn(N, S, V, generator=torch.Generator().manual_seed(9 * vf))).cuda()
                nll, hits = (torch.full((N,), 12345.0, dtype=torch.float64, device="cuda") for _ in range(2))
                tok = torch.full((N, S), 12345.0, device="cuda")
                rc = lib.genie_score_logits(c, rows.data_ptr(), targets.data_ptr(), T * S, K, N, nll.data_ptr(), 1, hits.data_ptr(), tok.data_ptr(),
                                            S, st)
                assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(tok).all())
                return rc, {"nll": nll, "hits": hits, "token_nll": tok}
            record_case(f"loss/{nfac}x{vf}/score_logits", score)

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
        for T, Dh, B, S, H, ldm in TEMPORAL_BWD_CASES:
            d = H * Dh
            gen = torch.Generator().manual_seed(1000 * T + Dh + B * S * H)
            qkv = torch.randn(B, T, S, 3 * d, generator=gen).cuda()
            qk = qkv if ldm == 3 else torch.randn(B, T, S, 2 * d, generator=gen).cuda()
            d_out = torch.randn(B, T, S, d, generator=gen).cuda()

            def bwd():
                d_qkv = torch.full((B, T, S, 3 * d), 12345.0, device="cuda")   # an element the kernel leaves unwritten shows in the digest
                rc = lib.genie_temporal_attention_backward(qkv.data_ptr(), qk.data_ptr(), ldm * d, d_out.data_ptr(), d_qkv.data_ptr(), B, T, S,
                                                           d, H, Dh, Dh ** -0.5, torch.cuda.current_stream().cuda_stream)
                assert bool(torch.isfinite(d_qkv).all())
                return rc, {"d_qkv": d_qkv}
            record_case(f"temporal_bwd/T{T}/h{Dh}/B{B}S{S}H{H}/ld{ldm}d", bwd, keep_refused=True)
        loss_cases()
        with open(out_path, "w") as f:
            json.dump(record, f)
        return

    def loop_cases(tag, m, B):
        """Every loop entry point of csrc/generate_api.hip on one model (action_vocab_size 5; cond = None runs it unconditioned), called
        through ctypes on buffers of this function's own: every output starts sentinel-filled, every cache zeroed"""
        cfg = m.config
        T, S, nv = cfg.T, cfg.S, cfg.num_factored_vocabs
        V = cfg.factored_vocab_size * nv
        c, w = m._weights()[:2]
        st = torch.cuda.current_stream().cuda_stream
        clip = torch.from_numpy(synth.make_clips(B, cfg, seed=7)).cuda().view(B, T, S)
        table = m.action_embed.weight
        law = _lib.Sampling(0.7, 50, 0.9, 4.5)
        RANDOM, GREEDY, CONF = _lib.UNMASK_RANDOM, _lib.UNMASK_GREEDY, _lib.UNMASK_CONFIDENCE
        ws = torch.zeros(max([lib.genie_generate_guided_workspace_bytes(c, B, P) for P in (1, T // 2, T - 1)]
                             + [lib.genie_rollout_workspace_bytes(c, B, T - 1, 1)]
                             + [lib.genie_fanout_workspace_bytes(c, B, 3, P, 1) for P in (1, T // 2, T - 1)]), dtype=torch.uint8, device="cuda")

        def rand(seed, *shape):
            return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()

        def sent(dtype, *shape):
            return torch.full(shape, -7 if dtype == torch.int64 else 12345.0, dtype=dtype, device="cuda")

        def ptr(t):
            return 0 if t is None else t.data_ptr()

        def acts(seed, rows, cols):
            a = torch.from_numpy(np.random.default_rng(seed).integers(1, 5, (rows, cols))).cuda()
            fc = _lib.FrameCond(table=table.data_ptr(), ids=a.data_ptr(), n_actions=5)
            fc.keep = a
            return fc

        def guide(scale):
            return _lib.Guidance(scale, 0)

        def draws(temperature, steps, n, rows, seed=3):
            """(noise (n, steps - 1, rows, S), uniforms (n, steps, nv, rows, S) or None at temperature 0)"""
            return rand(seed, n, max(steps - 1, 1), rows, S), rand(seed + 1, n, steps, nv, rows, S) if temperature > 0 else None

        def case(name, fn, tokens=()):
            def checked():
                rc, outs = fn()
                if rc == 0:
                    torch.cuda.synchronize()
                    for k, v in outs.items():   # (equal digests of NaNs, or of a constant frame, would compare nothing)
                        assert not v.is_floating_point() or bool(torch.isfinite(v).all()), (tag, name, k)
                    for k in tokens:
                        assert int(outs[k].min()) != int(outs[k].max()), (tag, name, k, "every generated token is one id")
                return rc, outs
            record_case(f"{tag}/{name}", checked, keep_refused=True)

        # ---- genie_maskgit_generate_ex / _guided: (cond, sampling, guidance, then the keyword edits of a refused call)
        def maskgit(mode=RANDOM, temperature=0.0, sampling=None, guidance=None, cond=None, layout=_lib.LAYOUT_TOKEN_MAJOR, steps=3,
                    out_t=T // 2, want_logits=True, null_prompt=False, short=0, no_uniforms=False):
            def fn():
                prompt = clip.clone()
                prompt[:, out_t if 0 < out_t < T else 1:] = cfg.image_vocab_size
                nz, uni = draws(temperature, steps, 1, B)
                samples, flag = sent(torch.int64, B, S), torch.zeros(1, dtype=torch.int32, device="cuda")
                lg = sent(torch.float32, B * S * V) if want_logits else None
                guided = guidance is not None
                need = lib.genie_generate_guided_workspace_bytes(c, B, 1) if guided else lib.genie_workspace_bytes(c, B)
                args = [c, w, 0 if null_prompt else prompt.data_ptr(), B, out_t, steps, temperature, mode, ptr(nz), 0 if no_uniforms else ptr(uni),
                        samples.data_ptr(), ptr(lg), layout, flag.data_ptr(), ws.data_ptr(), need - short, st, cond, sampling]
                rc = lib.genie_maskgit_generate_guided(*args, guidance) if guided else lib.genie_maskgit_generate_ex(*args)
                outs = {"tokens": samples, "prompt": prompt, "status": flag}
                if want_logits:
                    outs["logits0"] = lg
                return rc, outs
            return fn
        for mode, mname in ((RANDOM, "random"), (GREEDY, "greedy"), (CONF, "confidence")):
            case(f"maskgit/{mname}/t0", maskgit(mode, layout=_lib.LAYOUT_TOKEN_MAJOR), tokens=("tokens",))
            case(f"maskgit/{mname}/law", maskgit(mode, 1.0, law, layout=_lib.LAYOUT_BCTHW), tokens=("tokens",))
        case("maskgit/conf_default_law", maskgit(CONF, 1.0, None, want_logits=False), tokens=("tokens",))
        case("maskgit/actions", maskgit(cond=acts(11, B, T)), tokens=("tokens",))
        case("maskgit/guided3", maskgit(CONF, 1.0, law, guide(3.0), acts(11, B, T)), tokens=("tokens",))
        case("maskgit/guided3/bcthw", maskgit(RANDOM, 0.0, None, guide(3.0), acts(11, B, T), layout=_lib.LAYOUT_BCTHW), tokens=("tokens",))
        case("maskgit/guided1", maskgit(RANDOM, 0.0, None, guide(1.0), acts(11, B, T)), tokens=("tokens",))
        case("maskgit/refused/null", maskgit(null_prompt=True))
        case("maskgit/refused/out_t", maskgit(out_t=T))
        case("maskgit/refused/out_t_and_guidance", maskgit(out_t=0, guidance=guide(3.0)))
        case("maskgit/refused/steps", maskgit(steps=0))
        case("maskgit/refused/mode", maskgit(mode=7))
        case("maskgit/refused/workspace", maskgit(short=1))
        case("maskgit/refused/workspace_guided", maskgit(guidance=guide(3.0), cond=acts(11, B, T), short=1))
        case("maskgit/refused/uniforms", maskgit(temperature=1.0, no_uniforms=True))
        case("maskgit/refused/guidance", maskgit(guidance=guide(3.0)))
        case("maskgit/refused/null_action", maskgit(guidance=_lib.Guidance(3.0, 5), cond=acts(11, B, T)))

        # ---- genie_generate_cached_ex / _guided
        Pc, nc = T // 2, min(T - T // 2, 3)

        def cached(mode=RANDOM, temperature=0.0, sampling=None, guidance=None, cond=None, tf=0, merge=1, want_logits=False, steps=2, P=Pc,
                   n=nc, null_ids=False, short=0, no_uniforms=False):
            def fn():
                ids = clip[:, :min(P + n, T)].contiguous()
                nz, uni = draws(temperature, steps, n, B)
                NB = 2 * B if guidance is not None and guidance.scale != 1.0 else B
                gen = sent(torch.int64, B, n, S)
                lg = sent(torch.float32, B, n, S, V) if want_logits else None
                cache = torch.zeros(lib.genie_prefix_cache_bytes(c, NB), dtype=torch.uint8, device="cuda")
                need = (lib.genie_generate_guided_workspace_bytes if NB != B else lib.genie_generate_workspace_bytes)(c, B, min(P, T))
                args = [c, w, 0 if null_ids else ids.data_ptr(), B, P, n, steps, temperature, mode, ptr(nz), 0 if no_uniforms else ptr(uni), tf,
                        merge, gen.data_ptr(), ptr(lg), cache.data_ptr(), cache.numel(), ws.data_ptr(), need - short, st, cond, sampling]
                rc = lib.genie_generate_cached_guided(*args, guidance) if guidance is not None else lib.genie_generate_cached_ex(*args)
                outs = {"tokens": gen, "cache": cache}
                if want_logits:
                    outs["logits0"] = lg
                return rc, outs
            return fn
        case("cached/merged", cached(), tokens=("tokens",))
        case("cached/unmerged/logits0", cached(merge=0, want_logits=True), tokens=("tokens",))
        case("cached/tf/logits0", cached(GREEDY, tf=1, want_logits=True), tokens=("tokens",))
        case("cached/law", cached(CONF, 1.0, law), tokens=("tokens",))
        case("cached/actions/steps1", cached(cond=acts(12, B, T), steps=1), tokens=("tokens",))
        case("cached/guided3", cached(RANDOM, 1.0, law, guide(3.0), acts(12, B, T), want_logits=True), tokens=("tokens",))
        case("cached/guided3/unmerged/tf", cached(CONF, 0.0, None, guide(3.0), acts(12, B, T), tf=1, merge=0), tokens=("tokens",))
        case("cached/guided1", cached(guidance=guide(1.0), cond=acts(12, B, T)), tokens=("tokens",))
        case("cached/refused/null", cached(null_ids=True))
        case("cached/refused/frames", cached(P=T - 1, n=2))
        case("cached/refused/workspace", cached(short=1))
        case("cached/refused/uniforms", cached(temperature=1.0, no_uniforms=True))
        case("cached/refused/guidance", cached(guidance=guide(3.0)))
        case("cached/refused/mode", cached(mode=7))

        # ---- genie_rollout_cached past the window: 3 windows; in one call, and split in mid-window with resume = 1
        if T == 4:
            rolls = [("keep2", 2, 2, 5)]
        else:
            rolls = [("keep8", T - 2, 8, 4), ("keep15", T - 2, T - 1, 4)]

        def rollout(P, keep, n, split, guidance=None, cond_seed=None, temperature=0.0, mode=RANDOM, sampling=None, steps=2, null_frames=False,
                    short=0, no_uniforms=False, f1_over=0):
            def fn():
                cap = P + n
                frames = torch.full((B, cap, S), cfg.image_vocab_size, dtype=torch.int64, device="cuda")
                frames[:, :P] = clip[:, :P]
                cond = acts(cond_seed, B, cap) if cond_seed else None
                guided = guidance is not None and guidance.scale != 1.0
                nz, uni = draws(temperature, steps, n, B)
                cache = torch.zeros(lib.genie_prefix_cache_bytes(c, 2 * B if guided else B), dtype=torch.uint8, device="cuda")
                need = lib.genie_rollout_workspace_bytes(c, B, max(P, min(keep, T - 1)), int(guided))   # the largest context of the call(s)
                rc = 0
                for f0, f1, resume in ([(P, P + 1, 0), (P + 1, cap, 1)] if split else [(P, cap + f1_over, 0)]):
                    if rc == 0:
                        rc = lib.genie_rollout_cached(c, w, 0 if null_frames else frames.data_ptr(), B, P, keep, cap, f0, f1, resume, steps,
                                                      temperature, mode, nz[f0 - P:].data_ptr(), 0 if uni is None or no_uniforms else uni[f0 - P:].data_ptr(),
                                                      1, cache.data_ptr(), cache.numel(), ws.data_ptr(), need - short, st, cond, sampling, guidance)
                return rc, {"tokens": frames, "cache": cache}
            return fn
        for rname, P, keep, n in rolls:
            for split in (0, 1):
                case(f"rollout/{rname}/split{split}", rollout(P, keep, n, split), tokens=("tokens",))
                case(f"rollout/{rname}/split{split}/guided3", rollout(P, keep, n, split, guide(3.0), 13, 1.0, CONF, law), tokens=("tokens",))
            case(f"rollout/{rname}/actions", rollout(P, keep, n, 0, None, 13), tokens=("tokens",))
        rname, P, keep, n = rolls[0]
        case("rollout/refused/null", rollout(P, keep, n, 0, null_frames=True))
        case("rollout/refused/frames", rollout(P, keep, n, 0, f1_over=1))
        case("rollout/refused/keep", rollout(P, T, n, 0))
        case("rollout/refused/workspace", rollout(P, keep, n, 0, short=1))
        case("rollout/refused/uniforms", rollout(P, keep, n, 0, temperature=1.0, no_uniforms=True))
        case("rollout/refused/guidance", rollout(P, keep, n, 0, guide(3.0)))

        # ---- genie_generate_fanout and genie_score_fanout over one trunk
        def fanout(K, P, n, guidance=None, cond_seed=None, temperature=0.0, mode=RANDOM, sampling=None, steps=2, merge=1, null_ids=False, short=0,
                   no_uniforms=False, short_branch=0):
            def fn():
                guided = guidance is not None and guidance.scale != 1.0
                NB = 2 * B if guided else B
                ids = clip[:, :min(P, T)].contiguous()
                cond = acts(cond_seed, B * K, T) if cond_seed else None
                nz, uni = draws(temperature, steps, n, B * K)
                gen = sent(torch.int64, B, K, n, S)
                trunk = torch.zeros(lib.genie_prefix_cache_bytes(c, NB), dtype=torch.uint8, device="cuda")
                branch = torch.zeros(max(lib.genie_fanout_branch_bytes(c, NB, K, min(n, T - 1)), 256), dtype=torch.uint8, device="cuda")
                need = lib.genie_fanout_workspace_bytes(c, B, K, min(P, T - 1), int(guided))
                rc = lib.genie_generate_fanout(c, w, 0 if null_ids else ids.data_ptr(), B, K, P, n, steps, temperature, mode, ptr(nz),
                                               0 if no_uniforms else ptr(uni), merge, gen.data_ptr(), trunk.data_ptr(), trunk.numel(), branch.data_ptr(),
                                               branch.numel() - short_branch, ws.data_ptr(), need - short, st, cond, sampling, guidance)
                return rc, {"tokens": gen, "trunk": trunk, "branch": branch}
            return fn
        nf = min(T - 1, 3)
        for K in (1, 3):
            case(f"fanout/K{K}/P1", fanout(K, 1, nf, temperature=1.0, sampling=law), tokens=("tokens",))
            case(f"fanout/K{K}/Plast/actions", fanout(K, T - 1, 1, cond_seed=14), tokens=("tokens",))
            case(f"fanout/K{K}/P1/actions/unmerged", fanout(K, 1, nf, cond_seed=14, mode=CONF, merge=0), tokens=("tokens",))
            case(f"fanout/K{K}/P1/guided3", fanout(K, 1, nf, guide(3.0), 14, 1.0, GREEDY, law), tokens=("tokens",))
            case(f"fanout/K{K}/Phalf/guided3", fanout(K, T // 2, T - T // 2 if T == 4 else 2, guide(3.0), 14), tokens=("tokens",))
        case("fanout/refused/null", fanout(3, 1, nf, null_ids=True))
        case("fanout/refused/frames", fanout(3, T - 1, 2))
        case("fanout/refused/workspace", fanout(3, 1, nf, short=1))
        case("fanout/refused/branch", fanout(3, 1, nf, short_branch=1))
        case("fanout/refused/uniforms", fanout(3, 1, nf, temperature=1.0, no_uniforms=True))
        case("fanout/refused/guidance", fanout(3, 1, nf, guide(3.0)))
        case("fanout/refused/K", fanout(0, 1, nf))

        def score(K, P, n, merge=1, cond_seed=None, per_token=True, want_hits=True, null_ids=False, short=0, short_trunk=0):
            def fn():
                ids = clip[:, :min(P + n, T)].contiguous()
                cond = acts(cond_seed, B * K, T) if cond_seed else None
                nll = sent(torch.float64, B, max(K, 1), n)
                hits = sent(torch.float64, B, max(K, 1), n) if want_hits else None
                tok = sent(torch.float32, B, max(K, 1), n, S) if per_token else None
                trunk = torch.zeros(lib.genie_prefix_cache_bytes(c, B), dtype=torch.uint8, device="cuda")
                branch = torch.zeros(max(lib.genie_fanout_branch_bytes(c, B, K, min(n, T - 1)), 256), dtype=torch.uint8, device="cuda")
                need = lib.genie_score_workspace_bytes(c, B, K, min(P, T - 1))
                rc = lib.genie_score_fanout(c, w, 0 if null_ids else ids.data_ptr(), B, K, P, n, merge, nll.data_ptr(), ptr(hits), ptr(tok),
                                            trunk.data_ptr(), trunk.numel() - short_trunk, branch.data_ptr(), branch.numel(), ws.data_ptr(),
                                            need - short, st, cond)
                outs = {"nll": nll, "trunk": trunk, "branch": branch}
                if want_hits:
                    outs["hits"] = hits
                if per_token:
                    outs["token_nll"] = tok
                return rc, outs
            return fn
        ns = T - T // 2 if T == 4 else 3
        for K in (1, 3):
            case(f"score/K{K}/merged", score(K, T // 2, ns))
            case(f"score/K{K}/unmerged/actions", score(K, T // 2, ns, merge=0, cond_seed=15, per_token=False))
            case(f"score/K{K}/P1/actions/nll_only", score(K, 1, 2, cond_seed=15, per_token=False, want_hits=False))
        case("score/refused/null", score(3, T // 2, ns, null_ids=True))
        case("score/refused/frames", score(3, T - 1, 2))
        case("score/refused/workspace", score(3, T // 2, ns, short=1))
        case("score/refused/trunk", score(3, T // 2, ns, short_trunk=1))
        case("score/refused/K", score(0, T // 2, ns))
        del ws
        torch.cuda.empty_cache()

    if battery == "loops":
        for gname, d, heads, T, S, precs, clips in LOOP_MODELS:
            for qk_norm in (False, True):
                cfg = GenieConfig(num_layers=2, num_heads=heads, d_model=d, T=T, S=S, num_factored_vocabs=2, qk_norm=qk_norm, use_mup=False,
                                  qkv_bias=True, action_vocab_size=5)
                sd = synth.make_state_dict(cfg, seed=5, law="conditioned")
                nonzero_biases(sd, 6)
                sd["action_embed.weight"] = (0.5 * np.random.default_rng(8).standard_normal(sd["action_embed.weight"].shape)).astype(np.float32)
                for prec in precs:
                    m = STMaskGIT(cfg, precision=prec).load_numpy_state_dict(sd).to("cuda")
                    for B in clips:
                        loop_cases(f"{gname}/{'qknorm' if qk_norm else 'ln'}/{prec}/B{B}", m, B)
                    del m
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
    watched = {"train": TRAIN_WATCHED, "loops": LOOPS_WATCHED}.get(battery, WATCHED)
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
        bad += sums_differ(name, ca.get("sums", {}), cb.get("sums", {}))
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


def sums_differ(name, sa, sb):
    """The f64 sums of a loss case -> the number of differences.  A slot that workgroups add to with atomics holds non-negative addends in
    arrival order: two orders differ by at most (workgroups) * 2^-52 relative.  Every other slot must be equal."""
    if sorted(sa) != sorted(sb):
        print(f"DIFF {name}: sums recorded {sorted(sa)} != {sorted(sb)}")
        return 1
    bad = 0
    for k in sa:
        va, vb = ([float.fromhex(x) for x in s[k]["values"]] for s in (sa, sb))
        for i, (x, y) in enumerate(zip(va, vb)):
            bound = sa[k]["workgroups"] * 2.0 ** -52 * max(abs(x), abs(y)) if i in sa[k]["atomic"] else 0.0
            if len(va) != len(vb) or not abs(x - y) <= bound:
                bad += 1
                print(f"DIFF {name}: {k}[{i}]: {x!r} != {y!r} (bound {bound:g})")
    return bad


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
    ap.add_argument("--battery", default="all", choices=["all", "inference", "train", "loops"],
                    help="each battery runs in its own pair of child processes; a failing one ends the run")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.battery)
    if not (a.library_a and a.library_b):
        ap.error("two libraries")
    for battery in (["inference", "train", "loops"] if a.battery == "all" else [a.battery]):
        status = run_battery(a, battery)
        if status:
            return status
    print("PASS: zero differing bits, identical return codes, identical kernel tables")
    return 0


if __name__ == "__main__":
    sys.exit(main())
