#!/usr/bin/env python3
"""Time the HIP training step (forward + backward + clip + AdamW) on synthetic clips.
   python tools/bench_train.py --config c138 --batch 8 --steps 3
   python tools/bench_train.py --config c138 --precision bf16 --batch 8 --breakdown --ema_decay 0.999 [--ema_unfused]
   python tools/bench_train.py --config c138 --layers 4 --batch 8 --optimizer muon"""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = lambda n: importlib.import_module("1xgpt_amd" + ("." + n if n else ""))  # noqa: E731


def unfuse_ema(tr, lib, _lib):
    """Replace the trainer's fused AdamW + EMA launch by the two-pass pair it stands for (same bits; a yardstick for the fusion)."""
    class Unfused:
        def __getattr__(self, name):
            return getattr(lib, name)

        @staticmethod
        def genie_adamw_ema_step(p, g, m, v, ema, n, *rest):
            *adam, omd, st = rest
            rc = lib.genie_adamw_step(p, g, m, v, n, *adam, st)
            return rc or lib.genie_ema_update(ema, p, n, omd, st)
    tr.lib = Unfused()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c138", choices=["c35", "c138"])
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--T", type=int, default=0, help="frames per clip (default: the config's own 16); 32 and 64 train too")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--precision", default="exact", choices=["exact", "f16x3", "bf16"])
    ap.add_argument("--recompute", action="store_true",
                    help="keep one checkpoint per layer and rebuild each layer's activations in its backward (GenieTrainer(recompute=True))")
    ap.add_argument("--mlp_drop", type=float, default=0.0, help="train with MLP dropout of this probability (config.mlp_drop)")
    ap.add_argument("--label_smoothing", type=float, default=0.0, help="train with this label smoothing (GenieTrainer(label_smoothing=...))")
    ap.add_argument("--z_loss", type=float, default=0.0, help="train with this z-loss weight (GenieTrainer(z_loss=...))")
    ap.add_argument("--frame_loss_weights", type=str, default=None,
                    help="comma-separated per-frame loss weights, one per frame (GenieTrainer(frame_weights=...))")
    ap.add_argument("--ema_decay", type=float, default=None, help="time the step with an EMA of the weights (GenieTrainer(ema_decay=...))")
    ap.add_argument("--ema_unfused", action="store_true",
                    help="bench only, with --ema_decay: run the optimizer as genie_adamw_step followed by genie_ema_update per range (two passes) "
                         "instead of the one fused launch the trainer makes")
    ap.add_argument("--action_dim", type=int, default=0, help="condition the model on random per-frame action vectors of this many values")
    ap.add_argument("--train_only", type=str, default=None, metavar="P[,P...]",
                    help="train only the tensors matching these fnmatch patterns over state-dict names (GenieTrainer(trainable=...))")
    ap.add_argument("--freeze", type=str, default=None, metavar="P[,P...]", help="freeze the tensors matching these patterns")
    ap.add_argument("--lora_rank", type=int, default=0, help="train adapters of this rank instead of the weights (GenieTrainer(lora=LoraConfig(...)))")
    ap.add_argument("--lora_targets", type=str, default="decoder.layers.*", metavar="P[,P...]", help="with --lora_rank: the adapted Linears")
    ap.add_argument("--optimizer", default="adamw", choices=["adamw", "muon"],
                    help="muon: Muon on the Linear weights of every layer, AdamW on the rest (GenieTrainer(muon=MuonConfig()))")
    ap.add_argument("--muon_ns_steps", type=int, default=5, help="with --optimizer muon: Newton-Schulz iterations")
    ap.add_argument("--teacher", default=None, choices=["c35", "c138"],
                    help="distil from a teacher of this shape (synthetic weights; GenieTrainer(teacher=...)): its forward runs in every step")
    ap.add_argument("--teacher_precision", default=None, choices=["exact", "f16x3", "bf16"], help="the teacher's precision (default: --precision)")
    ap.add_argument("--distill_alpha", type=float, default=0.5, help="with --teacher: the mix of the distillation loss")
    ap.add_argument("--distill_temperature", type=float, default=1.0, help="with --teacher: the temperature of the distillation loss")
    a = ap.parse_args()
    cfgm, syn, _lib = pkg("config"), pkg("synthetic"), pkg("_lib")
    cfg = cfgm.c138() if a.config == "c138" else cfgm.c35()
    cfg.qk_norm = False
    if a.layers:
        cfg.num_layers = a.layers
    if a.T:
        cfg.T = a.T
    if a.action_dim:
        cfg = cfgm.GenieConfig(**{**vars(cfg), "action_dim": a.action_dim})
    cfg.mlp_drop = a.mlp_drop
    sd = syn.make_state_dict(cfg, seed=0, law="init")
    model = pkg("st_mask_git").STMaskGIT(cfg, precision=a.precision).load_numpy_state_dict(sd).to("cuda")
    fw = None if a.frame_loss_weights is None else [float(v) for v in a.frame_loss_weights.split(",")]
    trainable = None
    if a.train_only or a.freeze:
        try:
            trainable = sorted(pkg("train").select_trainable([n for n, _ in model.named_parameters()], a.train_only, a.freeze))
        except ValueError as e:
            ap.error(str(e))
    teacher = None
    if a.teacher:
        tcfg = cfgm.c138() if a.teacher == "c138" else cfgm.c35()
        tcfg.qk_norm, tcfg.T = False, cfg.T
        teacher = pkg("st_mask_git").STMaskGIT(tcfg, precision=a.teacher_precision or a.precision)
        teacher = teacher.load_numpy_state_dict(syn.make_state_dict(tcfg, seed=5, law="init")).to("cuda")
    tr = pkg("train").GenieTrainer(model, lr=1e-4, max_grad_norm=1.0, recompute=a.recompute, ema_decay=a.ema_decay,
                                   label_smoothing=a.label_smoothing, z_loss=a.z_loss, frame_weights=fw, trainable=trainable,
                                   teacher=teacher, distill_alpha=a.distill_alpha if teacher is not None else 0.0,
                                   distill_temperature=a.distill_temperature,
                                   lora=pkg("train").LoraConfig(rank=a.lora_rank, alpha=2.0 * a.lora_rank, targets=a.lora_targets) if a.lora_rank else None,
                                   muon=pkg("train").MuonConfig(ns_steps=a.muon_ns_steps) if a.optimizer == "muon" else None)
    if a.lora_rank:   # B = 0 would make dA exactly zero: time the step on adapters that have moved
        sd = tr.adapter_state_dict()
        g = torch.Generator(device="cuda").manual_seed(3)
        tr.load_adapter_state_dict({n: (t if n.endswith(".lora_A") else 0.02 * torch.randn(t.shape, generator=g, device="cuda")) for n, t in sd.items()})
        print(f"lora rank {a.lora_rank}: {len(tr.lora_targets)} adapted Linears, {tr.n_train} trainable elements of {tr.n_flat} flat; "
              f"optimizer state {8 * tr.n_train} bytes, all-reduce {4 * tr.n_train} bytes, {len(tr.adam_runs)} AdamW launches")
    lib = _lib.load()
    if a.ema_unfused:
        if a.ema_decay is None:
            ap.error("--ema_unfused needs --ema_decay")
        unfuse_ema(tr, lib, _lib)
    opt_events = []   # the optimizer step (sum of squares, AdamW [+ EMA], 16-bit repack) between two events of its own, no host sync
    inner = tr.optimizer_step

    def timed_optimizer_step():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = inner()
        ev[1].record()
        opt_events.append(ev)
        return out
    tr.optimizer_step = timed_optimizer_step
    teacher_events = []   # the teacher's forward (inside forward_backward) between two events of its own
    inner_distill = tr._distill

    def timed_distill(*args):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = inner_distill(*args)
        ev[1].record()
        teacher_events.append(ev)
        return out
    if teacher is not None:
        tr._distill = timed_distill
    ids = torch.from_numpy(syn.make_clips(a.batch, cfg, seed=1)).cuda()
    collate = pkg("data").maskgit_collate
    torch.manual_seed(0)
    import random
    random.seed(0)
    vecs = torch.randn(a.batch, cfg.T, a.action_dim, generator=torch.Generator().manual_seed(2)).cuda() if a.action_dim else None
    batch = collate(ids, cfg, action_vectors=vecs)
    for _ in range(a.warmup):
        out = tr.train_step(batch)
    torch.cuda.synchronize()
    opt_events.clear()
    teacher_events.clear()
    if a.breakdown:
        lib.genie_profile_enable(0x1F)
        lib.genie_profile_reset()
    t0 = time.perf_counter()
    step_events = []   # every whole step between two events of its own as well: the median and the range beside the mean
    for _ in range(a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = tr.train_step(batch)
        ev[1].record()
        step_events.append(ev)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    tokens = a.batch * cfg.T * cfg.S
    n_params = sum(p.numel() for p in model.parameters())
    flops = 6.0 * n_params * tokens  # the reference's own estimate (train.py:543)
    act_bytes = [lib.genie_train_activation_bytes_ex(tr.cfg, a.batch, m) for m in (0, 1)]
    ema = "off" if a.ema_decay is None else f"{a.ema_decay:g}" + ("(unfused)" if a.ema_unfused else "")
    objective = "off" if tr._objective is None else (f"eps={a.label_smoothing:g},zeta={a.z_loss:g},weights={'on' if tr.frame_weights else 'off'}"
                                                    f" (ce {float(out['ce']):.4f})")
    print(f"{a.config} L={cfg.num_layers} T={cfg.T} B={a.batch} recompute={int(a.recompute)} mlp_drop={a.mlp_drop:g} ema={ema} objective={objective}: {dt*1e3:.3f} ms/step, {tokens/dt:.0f} tokens/s, "
          f"{flops/dt/1e12:.1f} TFLOP/s (6ND), loss {float(out['loss']):.4f}, |g| {float(out['grad_norm']):.4f}, "
          f"acts {tr._acts.numel()/2**30:.1f} GiB, ws {tr._ws.numel()/2**30:.1f} GiB, "
          f"activation bytes saved / recomputed {act_bytes[0]} / {act_bytes[1]}")
    sms = sorted(e0.elapsed_time(e1) for e0, e1 in step_events)
    print(f"  whole step by events: median {sms[len(sms) // 2]:.3f} ms (min {sms[0]:.3f}, max {sms[-1]:.3f}) over {len(sms)} steps")
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in opt_events)
    print(f"  optimizer_step: AdamW launches {len(tr.adam_runs) * (2 if a.ema_unfused else 1)}, {sum(ms) / len(ms):.3f} ms/step "
          f"(min {ms[0]:.3f}, median {ms[len(ms) // 2]:.3f}, max {ms[-1]:.3f}; {tr.n_flat * 4 / 1e9:.3f} GB per flat f32 buffer)")
    if tr.muon is not None:
        shapes = sorted({(it.rows, it.cols) for it in tr.muon_items})
        flop = sum(tr.muon.ns_steps * (4.0 * min(it.rows, it.cols) ** 2 * max(it.rows, it.cols) + 2.0 * min(it.rows, it.cols) ** 3) for it in tr.muon_items)
        print(f"  muon: {len(tr.muon_names)} tensors = {len(tr.muon_items)} matrices of shapes {shapes} in {len(tr._muon_tables)} tables, "
              f"{tr.muon_launches()} launches per step beside the AdamW ones, {flop / 1e12:.3f} TFLOP of iterations per step "
              f"(at least {flop / 157e12 * 1e3:.2f} ms at the 157 TFLOP/s f32 peak), workspace {tr._muon_ws.numel() / 2**20:.1f} MiB")
    if teacher is not None:
        tms = sorted(e0.elapsed_time(e1) for e0, e1 in teacher_events)
        print(f"  distillation: teacher {a.teacher} {a.teacher_precision or a.precision}, alpha {a.distill_alpha:g}, tau {a.distill_temperature:g}: "
              f"teacher forward {sum(tms) / len(tms):.3f} ms/step (min {tms[0]:.3f}, max {tms[-1]:.3f}) = {sum(tms) / len(tms) / (dt * 1e3):.1%} "
              f"of the step; kd {float(out['kd']):.4f}, teacher_ce {float(out['teacher_ce']):.4f}, ce {float(out['ce']):.4f}")
    n_state = 2 + (tr.ema is not None)   # exp_avg, exp_avg_sq (and the average): one f32 per trainable element each
    print(f"  trainable {len(tr.trainable)} of {len(tr.order)} tensors, backward layers {cfg.num_layers - tr.layout.stop} of {cfg.num_layers}, "
          f"embedding backward {'on' if tr.layout.embed else 'off'}: gradient buffer = all-reduce traffic per step {tr.n_train * 4} bytes, "
          f"optimizer state {n_state * tr.n_train * 4} bytes (all-trainable: {tr.n_flat * 4} and {n_state * tr.n_flat * 4})")
    if a.breakdown:
        import ctypes as C
        buf = (C.c_double * 4)()
        for cls, name in enumerate(["gemm", "attn_spatial", "attn_temporal", "layernorm", "other"]):
            lib.genie_profile_read(cls, buf)
            if buf[0]:
                print(f"  {name:14s} launches {int(buf[0]):6d}  {buf[1]/a.steps:9.2f} ms/step  "
                      f"{buf[2]/max(buf[1],1e-9)/1e9:8.1f} TFLOP/s  {buf[3]/max(buf[1],1e-9)/1e6:8.1f} GB/s")
        if tr._objective is not None or tr._distilling:   # the general loss kernels by name (class "other"; the neutral step's are not bracketed)
            kbuf = C.create_string_buffer(16384)
            _lib.check(lib.genie_profile_kernels(_lib.KC_OTHER, kbuf, len(kbuf)), "profile_kernels")
            for ln in kbuf.value.decode().splitlines():
                name, n, ms = ln.split("\t")[:3]
                if name in ("ce_objective_kernel", "count_frames_kernel", "ce_distill_kernel"):
                    print(f"    {name:22s} launches {float(n) / a.steps:6.0f}  {float(ms) / a.steps:9.4f} ms/step")
        if a.mlp_drop:   # the dropout kernels by name (class "other"): launches and milliseconds per step
            kbuf = C.create_string_buffer(16384)
            _lib.check(lib.genie_profile_kernels(_lib.KC_OTHER, kbuf, len(kbuf)), "profile_kernels")
            for ln in kbuf.value.decode().splitlines():
                name, n, ms = ln.split("\t")[:3]
                if name.startswith("drop_"):
                    print(f"    {name:22s} launches {float(n) / a.steps:6.0f}  {float(ms) / a.steps:9.4f} ms/step")
        lib.genie_profile_enable(0)


if __name__ == "__main__":
    main()
