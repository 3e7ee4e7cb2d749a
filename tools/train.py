#!/usr/bin/env python3
"""CLI counterpart of the reference's `python train.py` (train.py:396-737) on the MI355X path: the same argument names for
what is built (dataset windows, GenieConfig json, AdamW + decay grouping, linear / custom_cosine schedules, gradient
accumulation, clipping, periodic teacher-forced eval, `save_pretrained` checkpoints with the optimizer state, resume).
Not built: accelerate/wandb logging, torch.compile, the Llama baseline, MuAdamW (--mu_transfer).
--ema_decay D keeps an exponential moving average of the weights (updated inside the AdamW launch): every checkpoint directory gains an
ema/ sub-directory that STMaskGIT.from_pretrained loads like any checkpoint, --eval_ema also evaluates with the averaged weights, and
--resume_from_checkpoint restores the average from trainer_state.pt.
--label_smoothing E, --z_loss Z and --frame_loss_weights w0,w1,... shape the training loss (per factor F.cross_entropy(label_smoothing=E)
+ Z * logsumexp^2, weighted per frame); the step line then prints the plain cross-entropy as `ce` next to train_loss, and evaluation
reports the plain cross-entropy as before.
--teacher_path DIR --distill_alpha A --distill_temperature TAU distil a trained model into this one: the loss becomes (1 - A) * the loss
above + A * TAU^2 KL(teacher || student) at temperature TAU, inside the same loss kernel; the teacher (a from_pretrained directory with
the student's window and vocabulary, any depth and width, --teacher_precision) runs one inference forward per micro-batch on the ids the
student sees.  The step line then prints `kd` (the KL per masked token) and `teacher_ce` (the teacher's own cross-entropy there).
A config with action_vocab_size > 0 trains an action-conditioned model on the datasets' actions.bin (refused without one);
--warmstart_path from an unconditioned checkpoint then starts from a zero action table.

  python tools/train.py --genie_config genie/configs/magvit_n32_h8_d256.json --train_data_dir data/train_v1.1 \\
      --val_data_dir data/val_v1.1 --output_dir out --per_device_train_batch_size 8 --max_train_steps 1000
  python tools/train.py --synthetic 64 --output_dir /tmp/out --max_train_steps 5        # offline smoke: synthetic clips
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/train.py ...   # data-parallel (RCCL)
"""
import argparse
import importlib
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def parse_args():
    p = argparse.ArgumentParser(description="Train a GENIE spatio-temporal MaskGIT model (MI355X path).")
    p.add_argument("--train_data_dir", type=str, default="data/train_v1.1")
    p.add_argument("--val_data_dir", type=str, default="data/val_v1.1")
    p.add_argument("--window_size", type=int, default=None,
                   help="frames per clip (default 16); a power of two up to 64.  With --synthetic: overrides the T of the model shape when given")
    p.add_argument("--stride", type=int, default=15)
    p.add_argument("--filter_overlaps", action="store_true")
    p.add_argument("--genie_config", type=str, help="GenieConfig json")
    p.add_argument("--warmstart_path", type=str, default=None)
    p.add_argument("--resume_from_checkpoint", type=str, default=None,
                   help="a step_N / final_checkpt directory written by this script (weights + trainer_state.pt)")
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--per_device_train_batch_size", type=int, default=4)
    p.add_argument("--per_device_eval_batch_size", type=int, default=4)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--recompute_activations", action="store_true",
                   help="keep one checkpoint per layer and rebuild each layer's activations in its backward: the same numbers from "
                        "about a tenth of the activation memory, for about one more forward of time")
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--num_train_epochs", type=int, default=1)
    p.add_argument("--max_train_steps", type=int, default=None)
    p.add_argument("--max_eval_steps", type=int, default=int(1e10))
    p.add_argument("--eval_every_n_steps", type=int, default=1000)
    p.add_argument("--lr_scheduler_type", type=str, default="linear", choices=["linear", "constant", "custom_cosine"])
    p.add_argument("--num_warmup_steps", type=int, default=0)
    p.add_argument("--max_grad_norm", type=float, default=1.0)
    p.add_argument("--adam_beta_1", type=float, default=0.9)
    p.add_argument("--adam_beta_2", type=float, default=0.999)
    p.add_argument("--adam_eps", type=float, default=1e-8)
    p.add_argument("--checkpointing_steps", type=str, default="1000")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--mu_transfer", action="store_true")
    p.add_argument("--precision", choices=["exact", "f16x3", "bf16"], default="bf16",
                   help="bf16 = what the reference computes under --mixed_precision bf16; f16x3 keeps f32-class gradients")
    p.add_argument("--action_dropout", type=float, default=0.0,
                   help="share of the training clips whose actions are replaced by --null_action (trains the null action of "
                        "classifier-free guidance; action-conditioned configs only)")
    p.add_argument("--mlp_drop", type=float, default=None,
                   help="MLP dropout probability in [0, 1) of the training step (overrides the config's mlp_drop; evaluation and "
                        "generation ignore it)")
    p.add_argument("--dropout_seed", type=int, default=0,
                   help="seed of the dropout masks (each rank adds its rank); saved with the trainer state")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing in [0, 1) of the training loss, per factor as F.cross_entropy(label_smoothing=); evaluation "
                        "reports the plain cross-entropy")
    p.add_argument("--z_loss", type=float, default=0.0,
                   help="weight >= 0 of the z-loss, z_loss * logsumexp^2 per softmax (e.g. 1e-4): keeps the readout's log-partition "
                        "from drifting in bf16 runs")
    p.add_argument("--frame_loss_weights", type=str, default=None,
                   help="comma-separated loss weights >= 0, one per frame of the window (w0,w1,...; frame 0 is never counted): the "
                        "loss is the weighted mean over the masked tokens")
    p.add_argument("--teacher_path", type=str, default=None, metavar="DIR",
                   help="distil from this model (a save_pretrained directory with the student's T, S and vocabulary; any depth and width)")
    p.add_argument("--teacher_precision", choices=["exact", "f16x3", "bf16"], default=None,
                   help="precision of the teacher's forward (default: --precision)")
    p.add_argument("--distill_alpha", type=float, default=0.0,
                   help="mix in [0, 1] of the distillation loss: (1 - alpha) * hard loss + alpha * tau^2 KL(teacher || student); needs "
                        "--teacher_path when > 0")
    p.add_argument("--distill_temperature", type=float, default=1.0, help="temperature tau > 0 of both softmaxes in the KL")
    p.add_argument("--ema_decay", type=float, default=None,
                   help="keep an exponential moving average of the weights with this decay in [0, 1] (e.g. 0.999); checkpoints gain an "
                        "ema/ directory with the averaged weights")
    p.add_argument("--ema_warmup", action="store_true",
                   help="with --ema_decay: use min(decay, (1 + n) / (10 + n)) at update n, so that the average follows the weights early on")
    p.add_argument("--eval_ema", action="store_true",
                   help="with --ema_decay: run the periodic evaluation with the averaged weights as well and log both losses")
    p.add_argument("--action_dim", type=int, default=0,
                   help="condition the model on continuous per-frame action vectors of this many values (the datasets' states.bin; "
                        "random vectors under --synthetic); with --action_dropout a dropped clip reads the model's learned null row")
    p.add_argument("--train_only", type=str, default=None, metavar="P[,P...]",
                   help="fine-tune: train only the tensors whose state-dict name matches one of these fnmatch patterns (e.g. "
                        "'action_*' or 'decoder.layers.3[01].*,out_x_proj.*'); the rest are frozen and cost no gradient, optimizer state, "
                        "all-reduce or repack (GenieTrainer(trainable=...))")
    p.add_argument("--freeze", type=str, default=None, metavar="P[,P...]",
                   help="freeze the tensors matching these patterns (applied after --train_only)")
    p.add_argument("--lr_scale", type=str, default=None, metavar="P=F[,P=F...]",
                   help="learning-rate factors by pattern, first match wins (e.g. 'action_*=10'): lr * F for the tensors matching P")
    p.add_argument("--lora_rank", type=int, default=0,
                   help="train low-rank adapters of this rank (1 .. 64) on the Linears --lora_targets selects instead of the weights: "
                        "the adapters alone train (plus what --train_only names), checkpoints gain an adapter/ directory "
                        "(adapter_config.json + adapter.safetensors) beside the merged weights; resuming needs the base model as "
                        "--warmstart_path")
    p.add_argument("--lora_alpha", type=float, default=None, help="the adapters' scale is alpha / rank (default: 2 * rank)")
    p.add_argument("--lora_targets", type=str, default="decoder.layers.*", metavar="P[,P...]",
                   help="fnmatch patterns over the Linear weight names (six per layer and out_x_proj.weight)")
    p.add_argument("--optimizer", choices=["adamw", "muon"], default="adamw",
                   help="muon: Muon (momentum and a Newton-Schulz orthogonalisation of the update) on the trainable Linear weights "
                        "--muon_targets selects, AdamW on everything else, under the one learning-rate schedule")
    p.add_argument("--muon_momentum", type=float, default=0.95)
    p.add_argument("--muon_ns_steps", type=int, default=5, help="Newton-Schulz iterations (0 .. 99)")
    p.add_argument("--muon_targets", type=str, default="decoder.layers.*", metavar="P[,P...]",
                   help="fnmatch patterns over the Linear weight names (six per layer and out_x_proj.weight)")
    p.add_argument("--muon_adjust_lr", choices=["match_rms_adamw", "original"], default="match_rms_adamw",
                   help="lr * 0.2 sqrt(max(rows, cols)) or lr * sqrt(max(1, rows / cols))")
    p.add_argument("--muon_no_nesterov", action="store_true", help="plain momentum instead of Nesterov's")
    p.add_argument("--null_action", type=int, default=None, help="row of the action table that stands for 'no action'")
    p.add_argument("--synthetic", type=int, default=0, help="train on N synthetic clips (no dataset on disk)")
    p.add_argument("--model", choices=["c138", "c35", "tiny"], default="c35", help="shape when no --genie_config is given")
    return p.parse_args()


def main():
    args = parse_args()
    if args.ema_decay is None and (args.ema_warmup or args.eval_ema):
        sys.exit("train.py: --ema_warmup and --eval_ema need --ema_decay")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay <= 1.0:
        sys.exit(f"train.py: --ema_decay {args.ema_decay} is not in [0, 1]")
    frame_weights = None
    if args.frame_loss_weights is not None:
        try:
            frame_weights = [float(v) for v in args.frame_loss_weights.split(",")]
        except ValueError:
            sys.exit(f"train.py: --frame_loss_weights {args.frame_loss_weights!r} is not a comma-separated list of numbers")
    try:   # the trainer's own rules, before anything is built
        importlib.import_module("1xgpt_amd.train").objective_settings(args.label_smoothing, args.z_loss, frame_weights)
    except ValueError as e:
        sys.exit(f"train.py: --label_smoothing / --z_loss / --frame_loss_weights: {e}")
    try:
        importlib.import_module("1xgpt_amd.train").distill_settings(args.distill_alpha, args.distill_temperature)
    except ValueError as e:
        sys.exit(f"train.py: --distill_alpha / --distill_temperature: {e}")
    if args.distill_alpha > 0 and not args.teacher_path:
        sys.exit(f"train.py: --distill_alpha {args.distill_alpha} needs --teacher_path")
    lora = None
    if args.lora_rank:
        try:
            lora = importlib.import_module("1xgpt_amd.train").LoraConfig(
                rank=args.lora_rank, alpha=2.0 * args.lora_rank if args.lora_alpha is None else args.lora_alpha,
                targets=args.lora_targets, seed=args.seed or 0)
        except ValueError as e:
            sys.exit(f"train.py: --lora_rank / --lora_alpha / --lora_targets: {e}")
        if args.freeze:
            sys.exit("train.py: --freeze has no meaning with --lora_rank (the adapters train, and what --train_only names)")
        if args.resume_from_checkpoint and not args.warmstart_path:
            sys.exit("train.py: resuming an adapter run needs the base model as --warmstart_path (the checkpoint holds merged weights)")
    muon = None
    if args.optimizer == "muon":
        try:
            muon = importlib.import_module("1xgpt_amd.train").MuonConfig(
                momentum=args.muon_momentum, nesterov=not args.muon_no_nesterov, ns_steps=args.muon_ns_steps, targets=args.muon_targets,
                adjust_lr=args.muon_adjust_lr)
        except ValueError as e:
            sys.exit(f"train.py: --muon_momentum / --muon_ns_steps / --muon_targets / --muon_adjust_lr: {e}")
    if args.mu_transfer:
        raise NotImplementedError("--mu_transfer needs the un-vendored mup fork (MuAdamW, set_base_shapes): not built")
    P = lambda n: importlib.import_module("1xgpt_amd." + n)  # noqa: E731
    dist_mod, cfgmod, synth, datamod, trainmod = P("distributed"), P("config"), P("synthetic"), P("data"), P("train")
    STMaskGIT = P("st_mask_git").STMaskGIT
    rank, world, local_rank = dist_mod.init_distributed()
    dev = torch.device("cuda", dist_mod.local_device_index(local_rank))
    torch.cuda.set_device(dev)
    if args.seed is not None:
        import random
        torch.manual_seed(args.seed)  # rank-independent while the model is built (the per-rank offset follows below)
        random.seed(args.seed)  # the collator's branch draws are host-side: keep the ranks in step

    # ---- data (train.py:421-436)
    get_train_acts = get_eval_acts = None   # per-frame actions (action-conditioned configs)
    if args.synthetic:
        cfg = (cfgmod.GenieConfig.from_pretrained(args.genie_config) if args.genie_config else
               {"c138": cfgmod.c138, "c35": cfgmod.c35,
                "tiny": lambda: cfgmod.GenieConfig(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2,
                                                   qk_norm=False, num_prompt_frames=2)}[args.model]())
        if args.window_size is not None:
            cfg = cfgmod.GenieConfig(**{**vars(cfg), "T": args.window_size})
        if args.action_dim:
            cfg = cfgmod.GenieConfig(**{**vars(cfg), "action_dim": args.action_dim})
        train_clips = torch.from_numpy(synth.make_clips(args.synthetic, cfg, seed=1))
        eval_clips = train_clips[: max(1, args.synthetic // 8)]
        get_train = lambda idx: train_clips[idx]  # noqa: E731
        get_eval = lambda idx: eval_clips[idx]  # noqa: E731
        n_train, n_eval = len(train_clips), len(eval_clips)
        if cfg.action_vocab_size:   # synthetic per-frame actions
            g = torch.Generator().manual_seed(2)
            train_acts = torch.randint(0, cfg.action_vocab_size, (len(train_clips), cfg.T), generator=g)
            get_train_acts = lambda idx: train_acts[idx]  # noqa: E731
            get_eval_acts = lambda idx: train_acts[: len(eval_clips)][idx]  # noqa: E731
        if cfg.action_dim:   # synthetic per-frame action vectors
            train_vecs = torch.randn(len(train_clips), cfg.T, cfg.action_dim, generator=torch.Generator().manual_seed(2))
            get_train_acts = lambda idx: train_vecs[idx]  # noqa: E731
            get_eval_acts = lambda idx: train_vecs[: len(eval_clips)][idx]  # noqa: E731
    else:
        if args.window_size is None:
            args.window_size = 16
        tds = datamod.RawTokenDataset(args.train_data_dir, window_size=args.window_size, stride=args.stride,
                                      filter_overlaps=args.filter_overlaps)
        eds = datamod.RawTokenDataset(args.val_data_dir, window_size=args.window_size, stride=args.stride,
                                      filter_overlaps=True)
        assert all(tds.metadata[k] == eds.metadata[k] for k in ("s", "vocab_size", "hz"))
        cfg = cfgmod.GenieConfig.from_pretrained(args.genie_config)
        cfg.image_vocab_size, cfg.T, cfg.S = tds.metadata["vocab_size"], args.window_size, tds.metadata["s"] ** 2
        cfg.__post_init__()
        if args.action_dim:
            cfg = cfgmod.GenieConfig(**{**vars(cfg), "action_dim": args.action_dim})
        get_train, get_eval, n_train, n_eval = tds.batch, eds.batch, len(tds), len(eds)
        if cfg.action_dim:
            for name, ds in (("train", tds), ("val", eds)):
                if ds.action_vectors is None or ds.action_vectors.shape[1] != cfg.action_dim:
                    sys.exit(f"train.py: the config takes action vectors (action_dim {cfg.action_dim}) but the {name} dataset has no "
                             f"states.bin of that width")
            get_train_acts, get_eval_acts = tds.action_vector_batch, eds.action_vector_batch
        if cfg.action_vocab_size:
            for name, ds in (("train", tds), ("val", eds)):
                if ds.actions is None:
                    sys.exit(f"train.py: the config is action-conditioned (action_vocab_size {cfg.action_vocab_size}) but the "
                             f"{name} dataset has no actions.bin")
            get_train_acts, get_eval_acts = tds.action_batch, eds.action_batch

    if frame_weights is not None and len(frame_weights) != cfg.T:
        sys.exit(f"train.py: --frame_loss_weights has {len(frame_weights)} entries, the window has {cfg.T} frames")
    # (an adapter run resumes on the base model: the adapters and the optimizer state come from the checkpoint further down)
    load_from = args.warmstart_path if lora is not None else (args.resume_from_checkpoint or args.warmstart_path)
    warm_actions = cfg.action_vocab_size if (args.warmstart_path and (lora is not None or not args.resume_from_checkpoint)) else None
    warm_dim = cfg.action_dim if (args.warmstart_path and (lora is not None or not args.resume_from_checkpoint)) else None
    model = (STMaskGIT.from_pretrained(load_from, precision=args.precision, action_vocab_size=warm_actions or None,
                                       action_dim=warm_dim or None) if load_from
             else STMaskGIT(cfg, precision=args.precision))
    conditioned = model.config.action_vocab_size or model.config.action_dim
    acts_of = (lambda get, idx: get(idx).to(dev)) if conditioned else (lambda get, idx: None)
    act_key = "action_vectors" if model.config.action_dim else "action_ids"   # the collator's and the model's keyword
    if model.config.action_vocab_size and not cfg.action_vocab_size:
        sys.exit("train.py: the checkpoint is action-conditioned: give a --genie_config with its action_vocab_size")
    if not load_from and args.mu_transfer:
        # reference train.py:420-424: init_weights() only on the muP path; otherwise PyTorch's default initialisation
        # of nn.Linear / nn.Embedding stays (kept here too, so from-scratch dynamics follow the reference recipe)
        model.init_weights()
    model = model.to(dev)
    if args.mlp_drop is not None:
        if not 0.0 <= args.mlp_drop < 1.0:
            sys.exit(f"train.py: --mlp_drop {args.mlp_drop} is not in [0, 1)")
        model.config.mlp_drop = args.mlp_drop   # read by the trainer; saved with the checkpoint's config
    if args.seed is not None:
        torch.manual_seed(args.seed + rank)  # collator draws differ per rank; the weights above do not

    B, accum = args.per_device_train_batch_size, args.gradient_accumulation_steps
    micro_per_epoch = n_train // (B * world)
    eb_ = args.per_device_eval_batch_size
    if micro_per_epoch < 1:
        sys.exit(f"train.py: {n_train} training windows < per_device_train_batch_size {B} x world {world}: no full batch")
    if n_eval < eb_ * world:
        sys.exit(f"train.py: {n_eval} eval windows < per_device_eval_batch_size {eb_} x world {world}: no full eval batch")
    updates_per_epoch = max(1, micro_per_epoch // accum)
    max_steps = args.max_train_steps or args.num_train_epochs * updates_per_epoch
    warm = args.num_warmup_steps
    lr_lambda = {"linear": trainmod.lr_factor_linear(warm, max_steps), "constant": lambda s: 1.0,
                 "custom_cosine": trainmod.lr_factor_custom_cosine(warm, max_steps)}[args.lr_scheduler_type]
    trainable = lr_scale = None
    try:   # the trainer's own rules: a pattern that matches nothing, an empty selection, a factor that is not a positive number
        names = [n for n, _ in model.named_parameters()]
        if args.train_only or args.freeze:
            trainable = sorted(trainmod.select_trainable(names, args.train_only, args.freeze))
        if args.lr_scale:
            pairs = [kv.rpartition("=") for kv in args.lr_scale.split(",") if kv]
            if any(not k or not v for k, _, v in pairs):
                raise ValueError(f"{args.lr_scale!r} is not a comma-separated list of PATTERN=FACTOR")
            lr_scale = {k: float(v) for k, _, v in pairs}
            trainmod.lr_factors(names, lr_scale)
    except ValueError as e:
        sys.exit(f"train.py: --train_only / --freeze / --lr_scale: {e}")
    teacher = None
    if args.teacher_path and args.distill_alpha > 0:   # never trained, saved or exchanged: every rank loads its own
        teacher = STMaskGIT.from_pretrained(args.teacher_path, precision=args.teacher_precision or args.precision).to(dev)
        try:
            trainmod.check_teacher(model.config, teacher.config)
        except ValueError as e:
            sys.exit(f"train.py: --teacher_path {args.teacher_path}: {e}")
    tr = trainmod.GenieTrainer(model, lr=args.learning_rate, betas=(args.adam_beta_1, args.adam_beta_2), eps=args.adam_eps,
                               weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm,
                               gradient_accumulation_steps=accum, lr_lambda=lr_lambda, recompute=args.recompute_activations,
                               dropout_seed=args.dropout_seed, ema_decay=args.ema_decay, ema_warmup=args.ema_warmup,
                               label_smoothing=args.label_smoothing, z_loss=args.z_loss, frame_weights=frame_weights,
                               trainable=trainable, lr_scale=lr_scale, teacher=teacher, distill_alpha=args.distill_alpha,
                               distill_temperature=args.distill_temperature, lora=lora, muon=muon)
    if args.resume_from_checkpoint and lora is not None:
        _, tensors = importlib.import_module("1xgpt_amd.lora").load_adapter_files(os.path.join(args.resume_from_checkpoint, "adapter"))
        tr.load_adapter_state_dict(tensors)
    if args.resume_from_checkpoint:  # optimizer moments, step counters (train.py:560-590), the EMA of the weights
        tr.load_state_dict(torch.load(os.path.join(args.resume_from_checkpoint, "trainer_state.pt"), map_location=dev))
    n_params = sum(p.numel() for p in model.parameters())
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
        if trainable is not None or lora is not None:
            print(f"training {len(tr.trainable)} of {len(tr.order)} tensors ({tr.n_train / 1e6:.2f} M of {tr.n_flat / 1e6:.1f} M flat "
                  f"elements); the backward stops at layer {tr.layout.stop}", flush=True)
        if muon is not None:
            print(f"muon on {len(tr.muon_names)} tensors ({len(tr.muon_items)} matrices, {tr.muon_launches()} launches per step), AdamW on the "
                  f"other {len(tr.trainable) - len(tr.muon_names)}", flush=True)
        print(f"params {n_params / 1e6:.1f} M, {n_train} train windows, batch {B} x {accum} x {world}, "
              f"{max_steps} update steps, precision {args.precision}", flush=True)

    def evaluate():
        """Teacher-forced loss / accuracy on collated eval batches (train.py:665-697)."""
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        eb = args.per_device_eval_batch_size
        for k, s0 in enumerate(range(rank * eb, n_eval - eb * world + 1, eb * world)):
            batch = datamod.maskgit_collate(get_eval(range(s0, s0 + eb)).to(dev), cfg,
                                            **{act_key: acts_of(get_eval_acts, range(s0, s0 + eb))})
            out = model(batch["input_ids"], batch["labels"], **{act_key: batch.get(act_key)})
            sums += torch.stack([out.loss.double() * eb, out.acc.double() * eb, torch.tensor(float(eb), device=dev).double()])
            if k + 1 >= args.max_eval_steps:
                break
        if world > 1:
            torch.distributed.all_reduce(sums)
        return (sums[0] / sums[2]).item(), (sums[1] / sums[2]).item()

    ckpt_every = int(args.checkpointing_steps) if args.checkpointing_steps.isdigit() else None
    completed, t0 = tr.completed_steps, time.time()
    # a training objective: the step also reports the plain CE; distillation: the KL and the teacher's own CE too
    extras = (["ce"] if tr._objective is not None or tr._distilling else []) + (["kd", "teacher_ce"] if tr._distilling else [])
    loss_info = torch.zeros(2 + len(extras), dtype=torch.float64, device=dev)   # sum loss, clips [, sum plain CE [, sum kd, sum teacher CE]]
    consumed = completed * accum  # micro-batches already trained on (resume): skip them in the data order
    for epoch in range(consumed // micro_per_epoch, 10 ** 9):
        g = torch.Generator().manual_seed((args.seed or 0) + epoch)
        perm = torch.randperm(n_train, generator=g)  # same permutation on every rank; rank r takes its slice
        for m in range(consumed % micro_per_epoch if epoch == consumed // micro_per_epoch else 0, micro_per_epoch):
            idx = perm[(m * world + rank) * B:(m * world + rank + 1) * B].tolist()
            batch = datamod.maskgit_collate(get_train(idx).to(dev), cfg, **{act_key: acts_of(get_train_acts, idx)},
                                            action_dropout=args.action_dropout if conditioned else 0.0,
                                            null_action=args.null_action)
            out = tr.train_step(batch)
            loss_info += torch.stack([out["loss"] * B, torch.tensor(float(B), device=dev, dtype=torch.float64)]
                                     + [out[k] * B for k in extras])
            if "lr" not in out:
                continue
            completed += 1
            if world > 1:
                torch.distributed.all_reduce(loss_info)
            avg = (loss_info[0] / loss_info[1]).item()
            ce = "".join(f" {k} {(loss_info[2 + i] / loss_info[1]).item():.4f}" for i, k in enumerate(extras))
            loss_info.zero_()
            if rank == 0:
                dt, t0 = time.time() - t0, time.time()
                print(f"step {completed}: train_loss {avg:.4f}{ce} ppl {math.exp(min(avg, 50)):.1f} lr {out['lr']:.3e} "
                      f"|g| {float(out['grad_norm']):.3f} {B * accum * world / dt:.1f} examples/s", flush=True)
            if completed % args.eval_every_n_steps == 0 or completed == max_steps:
                el, ea = evaluate()
                if rank == 0:
                    print(f"step {completed}: eval_loss {el:.4f} eval_teacher_acc {ea:.4f}", flush=True)
                if args.eval_ema:
                    with tr.ema_scope():
                        el, ea = evaluate()
                    if rank == 0:
                        print(f"step {completed}: ema_eval_loss {el:.4f} ema_eval_teacher_acc {ea:.4f}", flush=True)
            if rank == 0 and ((ckpt_every and completed % ckpt_every == 0) or completed == max_steps):
                ck = os.path.join(args.output_dir, "final_checkpt" if completed == max_steps else f"step_{completed}")
                model.save_pretrained(ck)
                torch.save(tr.state_dict(), os.path.join(ck, "trainer_state.pt"))
                if lora is not None:
                    tr.save_adapter(os.path.join(ck, "adapter"))
                if args.ema_decay is not None:   # the averaged weights as a checkpoint of their own (a swap local to this rank)
                    tr.save_ema_pretrained(os.path.join(ck, "ema"))
            if completed >= max_steps:
                dist_mod.barrier()
                return


if __name__ == "__main__":
    main()
