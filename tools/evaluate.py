#!/usr/bin/env python3
"""CLI counterpart of the reference's `python genie/evaluate.py` (evaluate.py:35-66, 145-204) on the MI355X path.

  python tools/evaluate.py --checkpoint_dir DIR --val_data_dir data/val_v1.1 [--maskgit_steps 2] [--batch_size 16]
  python tools/evaluate.py --synthetic 32 --model c138            # no checkpoint / dataset offline: synthetic weights + clips
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/evaluate.py ...   # data-parallel

  python tools/evaluate.py --synthetic 32 --model c35 --image_metrics   # + PSNR / SSIM / MSE of the decoded frames, per horizon

Prints the running means like the reference ({gen_time, loss, acc}); LPIPS is out of scope (needs the `lpips` AlexNet): --image_metrics
decodes the predicted and the ground-truth frames with the MAGVIT2 tokenizer (--tokenizer_ckpt; synthetic weights with --synthetic) and
adds PSNR, SSIM and MSE, as whole-job means and against the prediction horizon.
An action-conditioned checkpoint (action_vocab_size > 0) is evaluated with the dataset's actions.bin (refused without one)."""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description="Evaluate GENIE-style models (MI355X path).")
    ap.add_argument("--val_data_dir", type=str, default="data/val_v1.1")
    ap.add_argument("--checkpoint_dir", type=str)
    ap.add_argument("--adapter", type=str, default=None, metavar="DIR",
                    help="serve this adapter (a directory GenieTrainer.save_adapter / tools/train.py --lora_rank wrote) merged into the checkpoint's weights")
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--maskgit_steps", type=int, default=2)
    ap.add_argument("--temperature", type=float, default=0,
                    help="The reference's switch: 0 = arg-max, any value above 1e-8 = sample from the softmax. It does NOT temper "
                         "(0.7 and 1.0 draw from the same law); use --logit_temperature, --top_k, --top_p for that.")
    importlib.import_module("1xgpt_amd.sampling").add_cli_arguments(ap)
    ap.add_argument("--max_examples", type=int)
    ap.add_argument("--precision", choices=["exact", "f16x3", "bf16"], default="f16x3")
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate N synthetic clips with synthetic weights")
    ap.add_argument("--model", choices=["c138", "c35"], default="c35", help="shape for --synthetic")
    ap.add_argument("--no_reuse", action="store_true", help="reference schedule (15 x steps full forwards)")
    ap.add_argument("--image_metrics", action="store_true",
                    help="decode predicted and ground-truth frames and report PSNR / SSIM / MSE (means and per prediction horizon)")
    ap.add_argument("--tokenizer_ckpt", type=str, default="data/magvit2.ckpt", help="MAGVIT2 checkpoint for --image_metrics")
    return ap


def main():
    args = build_parser().parse_args()
    importlib.import_module("1xgpt_amd.sampling").SamplingConfig.from_args(args)   # (argument errors before the model loads)

    ev_mod = importlib.import_module("1xgpt_amd.evaluate")
    dist_mod = importlib.import_module("1xgpt_amd.distributed")
    cfgmod = importlib.import_module("1xgpt_amd.config")
    synth = importlib.import_module("1xgpt_amd.synthetic")
    STMaskGIT = importlib.import_module("1xgpt_amd.st_mask_git").STMaskGIT
    rank, world, local_rank = dist_mod.init_distributed()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    actions = None
    if args.synthetic:
        cfg = cfgmod.c138() if args.model == "c138" else cfgmod.c35()
        model = STMaskGIT(cfg, precision=args.precision).load_numpy_state_dict(synth.make_state_dict(cfg, seed=0))
        clips = torch.from_numpy(synth.make_clips(args.synthetic, cfg, seed=1234))
        side = model.h
    else:
        model = STMaskGIT.from_pretrained(args.checkpoint_dir, precision=args.precision)
        ds = importlib.import_module("1xgpt_amd.data").RawTokenDataset(
            args.val_data_dir, window_size=ev_mod.WINDOW_SIZE, stride=ev_mod.STRIDE, filter_overlaps=True)
        n = len(ds) if args.max_examples is None else min(len(ds), args.max_examples)
        clips = ds.batch(range(n))
        side = ds.metadata["s"]
        if model.config.action_vocab_size:
            if ds.actions is None:
                sys.exit(f"evaluate.py: the model is action-conditioned but {args.val_data_dir} has no actions.bin")
            actions = ds.action_batch(range(n))
    args.latent_h = args.latent_w = side
    lo, hi = dist_mod.shard_range(clips.shape[0], rank, world)
    decode_latents = None
    if args.image_metrics:
        mv = importlib.import_module("1xgpt_amd.magvit2")
        vq = None
        if args.synthetic:
            vq = mv.VQModel(mv.VQConfig())
            vq.load_state_dict({k: torch.from_numpy(v) for k, v in mv.make_vq_state_dict(vq, seed=1).items()})
        elif not os.path.exists(args.tokenizer_ckpt):
            sys.exit(f"evaluate.py: --image_metrics needs the tokenizer, and {args.tokenizer_ckpt} does not exist (--tokenizer_ckpt)")
        decode_latents = mv.decode_latents_wrapper(batch_size=64, tokenizer_ckpt=args.tokenizer_ckpt, model=vq, device=dev)
    ev = ev_mod.GenieEvaluator(args, decode_latents, dev, model=model)
    if args.adapter:
        try:
            ev.model.load_adapter(args.adapter)
        except (ValueError, FileNotFoundError) as e:
            sys.exit(f"evaluate.py: --adapter {args.adapter}: {e}")
        print(f"adapter {args.adapter} merged", flush=True)
    res = ev_mod.evaluate_clips(ev, clips[lo:hi], batch_size=args.batch_size, distributed=world > 1,
                                reuse=not args.no_reuse, action_ids=None if actions is None else actions[lo:hi],
                                **(dict(image_metrics=True) if args.image_metrics else {}))
    if rank == 0:
        res["gen_time_s_per_frame"] = res["seconds"] / max(res["frames"], 1)
        print(json.dumps(res))
        if args.image_metrics:
            print(f"loss {res['loss']:.4f}  acc {res['acc']:.4f}  PSNR {res['psnr']:.3f} dB  SSIM {res['ssim']:.4f}  MSE {res['mse']:.2f}")
            print("PSNR by horizon (dB): " + " ".join(f"{v:.2f}" for v in res["psnr_per_frame"]))


if __name__ == "__main__":
    main()
