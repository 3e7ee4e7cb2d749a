#!/usr/bin/env python3
"""CLI counterpart of the reference's `python genie/generate.py` (generate.py:21-116): prompt frames -> generated frames,
written as [prompt | generated | ground truth] video.bin + metadata.json (readable by RawTokenDataset / visualize).

  python tools/generate.py --checkpoint_dir DIR --val_data_dir data/val_v1.1 --output_dir data/genie_generated
  python tools/generate.py --synthetic --model c35 --output_dir /tmp/gen
An action-conditioned checkpoint (action_vocab_size > 0) generates with the example's actions from the dataset's actions.bin
(refused without one); --guidance_scale W --null_action K decodes such a model under classifier-free guidance.
--num_new_frames N rolls out N frames behind the prompt, past the model's window if need be (the window slides by T - keep frames and
re-runs the last --keep frames as its context); the output is then [prompt | N generated | whatever ground truth exists].
--fanout K generates K candidate futures of the example over one shared context cache (in-window; branches differ by their sampling
draws and, for an action-conditioned model, by the (K, n_new) action ids of --fanout_actions); branch k is written to OUTPUT_DIR/branch_k.
--score generates nothing: it prints the negative log-likelihood of each observed frame behind the prompt (score_frames), one row per
action hypothesis of --fanout_actions (or the example's own actions).
--known_box top,left,height,width (token coordinates) inpaints: every generated frame keeps the ground-truth tokens of that box and the
model fills in the rest, consistent with them.  With --teacher_force_time this is the edit: the observed clip is the context and only
the tokens outside the box are regenerated; it also works with --num_new_frames (inside the example's frames) and --fanout."""
import argparse
import importlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--val_data_dir", type=str, default="data/val_v1.1")
    ap.add_argument("--checkpoint_dir", type=str)
    ap.add_argument("--adapter", type=str, default=None, metavar="DIR",
                    help="serve this adapter (a directory GenieTrainer.save_adapter / tools/train.py --lora_rank wrote) merged into the checkpoint's weights")
    ap.add_argument("--output_dir", type=str, default="data/genie_generated")
    ap.add_argument("--num_prompt_frames", type=int, default=8)
    ap.add_argument("--window_size", type=int, default=16)
    ap.add_argument("--example_ind", type=int, default=0)
    ap.add_argument("--teacher_force_time", action="store_true")
    ap.add_argument("--maskgit_steps", type=int, default=2)
    ap.add_argument("--temperature", type=float, default=0,
                    help="The reference's switch: 0 = arg-max, any value above 1e-8 = sample from the softmax. It does NOT temper "
                         "(0.7 and 1.0 draw from the same law); use --logit_temperature, --top_k, --top_p for that.")
    importlib.import_module("1xgpt_amd.sampling").add_cli_arguments(ap)
    importlib.import_module("1xgpt_amd.sampling").add_guidance_arguments(ap)
    ap.add_argument("--precision", choices=["exact", "f16x3", "bf16"], default="f16x3")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--model", choices=["c138", "c35"], default="c35")
    ap.add_argument("--schedule", choices=["kv_cache", "full_forward"], default="kv_cache",
                    help="kv_cache: one-frame passes against a temporal KV cache (same frames up to f32 accumulation order); "
                         "full_forward: the reference's schedule, a full 16-frame forward per MaskGIT step (generate.py:81-95)")
    ap.add_argument("--num_new_frames", type=int, default=None,
                    help="Roll out this many frames behind the prompt in one library call, past the model's window if need be "
                         "(default: fill the window, as the reference does).")
    ap.add_argument("--keep", type=int, default=None,
                    help="With --num_new_frames: frames of context each later window re-runs, 1 .. T-1 (default: --num_prompt_frames); "
                         "T-1 is the true sliding window, smaller is cheaper.")
    ap.add_argument("--fanout", type=int, default=None,
                    help="Generate this many candidate futures of the example in one library call (fanout_frames): the context runs once, "
                         "every branch keeps only its new frames' cache slots. In-window: fills the window, or --num_new_frames of it.")
    ap.add_argument("--fanout_actions", type=str, default=None,
                    help="With --fanout on an action-conditioned model: a text file of K rows of n_new action ids, one row per branch "
                         "(the prompt frames keep the example's actions).")
    ap.add_argument("--score", action="store_true",
                    help="Generate nothing: print the per-frame negative log-likelihood of the example's observed frames behind the prompt "
                         "(score_frames). On an action-conditioned model --fanout_actions scores K hypotheses (K rows of ids) and names the "
                         "likeliest; without it the example's own actions are scored.")
    ap.add_argument("--known_box", type=str, default=None, metavar="TOP,LEFT,HEIGHT,WIDTH",
                    help="Keep the ground-truth tokens of this box (token coordinates) in every generated frame and generate only the rest "
                         "(inpainting). Works with and without --teacher_force_time.")
    return ap


def known_box(args, model, ex, G, N):
    """--known_box: the (1, N, H, W) known tokens of the N frames behind the prompt, or None without the flag."""
    if args.known_box is None:
        return None
    try:
        top, left, height, width = (int(v) for v in args.known_box.split(","))
    except ValueError:
        sys.exit(f"generate.py: --known_box wants top,left,height,width, got {args.known_box!r}")
    if not (0 <= top and 0 <= left and height >= 1 and width >= 1 and top + height <= model.h and left + width <= model.w):
        sys.exit(f"generate.py: --known_box {args.known_box} does not lie inside the {model.h} x {model.w} token grid")
    P = args.num_prompt_frames
    if P + N > ex.shape[1]:
        sys.exit(f"generate.py: --known_box keeps ground-truth tokens, and the example has {ex.shape[1] - P} frames behind the prompt, not {N}")
    keep = torch.zeros(model.h, model.w, dtype=torch.bool, device=ex.device)
    keep[top:top + height, left:left + width] = True
    return G.known_tokens(ex[:, P:P + N], keep, model.mask_token_id)


def score_main(args, model, ex, actions, G):
    """--score: one line per hypothesis, the NLL of each observed frame in nats and their sum."""
    import numpy as np
    P = args.num_prompt_frames
    N = args.window_size - P if args.num_new_frames is None else args.num_new_frames
    kw = dict(K=1)
    if model.config.action_vocab_size:
        ids = actions[:, P:P + N].numpy()
        if args.fanout_actions is not None:
            ids = np.loadtxt(args.fanout_actions, dtype=np.int64, ndmin=2)
            if ids.shape[1] != N:
                sys.exit(f"generate.py: --fanout_actions holds {ids.shape} ids, expected (K, {N})")
        kw = dict(action_ids=torch.from_numpy(np.ascontiguousarray(ids))[None].to("cuda"), prompt_actions=actions[:, :P].to("cuda"))
    best, nll = G.infer_actions(model, ex[:, :P + N], P, **kw)
    for k, row in enumerate(nll[0].tolist()):
        print(f"hypothesis {k}: nll per frame [" + ", ".join(f"{v:.3f}" for v in row) + f"] sum {sum(row):.3f}")
    print(f"likeliest hypothesis: {int(best[0])}")


def fanout_main(args, model, ex, actions, meta, sampling, guidance, G):
    """--fanout K: [prompt | branch k's frames | ground truth] per branch, in OUTPUT_DIR/branch_k."""
    import numpy as np
    P, K = args.num_prompt_frames, args.fanout
    N = args.window_size - P if args.num_new_frames is None else args.num_new_frames
    if args.teacher_force_time or args.schedule != "kv_cache":
        sys.exit("generate.py: --fanout runs on the KV cache and has no teacher forcing in time")
    kw = {}
    if model.config.action_vocab_size:
        if args.fanout_actions is None:
            sys.exit("generate.py: --fanout on an action-conditioned model needs --fanout_actions (K rows of n_new ids)")
        ids = np.loadtxt(args.fanout_actions, dtype=np.int64, ndmin=2)
        if ids.shape != (K, N):
            sys.exit(f"generate.py: --fanout_actions holds {ids.shape} ids, expected ({K}, {N})")
        kw = dict(action_ids=torch.from_numpy(ids)[None].to("cuda"), prompt_actions=actions[:, :P].to("cuda"))
    out = G.fanout_frames(model, ex[:, :P], N, K=K, maskgit_steps=args.maskgit_steps, temperature=args.temperature,
                          unmask_mode=args.unmask_mode, sampling=sampling, guidance=guidance, known=known_box(args, model, ex, G, N), **kw)
    for k in range(K):
        frames = torch.cat([ex[:, :P], out[:, k], ex[:, P:]], dim=1)
        print(G.write_outputs(frames, os.path.join(args.output_dir, f"branch_{k}"), meta, vars(args)))


def main():
    args = build_parser().parse_args()
    sampling = importlib.import_module("1xgpt_amd.sampling").SamplingConfig.from_args(args)
    guidance = importlib.import_module("1xgpt_amd.sampling").Guidance.from_args(args)
    actions = None
    G = importlib.import_module("1xgpt_amd.generate")
    STMaskGIT = importlib.import_module("1xgpt_amd.st_mask_git").STMaskGIT
    if args.synthetic:
        cfgmod = importlib.import_module("1xgpt_amd.config")
        synth = importlib.import_module("1xgpt_amd.synthetic")
        cfg = cfgmod.c138() if args.model == "c138" else cfgmod.c35()
        model = STMaskGIT(cfg, precision=args.precision).load_numpy_state_dict(synth.make_state_dict(cfg, seed=0))
        example = torch.from_numpy(synth.make_clips(1, cfg, seed=1234 + args.example_ind))
        meta = {"s": model.h, "vocab_size": cfg.image_vocab_size, "hz": 2, "token_dtype": "uint32"}
    else:
        model = STMaskGIT.from_pretrained(args.checkpoint_dir, precision=args.precision)
        ds = importlib.import_module("1xgpt_amd.data").RawTokenDataset(args.val_data_dir, window_size=args.window_size,
                                                                      stride=G.STRIDE)
        item = ds[args.example_ind]
        example = item["input_ids"][None]
        meta = ds.metadata
        if model.config.action_vocab_size:
            if "action_ids" not in item:
                sys.exit(f"generate.py: the model is action-conditioned but {args.val_data_dir} has no actions.bin")
            actions = item["action_ids"][None]
    model = model.to("cuda")
    if args.adapter:
        try:
            model.load_adapter(args.adapter)
        except (ValueError, FileNotFoundError) as e:
            sys.exit(f"generate.py: --adapter {args.adapter}: {e}")
    ex = example.to("cuda").view(1, args.window_size, model.h, model.w)
    if args.score:
        if args.known_box is not None:
            sys.exit("generate.py: --score has no --known_box (scoring conditional on known tokens is not supported)")
        return score_main(args, model, ex, actions, G)
    if args.fanout is not None:
        return fanout_main(args, model, ex, actions, meta, sampling, guidance, G)
    if args.num_new_frames is not None:
        P, N = args.num_prompt_frames, args.num_new_frames
        if args.teacher_force_time or args.schedule != "kv_cache":
            sys.exit("generate.py: --num_new_frames runs on the KV cache and has no teacher forcing in time")
        if actions is not None and actions.shape[1] < P + N:
            sys.exit(f"generate.py: {P} + {N} frames need as many actions, the example has {actions.shape[1]}: raise --window_size")
        out = G.rollout_frames(model, ex[:, :P], N, keep=args.keep, maskgit_steps=args.maskgit_steps, temperature=args.temperature,
                               unmask_mode=args.unmask_mode, action_ids=None if actions is None else actions[:, :P + N].to("cuda"),
                               sampling=sampling, guidance=guidance, known=known_box(args, model, ex, G, N))
        print(G.write_outputs(torch.cat([out, ex[:, P:]], dim=1), args.output_dir, meta, vars(args)))
        return
    fn = G.generate_frames_cached if args.schedule == "kv_cache" else G.generate_frames
    out = fn(model, ex, args.num_prompt_frames, args.maskgit_steps, args.temperature, args.teacher_force_time,
             action_ids=None if actions is None else actions.to("cuda"), sampling=sampling, unmask_mode=args.unmask_mode,
             guidance=guidance, known=known_box(args, model, ex, G, args.window_size - args.num_prompt_frames))
    print(G.write_outputs(out, args.output_dir, meta, vars(args)))


if __name__ == "__main__":
    main()
