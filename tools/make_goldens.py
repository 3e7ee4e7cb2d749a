#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (imported read-only from /root/reference).

Build-container only: /root/reference does not exist on the GPU box, so the outputs (small arrays) are
committed and this script documents exactly how they were made.  Nothing from the reference's source
is copied; only inputs and the outputs it computed are stored.

The reference imports five packages that are not in this image.  None of them contributes arithmetic
to the fixtures, except where stated:
  * ``xformers.ops``  -- imported unconditionally (genie/attention.py:3).  With XFORMERS_DISABLED=true the
    executed attention is the pure-torch BasicSelfAttention (attention.py:36-61), which the reference's
    own test_attention.py:18 pins equal to the xformers path.  The placeholder's attention entry raises.
  * ``mup``           -- subclassed at st_mask_git.py:316.  For use_mup=False it is never instantiated.
    For use_mup=True the placeholder supplies ``width_mult() = d_model/256`` and ``output_mult = 1``,
    i.e. mup's documented readout formula -> those fixtures are marked ``mup_pinned = 0`` (parity
    unpinned for the muP readout; everything else in them is the reference's own arithmetic).
Placeholders live only in this process's ``sys.modules``.

Weights/clips come from 1xgpt_amd.synthetic (NumPy PCG64), so the GPU box rebuilds them bit-identically
and fixtures only need to hold outputs.
"""
import importlib
import math
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

os.environ["XFORMERS_DISABLED"] = "true"
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")


def _install_placeholders():
    def mod(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m
        return m

    def _no_xformers(*a, **k):
        raise RuntimeError("xformers is not available; XFORMERS_DISABLED=true path expected")

    ops = mod("xformers.ops", LowerTriangularMask=object, memory_efficient_attention=_no_xformers,
              unbind=torch.unbind)
    mod("xformers", ops=ops)

    class MuReadout(nn.Linear):  # mup.MuReadout's readout formula only
        output_mult = 1.0

        def width_mult(self):
            return self.in_features / 256  # base shape d_model=256 (st_mask_git.py:298-304)

    mod("mup", MuReadout=MuReadout, normal_=None, set_base_shapes=None, MuAdamW=None)
    tvf = mod("torchvision.transforms.functional", pil_to_tensor=None)
    tvf2 = mod("torchvision.transforms.v2.functional", to_pil_image=None)
    tv2 = mod("torchvision.transforms.v2", functional=tvf2)
    tvt = mod("torchvision.transforms", functional=tvf, v2=tv2)
    mod("torchvision", transforms=tvt, models=None)
    mod("lpips", LPIPS=None)
    mod("lightning", LightningModule=nn.Module)


import transformers  # noqa: E402,F401  (real package; imported before the placeholders so its own probes see the truth)
from transformers.utils import ModelOutput  # noqa: E402,F401

_install_placeholders()
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
pkg = importlib.import_module("1xgpt_amd")
synthetic = importlib.import_module("1xgpt_amd.synthetic")
MyConfig = importlib.import_module("1xgpt_amd.config").GenieConfig

from genie.config import GenieConfig as RefConfig  # noqa: E402
from genie.st_mask_git import STMaskGIT  # noqa: E402
import genie.evaluate as ref_evaluate  # noqa: E402
import eval_utils as ref_eval_utils  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(8)


def build_ref_model(cfg_kwargs, seed):
    rcfg = RefConfig(**cfg_kwargs)
    mcfg = MyConfig(**cfg_kwargs)
    model = STMaskGIT(rcfg)
    sd = synthetic.make_state_dict(mcfg, seed=seed, law="conditioned")
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    model.eval()
    return model, mcfg


class Recorder:
    """Captures torch.rand_like draws and the top-2 logit gap of frame out_t at every forward."""

    def __init__(self, model):
        self.model = model
        self.noise = []
        self.min_gap = float("inf")
        self.min_conf_relgap = float("inf")
        self.out_t = None
        self._orig_rand_like = torch.rand_like
        self._orig_logits = model.compute_logits

    def __enter__(self):
        def rand_like(x, *a, **k):
            r = self._orig_rand_like(x, *a, **k)
            self.noise.append(r.reshape(r.shape[0], -1).numpy().copy())
            return r

        def compute_logits(x):
            lg = self._orig_logits(x)
            if self.out_t is not None:
                f = lg[:, :, self.out_t]  # (B, nv * vf, H, W), channel = factor * vf + k
                B = f.shape[0]
                c = self.model.config
                ff = f.reshape(B, c.num_factored_vocabs, c.factored_vocab_size, -1)
                top2 = ff.topk(2, dim=2).values
                self.min_gap = min(self.min_gap, float((top2[:, :, 0] - top2[:, :, 1]).min()))
                conf = ff.softmax(2).amax(2).prod(1)  # (B, S) confidence of the argmax sample
                srt = conf.double().sort(-1).values
                self.min_conf_relgap = min(self.min_conf_relgap, float(((srt[:, 1:] - srt[:, :-1]) / srt[:, 1:]).min()))
            return lg

        torch.rand_like = rand_like
        self.model.compute_logits = compute_logits
        return self

    def __exit__(self, *exc):
        torch.rand_like = self._orig_rand_like
        self.model.compute_logits = self._orig_logits


def run_maskgit(model, prompt, out_t, steps, mode, temperature=0.0):
    with Recorder(model) as rec:
        rec.out_t = out_t
        p = prompt.clone()
        s, fl = model.maskgit_generate(p, out_t, maskgit_steps=steps, temperature=temperature, unmask_mode=mode)
    noise = np.stack(rec.noise) if rec.noise else np.zeros((0, prompt.shape[0], prompt.shape[2] * prompt.shape[3]),
                                                            np.float32)
    if mode == "greedy" and rec.min_conf_relgap < 1e-4:  # confidence order numerically fragile
        return s.numpy(), fl.numpy(), p.numpy(), noise, 0.0
    if mode == "random" and noise.size and conf_gap(noise) <= 0.0:  # exact tie in the injected keys
        return s.numpy(), fl.numpy(), p.numpy(), noise, 0.0
    return s.numpy(), fl.numpy(), p.numpy(), noise, rec.min_gap


def conf_gap(noise):
    """Smallest distance between two sort keys of one clip (ties would make argsort order undefined)."""
    if noise.size == 0:
        return float("inf")
    srt = np.sort(noise.astype(np.float64), axis=-1)
    return float(np.diff(srt, axis=-1).min())


def tiny_fixture(name, cfg_kwargs, wseed):
    model, cfg = build_ref_model(cfg_kwargs, wseed)
    H = W = math.isqrt(cfg.S)
    B = 2
    for clip_seed in range(100, 140):
        ids = synthetic.make_clips(B, cfg, seed=clip_seed)
        x = torch.from_numpy(ids).reshape(B, cfg.T, H, W)
        out = {"clip_seed": clip_seed, "weight_seed": wseed, "ids": ids}
        gaps = []
        out["logits"] = model.compute_logits(x).numpy()
        # masked forward: frames >= 2 fully masked plus scattered masks in frame 1
        xm = x.clone()
        xm[:, 2:] = model.mask_token_id
        g = np.random.default_rng(clip_seed + 7)
        scatter = torch.from_numpy(g.random((B, H, W)) < 0.3)
        xm[:, 1][scatter] = model.mask_token_id
        fo = model(xm.reshape(B, -1), torch.from_numpy(ids))
        out["fwd_input"] = xm.reshape(B, -1).numpy()
        out["fwd_loss"] = np.float64(fo.loss.item())
        out["fwd_acc"] = np.float64(fo.acc.item())
        out["fwd_logits_sum"] = np.float64(fo.logits.double().sum().item())
        # unmasked forward -> nan loss (0/0), reference has no guard
        fo2 = model(x.reshape(B, -1), torch.from_numpy(ids))
        out["fwd_nomask_loss_isnan"] = np.bool_(math.isnan(fo2.loss.item()))
        # maskgit
        prompt = x.clone()
        prompt[:, 2:] = model.mask_token_id
        for steps in (1, 2, 3, 8):
            for mode in ("random", "greedy"):
                torch.manual_seed(1000 + steps)
                s, fl, p_after, noise, gap = run_maskgit(model, prompt, 2, steps, mode)
                k = f"mg_s{steps}_{mode}"
                out[k + "_samples"] = s
                out[k + "_prompt_after"] = p_after
                out[k + "_noise"] = noise
                if steps == 2 and mode == "random":
                    out["mg_step0_factored_logits"] = fl
                gaps.append(gap)
        # generate(): 2 prompt frames -> 2 new frames
        with Recorder(model) as rec:
            torch.manual_seed(77)
            rec.out_t = None
            gen, gl = model.generate(torch.from_numpy(ids[:, :2 * cfg.S]), None, max_new_tokens=2 * cfg.S,
                                     return_logits=True, maskgit_steps=2, temperature=0.0)
        out["gen_out"] = gen.numpy()
        if name == "tiny_ln":
            out["gen_logits"] = gl.numpy()
        out["gen_noise"] = np.stack(rec.noise).reshape(2, 1, B, cfg.S)
        # evaluator harness (genie/evaluate.py:82-122) with its window constant set to this T
        ref_evaluate.WINDOW_SIZE = cfg.T
        ev = object.__new__(ref_evaluate.GenieEvaluator)
        ev.model, ev.device, ev.decode_latents = model, "cpu", None
        ev.args = SimpleNamespace(maskgit_steps=2, temperature=0, latent_h=H, latent_w=W)
        with Recorder(model) as rec:
            torch.manual_seed(99)
            samples, fl = ev.predict_zframe_logits(torch.from_numpy(ids))
        out["ev_samples"] = samples.numpy()
        out["ev_logits"] = fl.numpy()
        out["ev_noise"] = np.stack(rec.noise).reshape(cfg.T - 1, 1, B, cfg.S)
        out["ev_loss"] = np.float64(ref_eval_utils.compute_loss(torch.from_numpy(ids), fl))
        out["ev_acc"] = np.float64((x[:, 1:] == samples).float().mean().item())
        # gap of the harness-level forwards (generate / evaluate): recompute conservatively over all frames >= 1
        lg = torch.from_numpy(out["ev_logits"])  # step-0 only; later steps covered by mg_* gaps above
        t2 = lg.permute(0, 2, 3, 4, 5, 1).topk(2, dim=-1).values
        gaps.append(float((t2[..., 0] - t2[..., 1]).min()))
        min_gap = min(gaps)
        if min_gap > 2e-4:
            break
    out["min_gap"] = np.float64(min_gap)
    out["mup_pinned"] = np.int64(0 if cfg.use_mup else 1)
    out["cfg"] = np.array(repr(cfg_kwargs))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: clip_seed={clip_seed} min_gap={min_gap:.3e} ev_loss={out['ev_loss']:.6f} "
          f"fwd_loss={out['fwd_loss']:.6f}")


def vocab_fixture(name, cfg_kwargs, wseed, n_probe=None):
    """tiny_fixture's contents for a vocabulary other than 2 x 512 (image_vocab_size = vf ** nv, V = nv * vf logits per token).
    The reference's compute_loss_and_acc factorises its targets with factorize_labels' DEFAULTS (st_mask_git.py:241: 2 x 512),
    which raises for any other vocabulary; for the forward loss / acc it is called here with the model's own factorisation,
    the operation the surrounding code (rearrange with the config's vocab_size / num_vocabs, :236-239) means.  Everything else
    (FactorizedEmbedding, readout, maskgit_generate's per-factor sampling, generate) reads the config already.
    n_probe: keep that many (t, s) probe columns of the logits instead of all of them (file size)."""
    import genie.st_mask_git as ref_smg
    from genie.factorization_utils import factorize_labels as ref_factorize_labels
    model, cfg = build_ref_model(cfg_kwargs, wseed)
    nv, vf = cfg.num_factored_vocabs, cfg.factored_vocab_size
    H = W = math.isqrt(cfg.S)
    B = 2
    orig_fl = ref_smg.factorize_labels
    ref_smg.factorize_labels = lambda t: ref_factorize_labels(t, nv, vf)
    try:
        for clip_seed in range(100, 140):
            ids = synthetic.make_clips(B, cfg, seed=clip_seed)
            x = torch.from_numpy(ids).reshape(B, cfg.T, H, W)
            out = {"clip_seed": clip_seed, "weight_seed": wseed, "ids": ids}
            gaps = []
            lg = model.compute_logits(x)  # (B, V, T, H, W)
            if n_probe is None:
                out["logits"] = lg.numpy()
            else:
                g = np.random.default_rng(5)
                pt, ps = g.integers(0, cfg.T, n_probe), g.integers(0, cfg.S, n_probe)
                out["probe_t"], out["probe_s"] = pt, ps
                out["probe_logits"] = np.stack([lg[:, :, t, s // W, s % W].numpy() for t, s in zip(pt, ps)], 1)  # (B, n, V)
            out["logits_sum"] = np.float64(lg.double().sum().item())
            # masked forward: frames >= 2 fully masked plus scattered masks in frame 1
            xm = x.clone()
            xm[:, 2:] = model.mask_token_id
            g = np.random.default_rng(clip_seed + 7)
            scatter = torch.from_numpy(g.random((B, H, W)) < 0.3)
            xm[:, 1][scatter] = model.mask_token_id
            fo = model(xm.reshape(B, -1), torch.from_numpy(ids))
            out["fwd_input"] = xm.reshape(B, -1).numpy()
            out["fwd_loss"] = np.float64(fo.loss.item())
            out["fwd_acc"] = np.float64(fo.acc.item())
            out["fwd_logits_sum"] = np.float64(fo.logits.double().sum().item())
            # maskgit on frame 2 with the captured draws
            prompt = x.clone()
            prompt[:, 2:] = model.mask_token_id
            for steps in (1, 2, 3, 8):
                for mode in ("random", "greedy"):
                    torch.manual_seed(1000 + steps)
                    s, fl, p_after, noise, gap = run_maskgit(model, prompt, 2, steps, mode)
                    k = f"mg_s{steps}_{mode}"
                    out[k + "_samples"] = s
                    out[k + "_prompt_after"] = p_after
                    out[k + "_noise"] = noise
                    if steps == 2 and mode == "random":
                        out["mg_step0_factored_logits"] = fl if n_probe is None else fl[:, :, :, :1, :]
                    gaps.append(gap)
            # generate(): 2 prompt frames -> 2 new frames
            orig_mg = model.maskgit_generate
            with Recorder(model) as rec:
                def mg(prompt, out_t, **kw):  # gap-track the frame each of generate()'s decodes samples
                    rec.out_t = out_t
                    return orig_mg(prompt, out_t, **kw)

                model.maskgit_generate = mg
                torch.manual_seed(77)
                try:
                    gen = model.generate(torch.from_numpy(ids[:, :2 * cfg.S]), None, max_new_tokens=2 * cfg.S,
                                         maskgit_steps=2, temperature=0.0)
                finally:
                    model.maskgit_generate = orig_mg
            out["gen_out"] = gen.numpy()
            out["gen_noise"] = np.stack(rec.noise).reshape(2, 1, B, cfg.S)
            gaps.append(rec.min_gap if conf_gap(out["gen_noise"]) > 0 else 0.0)
            min_gap = min(gaps)
            if min_gap > 2e-4:
                break
    finally:
        ref_smg.factorize_labels = orig_fl
    out["min_gap"] = np.float64(min_gap)
    out["mup_pinned"] = np.int64(0 if cfg.use_mup else 1)
    out["cfg"] = np.array(repr(cfg_kwargs))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: clip_seed={clip_seed} min_gap={min_gap:.3e} fwd_loss={out['fwd_loss']:.6f} "
          f"fwd_acc={out['fwd_acc']:.6f} bytes={os.path.getsize(os.path.join(OUT, name + '.npz'))}")


def shape_fixture(name, cfg_kwargs, wseed, gap_thr, do_eval=True, B=1, steps_list=(2,), n_probe=64):
    """Real token geometry (T=16, S=256).  Logits are too big to commit whole: keep a probe subset."""
    model, cfg = build_ref_model(cfg_kwargs, wseed)
    H = W = math.isqrt(cfg.S)
    for clip_seed in range(200, 240):
        ids = synthetic.make_clips(B, cfg, seed=clip_seed)
        x = torch.from_numpy(ids).reshape(B, cfg.T, H, W)
        out = {"clip_seed": clip_seed, "weight_seed": wseed, "ids": ids}
        gaps = []
        # forward + CE with frames >= 8 masked (BASELINE config 2)
        xm = x.clone()
        xm[:, 8:] = model.mask_token_id
        fo = model(xm.reshape(B, -1), torch.from_numpy(ids))
        out["fwd_loss"] = np.float64(fo.loss.item())
        out["fwd_acc"] = np.float64(fo.acc.item())
        lg = fo.logits  # (B,1024,T,H,W)
        g = np.random.default_rng(5)
        probe_t = g.integers(0, cfg.T, n_probe)
        probe_s = g.integers(0, cfg.S, n_probe)
        out["probe_t"], out["probe_s"] = probe_t, probe_s
        out["probe_logits"] = np.stack([lg[:, :, t, s // W, s % W].numpy() for t, s in zip(probe_t, probe_s)], 1)
        # CE per frame of the masked forward, from the reference's own loss helper on frame slices
        fl_all = lg[:, :, 1:].reshape(B, 2, 512, cfg.T - 1, H, W).permute(0, 2, 1, 3, 4, 5)
        out["fwd_compute_loss_allframes"] = np.float64(ref_eval_utils.compute_loss(torch.from_numpy(ids), fl_all))
        # maskgit on frame 8 (generate.py's first step)
        for steps in steps_list:
            torch.manual_seed(4242 + steps)
            s, fl, p_after, noise, gap = run_maskgit(model, xm, 8, steps, "random")
            out[f"mg_s{steps}_samples"] = s
            out[f"mg_s{steps}_noise"] = noise
            gaps.append(gap)
        if do_eval:
            ref_evaluate.WINDOW_SIZE = cfg.T
            ev = object.__new__(ref_evaluate.GenieEvaluator)
            ev.model, ev.device, ev.decode_latents = model, "cpu", None
            ev.args = SimpleNamespace(maskgit_steps=2, temperature=0, latent_h=H, latent_w=W)
            with Recorder(model) as rec:
                torch.manual_seed(4321)
                # gap must be tracked per timestep: hook maskgit_generate to set out_t
                orig_mg = model.maskgit_generate

                def mg(prompt, out_t, **kw):
                    rec.out_t = out_t
                    return orig_mg(prompt, out_t, **kw)

                model.maskgit_generate = mg
                samples, fl = ev.predict_zframe_logits(torch.from_numpy(ids))
                model.maskgit_generate = orig_mg
            out["ev_samples"] = samples.numpy().astype(np.int32)
            out["ev_noise"] = np.stack(rec.noise).reshape(cfg.T - 1, 1, B, cfg.S)
            out["ev_loss"] = np.float64(ref_eval_utils.compute_loss(torch.from_numpy(ids), fl))
            out["ev_acc"] = np.float64((x[:, 1:] == samples).float().mean().item())
            gaps.append(rec.min_gap)
            gaps.append(1.0 if conf_gap(out["ev_noise"]) > 0 else 0.0)
        min_gap = min(gaps)
        print(f"  {name}: try clip_seed={clip_seed} min_gap={min_gap:.3e}")
        if min_gap > gap_thr:
            break
    out["min_gap"] = np.float64(min_gap)
    out["mup_pinned"] = np.int64(0 if cfg.use_mup else 1)
    out["cfg"] = np.array(repr(cfg_kwargs))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: clip_seed={clip_seed} min_gap={min_gap:.3e} fwd_loss={out['fwd_loss']:.6f} "
          f"ev_loss={out.get('ev_loss', float('nan')):.6f}")


def harness_fixture():
    """generate.py semantics (prompt 2 -> 2 frames, [prompt | generated | gt]) and the RawTokenDataset filters,
    produced by the reference's own data.py and the body of generate.py:77-103 driven on the tiny model."""
    import tempfile
    import data as ref_data
    cfg_kwargs = dict(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2, qk_norm=False,
                      use_mup=False)
    model, cfg = build_ref_model(cfg_kwargs, 11)
    g = np.random.default_rng(321)
    n_img, side = 60, 4
    tokens = g.integers(0, 262144, size=(n_img, side, side)).astype(np.uint32)
    seg = np.sort(g.integers(0, 4, size=n_img)).astype(np.int32)
    out = {"tokens": tokens, "segment_ids": seg, "cfg": np.array(repr(cfg_kwargs)), "weight_seed": 11}
    with tempfile.TemporaryDirectory() as d:
        tokens.tofile(os.path.join(d, "video.bin"))
        seg.tofile(os.path.join(d, "segment_ids.bin"))
        with open(os.path.join(d, "metadata.json"), "w") as f:
            import json
            json.dump({"num_images": n_img, "s": side, "vocab_size": 262144, "hz": 30, "token_dtype": "uint32"}, f)
        for name, kw in [("w4s3", dict(window_size=4, stride=3)),
                         ("w4s3_overlap", dict(window_size=4, stride=3, filter_overlaps=True)),
                         ("w4s1_nointerrupt", dict(window_size=4, stride=1, filter_interrupts=False)),
                         ("w4s2_overlap", dict(window_size=4, stride=2, filter_overlaps=True))]:
            ds = ref_data.RawTokenDataset(d, **kw)
            out["ds_" + name + "_starts"] = np.array(ds.valid_start_inds, dtype=np.int64)
            out["ds_" + name + "_item0"] = ds[0]["input_ids"].numpy()
            out["ds_" + name + "_item_last"] = ds[len(ds) - 1]["input_ids"].numpy()
        ds = ref_data.RawTokenDataset(d, window_size=4, stride=3)
        # generate.py:70-103 on example 1 (window 4, 2 prompt frames, 2 maskgit steps, temperature 0)
        example = ds[1]["input_ids"].reshape(1, 4, side, side)
        for tf in (False, True):
            with Recorder(model) as rec:
                torch.manual_seed(5)
                samples = []
                prompt = example.clone()
                prompt[:, 2:] = model.mask_token_id
                for t in range(2, 4):
                    if tf:
                        prompt = example.clone()
                        prompt[:, t:] = model.mask_token_id  # what generate.py:86 means (image_mask_token is a bug)
                    s_hw, _ = model.maskgit_generate(prompt, out_t=t, maskgit_steps=2, temperature=0)
                    samples.append(s_hw)
                    if not tf:
                        prompt[:, t] = s_hw
                outs = torch.cat([example[:, :2], torch.stack(samples, 1), example[:, 2:]], 1)
            key = "gen_tf" if tf else "gen_ar"
            out[key + "_outputs"] = outs.numpy()
            out[key + "_noise"] = np.stack(rec.noise).reshape(2, 1, 1, side * side)
        out["gen_example"] = example.numpy()
    np.savez_compressed(os.path.join(OUT, "harness.npz"), **out)
    print("harness: dataset windows", {k: v.shape for k, v in out.items() if k.endswith("_starts")})


def magvit_fixture():
    """MAGVIT2 inference pieces from the reference: LFQ bit order, ResBlock/Upsampler/Decoder/Encoder I/O on a small
    VQConfig, and rescale_magvit_output on bf16 (visualize.py)."""
    from magvit2.config import VQConfig as RefVQ
    from magvit2.modules.diffusionmodules.improved_model import Encoder as RefEnc, Decoder as RefDec
    from magvit2.modules.vqvae.lookup_free_quantize import LFQ
    mv = importlib.import_module("1xgpt_amd.magvit2")
    small = dict(base_channels=32, ch_mult=(1, 2), num_res_blocks=1)
    rcfg = RefVQ(**small)
    mine = mv.VQModel(mv.VQConfig(**small))
    sd = mv.make_vq_state_dict(mine, seed=1)
    enc, dec = RefEnc(rcfg), RefDec(rcfg)
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("encoder.")})
    dec.load_state_dict({k[len("decoder."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("decoder.")})
    enc.eval(), dec.eval()
    g = np.random.default_rng(9)
    out = {"cfg": np.array(repr(small)), "weight_seed": 1}
    # a18: token -> bits (LFQ on the full 2^18 codebook config)
    lfq = LFQ(RefVQ())
    ids = g.integers(0, 262144, size=(3, 16)).astype(np.int64)
    ids[0, :4] = [0, 1, 2, 262143]
    quant = lfq.get_codebook_entry(torch.from_numpy(ids), bhwc=(3, 4, 4, 18)).flip(1)
    out["bits_ids"], out["bits_z"] = ids.reshape(3, 4, 4), quant.numpy().astype(np.float32)
    # decoder: tokens -> frames, f32 and bf16 (the reference decodes in bf16, visualize.py:97-101)
    tok = g.integers(0, 262144, size=(2, 4, 4)).astype(np.int64)
    z = lfq.get_codebook_entry(torch.from_numpy(tok.reshape(2, 16)), bhwc=(2, 4, 4, 18)).flip(1).float()
    y32 = dec(z)
    out["dec_tokens"], out["dec_out_f32"] = tok, y32.numpy()
    import visualize as ref_vis
    out["dec_u8_f32"] = ref_vis.rescale_magvit_output(y32).numpy()
    dec16 = RefDec(rcfg)
    dec16.load_state_dict(dec.state_dict())
    dec16 = dec16.to(torch.bfloat16).eval()
    y16 = dec16(z.to(torch.bfloat16))
    out["dec_out_bf16_as_f32"] = y16.float().numpy()
    out["dec_u8_bf16"] = ref_vis.rescale_magvit_output(y16).numpy()
    # rescale alone on arbitrary bf16 values (bit-exact target)
    r = (torch.from_numpy(g.standard_normal(4096).astype(np.float32)) * 1.3).to(torch.bfloat16)
    out["rescale_in_bf16_as_f32"] = r.float().numpy()
    out["rescale_out"] = ref_vis.rescale_magvit_output(r).numpy()
    # encoder: frames -> code (pre-quantisation) -> sign bits
    frames = g.integers(0, 256, size=(2, 3, 8, 8)).astype(np.uint8)
    xin = torch.from_numpy(frames).float() / 127.5 - 1.0
    hcode = enc(xin)
    out["enc_frames"], out["enc_h"] = frames, hcode.numpy()
    out["enc_min_abs_h"] = np.float64(hcode.abs().min().item())
    np.savez_compressed(os.path.join(OUT, "magvit_small.npz"), **out)
    # mid-size decoder (ResBlock widths 256/128: the geometry class of the shipped config) for the hand-written conv path
    mid = dict(base_channels=128, ch_mult=(1, 2), num_res_blocks=1)
    rcfg2 = RefVQ(**mid)
    mine2 = mv.VQModel(mv.VQConfig(**mid))
    sd2 = mv.make_vq_state_dict(mine2, seed=2)
    dec2 = RefDec(rcfg2)
    dec2.load_state_dict({k[len("decoder."):]: torch.from_numpy(v) for k, v in sd2.items() if k.startswith("decoder.")})
    dec2.eval()
    tok2 = g.integers(0, 262144, size=(3, 8, 8)).astype(np.int64)
    z2 = lfq.get_codebook_entry(torch.from_numpy(tok2.reshape(3, 64)), bhwc=(3, 8, 8, 18)).flip(1).float()
    y2 = dec2(z2)
    enc2 = RefEnc(rcfg2)
    enc2.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd2.items() if k.startswith("encoder.")})
    enc2.eval()
    frames2 = g.integers(0, 256, size=(3, 3, 32, 32)).astype(np.uint8)
    h2 = enc2(torch.from_numpy(frames2).float() / 127.5 - 1.0)
    o2 = {"cfg": np.array(repr(mid)), "weight_seed": 2, "dec_tokens": tok2, "dec_out_f32": y2.numpy(),
          "dec_u8_f32": ref_vis.rescale_magvit_output(y2).numpy(), "enc_frames": frames2, "enc_h": h2.numpy()}
    np.savez_compressed(os.path.join(OUT, "magvit_mid.npz"), **o2)
    print("magvit_mid: dec out range", float(y2.min()), float(y2.max()), y2.shape)
    print("magvit_small: dec out range", float(y32.min()), float(y32.max()), "enc |h| min", out["enc_min_abs_h"])


def magvit_full_fixture():
    """The SHIPPED tokenizer geometry (magvit2/config.py:9-43: base 128, ch_mult (1,1,2,2,4), 2 ResBlocks, 18-bit
    codebook): one 16x16-token frame through the reference Decoder (improved_model.py:162-182) and one 256x256 RGB
    frame through the reference Encoder (:103-121), each in f32 and as the bf16 module the reference actually runs
    (visualize.py:97-101), so that the GPU test can hold the hand-written conv stack to the reference's own
    bf16-vs-f32 error."""
    from magvit2.config import VQConfig as RefVQ
    from magvit2.modules.diffusionmodules.improved_model import Encoder as RefEnc, Decoder as RefDec
    from magvit2.modules.vqvae.lookup_free_quantize import LFQ
    import visualize as ref_vis
    mv = importlib.import_module("1xgpt_amd.magvit2")
    rcfg = RefVQ()
    mine = mv.VQModel(mv.VQConfig())
    sd = mv.make_vq_state_dict(mine, seed=3)
    enc, dec = RefEnc(rcfg), RefDec(rcfg)
    enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("encoder.")})
    dec.load_state_dict({k[len("decoder."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("decoder.")})
    enc.eval(), dec.eval()
    g = np.random.default_rng(31)
    lfq = LFQ(rcfg)
    tok = g.integers(0, 262144, size=(1, 16, 16)).astype(np.int64)
    z = lfq.get_codebook_entry(torch.from_numpy(tok.reshape(1, 256)), bhwc=(1, 16, 16, 18)).flip(1).float()
    y32 = dec(z)
    dec16 = RefDec(rcfg)
    dec16.load_state_dict(dec.state_dict())
    dec16 = dec16.to(torch.bfloat16).eval()
    y16 = dec16(z.to(torch.bfloat16))
    out = {"weight_seed": 3, "dec_tokens": tok, "dec_out_f32": y32.numpy(),
           "dec_out_bf16_bits": y16.view(torch.int16).numpy(),
           "dec_u8_f32": ref_vis.rescale_magvit_output(y32).numpy(),
           "dec_u8_bf16": ref_vis.rescale_magvit_output(y16).numpy()}
    # a smooth-ish synthetic frame (low-pass noise) so that the encoder sees image-like statistics, plus white noise
    base = g.standard_normal((1, 3, 32, 32)).astype(np.float32)
    up = torch.nn.functional.interpolate(torch.from_numpy(base), size=(256, 256), mode="bicubic", align_corners=False)
    img = (up * 60 + 128 + torch.from_numpy(g.standard_normal((1, 3, 256, 256)).astype(np.float32)) * 12).clamp(0, 255)
    frames = img.to(torch.uint8).numpy()
    xin = torch.from_numpy(frames).float() / 127.5 - 1.0
    h32 = enc(xin)
    enc16 = RefEnc(rcfg)
    enc16.load_state_dict(enc.state_dict())
    enc16 = enc16.to(torch.bfloat16).eval()
    h16 = enc16(xin.to(torch.bfloat16))
    out.update({"enc_frames": frames, "enc_h_f32": h32.numpy(), "enc_h_bf16_as_f32": h16.float().numpy()})
    np.savez_compressed(os.path.join(OUT, "magvit_full.npz"), **out)
    d = (out["dec_u8_bf16"].astype(np.int32) - out["dec_u8_f32"].astype(np.int32))
    print("magvit_full: dec range", float(y32.min()), float(y32.max()), "ref bf16-vs-f32 u8 |d| mean", np.abs(d).mean(),
          "max", np.abs(d).max(), "| enc h std", float(h32.std()), "bit flips bf16 vs f32",
          int(((h32 > 0) != (h16.float() > 0)).sum()), "of", h32.numel())


def generate_fixture(name, cfg_kwargs, wseed, clip_seed=300):
    """BASELINE config 3 at full size: generate.py semantics (generate.py:77-103: prompt 8 frames, sample frames 8..15
    autoregressively, each with `maskgit_steps` MaskGIT steps at temperature 0) for steps 2 and 8 (schedule
    st_mask_git.py:199).  Over 8 frames x steps forwards x 512 argmax decisions SOME top-2 logit gap is always within
    f32 accumulation noise, so the smallest gap is recorded PER FRAME: a test holds frames with a robust gap to
    bit-exact ids (with the reference's own earlier frames as the prompt) and the fragile ones to near-equality."""
    model, cfg = build_ref_model(cfg_kwargs, wseed)
    H = W = math.isqrt(cfg.S)
    ids = synthetic.make_clips(1, cfg, seed=clip_seed)
    example = torch.from_numpy(ids).reshape(1, cfg.T, H, W)
    out = {"clip_seed": clip_seed, "weight_seed": wseed, "ids": ids}
    for steps in (2, 8):
        frame_gaps, noises, samples = [], [], []
        prompt = example.clone()
        prompt[:, 8:] = model.mask_token_id
        torch.manual_seed(9000 + steps)
        for t in range(8, cfg.T):
            with Recorder(model) as rec:
                rec.out_t = t
                s_hw, _ = model.maskgit_generate(prompt, out_t=t, maskgit_steps=steps, temperature=0)
            samples.append(s_hw)
            prompt[:, t] = s_hw
            frame_gaps.append(rec.min_gap if conf_gap(np.stack(rec.noise)) > 0 else 0.0)
            noises.append(np.stack(rec.noise).reshape(steps - 1, 1, cfg.S))
            print(f"  {name}: steps={steps} frame {t} min top-2 gap {frame_gaps[-1]:.3e}", flush=True)
        outs = torch.cat([example[:, :8], torch.stack(samples, 1), example[:, 8:]], 1)
        out[f"gen_s{steps}_outputs"] = outs.numpy().astype(np.int32)   # [prompt | generated | ground truth], 24 frames
        out[f"gen_s{steps}_noise"] = np.stack(noises)                    # (8 frames, steps-1, 1, S)
        out[f"gen_s{steps}_frame_gap"] = np.array(frame_gaps, np.float64)
    out["mup_pinned"] = np.int64(0 if cfg.use_mup else 1)
    out["cfg"] = np.array(repr(cfg_kwargs))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: frame gaps s2 {out['gen_s2_frame_gap']} s8 {out['gen_s8_frame_gap']}")


class _Fragile(Exception):
    """A timestep of a candidate clip whose smallest top-2 gap is below the bar of a robust-fixture search."""


def evaluate_fixture(name, cfg_kwargs, wseed, clip_seed=1234, noise_seed=4242, min_gap=None, model_cfg=None):
    """The BENCHMARKED workload at full size (bench.py: teacher-forced evaluate, genie/evaluate.py:82-122, 2 MaskGIT steps,
    temperature 0) on bench.py's own weights (seed 0) and its clip 0 (synthetic.make_clips(.., seed=1234)[0]): the reference's
    predict_zframe_logits + compute_loss on that clip.  The "random" unmasking draws are INJECTED (torch.rand_like returns
    synthetic.make_noise(seed=noise_seed) slices) so that a batched GPU run can replay them for this clip beside other clips.
    30 forwards x 512 argmax decisions: the smallest top-2 gap is recorded per timestep (robust timesteps are held to
    bit-exact ids, fragile ones to near-equality), and the per-timestep CE so that a test can localise a deviation."""
    """min_gap: give up (raise _Fragile) at the first timestep whose smallest top-2 gap is <= min_gap -- the robust-fixture search
    (robust_evaluate_fixture) walks clip seeds until all 15 timesteps pass; model_cfg: an already built (model, cfg) pair."""
    model, cfg = model_cfg if model_cfg is not None else build_ref_model(cfg_kwargs, wseed)
    H = W = math.isqrt(cfg.S)
    ids = synthetic.make_clips(1, cfg, seed=clip_seed)
    noise = synthetic.make_noise((cfg.T - 1, 1, 1, cfg.S), seed=noise_seed)
    x = torch.from_numpy(ids).reshape(1, cfg.T, H, W)
    ref_evaluate.WINDOW_SIZE = cfg.T
    ev = object.__new__(ref_evaluate.GenieEvaluator)
    ev.model, ev.device, ev.decode_latents = model, "cpu", None
    ev.args = SimpleNamespace(maskgit_steps=2, temperature=0, latent_h=H, latent_w=W)
    gaps, draws = [], iter(noise[:, 0])
    orig_rand_like, orig_mg, orig_logits = torch.rand_like, model.maskgit_generate, model.compute_logits
    state = {"t": None, "gap": float("inf")}

    def rand_like(t, *a, **k):
        return torch.from_numpy(next(draws).reshape(tuple(t.shape)).copy())

    def compute_logits(xx):
        lg = orig_logits(xx)
        f = lg[:, :, state["t"]].reshape(1, 2, 512, -1)
        top2 = f.topk(2, dim=2).values
        state["gap"] = min(state["gap"], float((top2[:, :, 0] - top2[:, :, 1]).min()))
        return lg

    def mg(prompt, out_t, **kw):
        state["t"], state["gap"] = out_t, float("inf")
        r = orig_mg(prompt, out_t, **kw)
        gaps.append(state["gap"])
        print(f"  {name}: timestep {out_t} min top-2 gap {state['gap']:.3e}", flush=True)
        if min_gap is not None and state["gap"] <= min_gap:
            raise _Fragile(f"clip seed {clip_seed}: timestep {out_t} gap {state['gap']:.3e}")
        return r

    torch.rand_like, model.maskgit_generate, model.compute_logits = rand_like, mg, compute_logits
    try:
        samples, fl = ev.predict_zframe_logits(torch.from_numpy(ids))
    finally:
        torch.rand_like, model.maskgit_generate, model.compute_logits = orig_rand_like, orig_mg, orig_logits
    out = {"clip_seed": clip_seed, "weight_seed": wseed, "noise_seed": noise_seed, "ids": ids,
           "ev_samples": samples.numpy().astype(np.int32), "ev_noise": noise,
           "ev_loss": np.float64(ref_eval_utils.compute_loss(torch.from_numpy(ids), fl)),
           "ev_acc": np.float64((x[:, 1:] == samples).float().mean().item()),
           "ev_frame_gap": np.array(gaps, np.float64)}
    # CE of each timestep on its own: the reference's compute_loss on a two-frame slice [frame 0, frame k+1] (it reads
    # labels[:, 1:] and takes T from the logits, eval_utils.py:66-73)
    per_t = []
    clip = ids.reshape(1, cfg.T, -1)
    for k in range(cfg.T - 1):
        lab = torch.from_numpy(np.concatenate([clip[:, :1], clip[:, k + 1:k + 2]], 1).reshape(1, -1))
        per_t.append(ref_eval_utils.compute_loss(lab, fl[:, :, :, k:k + 1]))
    out["ev_loss_per_t"] = np.array(per_t, np.float64)
    g = np.random.default_rng(5)
    pk, ps = g.integers(0, cfg.T - 1, 64), g.integers(0, cfg.S, 64)
    out["probe_k"], out["probe_s"] = pk, ps
    out["probe_logits"] = np.stack([fl[0, :, :, k, s // W, s % W].numpy() for k, s in zip(pk, ps)], 0)  # (64, 512, 2)
    out["mup_pinned"] = np.int64(0 if cfg.use_mup else 1)
    out["cfg"] = np.array(repr(cfg_kwargs))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: ev_loss={out['ev_loss']:.6f} ev_acc={out['ev_acc']:.6f} gaps {out['ev_frame_gap']}")



def robust_evaluate_fixture(name, cfg_kwargs, wseed, first_seed, bar=6e-5, max_tries=400):
    """An evaluate fixture whose 15 timesteps ALL have a smallest top-2 logit gap above `bar` (the tests' ROBUST), so that a test can
    hold every sampled id bit-exact without a fragile branch: walk clip seeds first_seed, first_seed + 1, ... (a candidate is dropped
    at its first fragile timestep) and keep the first clip that passes.  Same weights as bench.py (seed 0)."""
    mc = build_ref_model(cfg_kwargs, wseed)
    for k in range(max_tries):
        try:
            evaluate_fixture(name, cfg_kwargs, wseed, clip_seed=first_seed + k, noise_seed=4242 + k, min_gap=bar, model_cfg=mc)
            print(f"{name}: clip seed {first_seed + k} is robust after {k + 1} candidates", flush=True)
            return
        except _Fragile as e:
            print(f"  {name}: dropped -- {e}", flush=True)
    raise SystemExit(f"{name}: no robust clip in {max_tries} candidates")


def main():
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["tiny", "shape", "c35", "c138", "harness", "magvit", "magvit_full", "c138_gen", "vocab"]
    if "magvit_full" in which:
        magvit_full_fixture()
    c138 = dict(num_layers=32, d_model=512, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    if "c138_ev" in which:      # not in the default list: ~2 minutes of reference forwards each
        evaluate_fixture("ev_c138", dict(c138, num_heads=8), 0)
    if "c138_ev_h16" in which:
        evaluate_fixture("ev_c138_h16", dict(c138, num_heads=16), 0)
    if "c35_ev" in which:       # BASELINE config 1's workload on the SHIPPED config (genie/configs/magvit_n32_h8_d256.json) at full depth
        evaluate_fixture("ev_c35", dict(num_layers=32, num_heads=8, d_model=256, T=16, S=256, num_factored_vocabs=2, qk_norm=False,
                                        use_mup=False), 0)
    c35 = dict(num_layers=32, num_heads=8, d_model=256, T=16, S=256, num_factored_vocabs=2, qk_norm=False, use_mup=False)
    # the reference's DEFAULT attention variant (genie/config.py:33 qk_norm=True: per-head LayerNorm of q and k, norm1 / norm2 = Identity,
    # attention.py:31-34,42-47, st_transformer.py:44,67) on the GENIE_138M shape, and the dataclass defaults proper (qk_norm + use_mup:
    # scale 8 / head_dim, readout x 256 / d -- the muP readout factor is the placeholder's, mup_pinned = 0)
    if "c138_ev_qknorm" in which:
        evaluate_fixture("ev_c138_qknorm", dict(c138, num_heads=8, qk_norm=True), 0)
    if "c138_gen_qknorm" in which:
        generate_fixture("gen_c138_qknorm", dict(c138, num_heads=8, qk_norm=True), 0)
    if "c138_ev_default" in which:
        evaluate_fixture("ev_c138_default", dict(c138, num_heads=8, qk_norm=True, use_mup=True), 0)
    if "c35_ev_robust" in which:    # every timestep's smallest top-2 gap above the tests' bar: ids bit-exact with no fragile branch
        robust_evaluate_fixture("ev_c35_robust", c35, 0, 5000)
    if "c138_ev_robust" in which:
        robust_evaluate_fixture("ev_c138_robust", dict(c138, num_heads=8), 0, 6000)
    if "c138_gen" in which:
        generate_fixture("gen_c138", dict(num_layers=32, num_heads=8, d_model=512, T=16, S=256,
                                          num_factored_vocabs=2, qk_norm=False, use_mup=False), 0)
    if "harness" in which:
        harness_fixture()
    if "magvit" in which:
        magvit_fixture()
    base = dict(num_layers=2, num_heads=2, d_model=64, T=4, S=16, num_factored_vocabs=2)
    if "tiny" in which:
        tiny_fixture("tiny_ln", dict(base, qk_norm=False, use_mup=False), 11)
        tiny_fixture("tiny_qknorm", dict(base, qk_norm=True, use_mup=False), 12)
        tiny_fixture("tiny_mup", dict(base, qk_norm=False, use_mup=True), 13)
        tiny_fixture("tiny_qknorm_mup", dict(base, qk_norm=True, use_mup=True), 14)
    if "vocab" in which:        # vocabularies other than 2 x 512 (image_vocab_size, num_factored_vocabs -> vf, V = nv * vf)
        small = dict(num_layers=2, num_heads=2, d_model=64, T=4, S=16, use_mup=False)
        vocab_fixture("vocab_v4096_n1", dict(small, image_vocab_size=4096, num_factored_vocabs=1, qk_norm=False), 41, n_probe=16)
        vocab_fixture("vocab_v64_n3_qknorm", dict(small, image_vocab_size=262144, num_factored_vocabs=3, qk_norm=True), 42)
        vocab_fixture("vocab_v16_n4", dict(small, image_vocab_size=65536, num_factored_vocabs=4, qk_norm=False), 43)
        vocab_fixture("vocab_v100_n2", dict(small, image_vocab_size=10000, num_factored_vocabs=2, qk_norm=False), 44)
    if "shape" in which:
        real = dict(num_layers=2, T=16, S=256, num_factored_vocabs=2)
        shape_fixture("shape_dh32", dict(real, num_heads=2, d_model=64, qk_norm=False, use_mup=False), 21, 5e-5)
        shape_fixture("shape_dh64", dict(real, num_heads=2, d_model=128, qk_norm=False, use_mup=False), 22, 5e-5)
        shape_fixture("shape_dh64_qknorm", dict(real, num_heads=2, d_model=128, qk_norm=True, use_mup=False), 23,
                      5e-5, do_eval=False, steps_list=(2, 8))
    if "c35" in which:
        shape_fixture("anchor_c35", dict(num_layers=32, num_heads=8, d_model=256, T=16, S=256,
                                         num_factored_vocabs=2, qk_norm=False, use_mup=False), 0, 2e-4,
                      do_eval=False, steps_list=(2,))
    if "c138" in which:
        shape_fixture("anchor_c138", dict(num_layers=32, num_heads=8, d_model=512, T=16, S=256,
                                          num_factored_vocabs=2, qk_norm=False, use_mup=False), 0, 2e-4,
                      do_eval=False, steps_list=(2,))


if __name__ == "__main__":
    main()
