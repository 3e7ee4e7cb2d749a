"""RawTokenDataset -- reader of the 1X token dataset layout (counterpart of the reference's data.py:17-106).

On disk: ``metadata.json`` {num_images, s, vocab_size, hz, token_dtype?}, ``video.bin`` = (num_images, s, s) tokens
(uint32 by default), optional ``segment_ids.bin`` = (num_images,) int32, optional ``actions.bin`` = (num_images,) uint16 (the
action of each frame; items then carry ``action_ids`` (window_size,) int64 aligned with the frames), optional ``states.bin`` =
(num_images, A) float32 (the continuous action vector of each frame, A = metadata["state_dim"] or the file size over num_images; items
then carry ``action_vectors`` (window_size, A) float32).  Windows of ``window_size`` frames spaced
``stride`` apart; ``filter_interrupts`` drops windows whose first and last frame belong to different segments,
``filter_overlaps`` keeps each frame in at most one window.  Same constructor, attributes (``data``,
``metadata``, ``valid_start_inds``) and item dict as the reference.  ``get_maskgit_collator`` is the training
collator of data.py:109-169 (random corruption + MaskGIT masking) on whatever device the clips are on.
"""
import json
import math
import random
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset as TorchDataset


def _window_starts(n_frames, span, segment_ids=None):
    """First-frame indices of all windows that fit (their last frame is `span` frames later); with `segment_ids`, only windows
    that begin and end in the same recording segment."""
    starts = np.arange(max(n_frames - span, 0))
    if segment_ids is not None and len(starts):
        seg = np.asarray(segment_ids)
        starts = starts[seg[starts] == seg[starts + span]]
    return starts.tolist()


def _drop_shared_frames(starts, window_size, stride):
    """Walk the (increasing) window starts and keep one only if it shares no frame with a window kept before: two windows on
    the same stride grid share a frame exactly when their starts differ by stride, 2 stride, ..., (window_size - 1) stride.
    (Equivalent to the reference's scan over its most recent kept entries, data.py:72-88: kept starts are distinct integers, so
    every one close enough to collide is among them.)"""
    kept, seen = [], set()
    for s0 in starts:
        if not any((s0 - i * stride) in seen for i in range(1, window_size)):
            kept.append(s0)
            seen.add(s0)
    return kept


class RawTokenDataset(TorchDataset):
    def __init__(self, data_dir, window_size, stride=1, filter_interrupts=True, filter_overlaps=False):
        root = Path(data_dir)
        self.metadata = json.loads((root / "metadata.json").read_text())
        n, side = self.metadata["num_images"], self.metadata["s"]
        self.data = np.memmap(root / "video.bin", mode="r", shape=(n, side, side),
                              dtype=np.dtype(self.metadata.get("token_dtype", "uint32")))
        seg_file = root / "segment_ids.bin"
        self.segment_ids = np.memmap(seg_file, dtype=np.int32, mode="r", shape=(n,)) if seg_file.is_file() else None
        act_file = root / "actions.bin"   # (the reference names it and leaves it commented out, data.py:44-48)
        self.actions = np.memmap(act_file, dtype=np.uint16, mode="r", shape=(n,)) if act_file.is_file() else None
        vec_file = root / "states.bin"    # continuous per-frame action vectors (this project's name: the reference ships no such file)
        self.action_vectors = None
        if vec_file.is_file():
            A = self.metadata.get("state_dim")
            if A is None:
                A, rem = divmod(vec_file.stat().st_size, 4 * n) if n else (0, 1)
                if rem or A < 1:
                    raise ValueError(f"states.bin: {vec_file.stat().st_size} bytes are not {n} rows of float32 vectors")
            self.action_vectors = np.memmap(vec_file, dtype=np.float32, mode="r", shape=(n, int(A)))
        if filter_interrupts and self.segment_ids is None:
            raise NotImplementedError("Cannot filter interrupted sequences without segment ids.")
        self.window_size, self.stride = window_size, stride
        self.video_len = (window_size - 1) * stride          # distance from a window's first frame to its last
        self.valid_start_inds = _window_starts(len(self.data), self.video_len, self.segment_ids if filter_interrupts else None)
        if filter_overlaps:
            self.valid_start_inds = _drop_shared_frames(self.valid_start_inds, window_size, stride)

    def __len__(self):
        return len(self.valid_start_inds)

    def __getitem__(self, idx):
        start_ind = self.valid_start_inds[idx]
        x = torch.from_numpy((self.data[start_ind: start_ind + self.video_len + 1: self.stride]).astype(np.int64))
        x = x.flatten()
        item = {"input_ids": x, "labels": x, "attention_mask": torch.ones_like(x)}
        if self.actions is not None:   # same frames as the window
            item["action_ids"] = torch.from_numpy(self.actions[start_ind: start_ind + self.video_len + 1: self.stride].astype(np.int64))
        if self.action_vectors is not None:
            item["action_vectors"] = torch.from_numpy(
                np.array(self.action_vectors[start_ind: start_ind + self.video_len + 1: self.stride], dtype=np.float32))
        return item

    def batch(self, idxs):
        """Stack several windows -> (len(idxs), window_size * s * s) int64 (what default_data_collator builds)."""
        return torch.stack([self[i]["input_ids"] for i in idxs])

    def action_batch(self, idxs):
        """The windows' per-frame actions -> (len(idxs), window_size) int64 (needs actions.bin)."""
        if self.actions is None:
            raise FileNotFoundError("this dataset has no actions.bin")
        return torch.stack([self[i]["action_ids"] for i in idxs])

    def action_vector_batch(self, idxs):
        """The windows' per-frame action vectors -> (len(idxs), window_size, A) float32 (needs states.bin)."""
        if self.action_vectors is None:
            raise FileNotFoundError("this dataset has no states.bin")
        return torch.stack([self[i]["action_vectors"] for i in idxs])


def write_token_dataset(data_dir, tokens: np.ndarray, segment_ids: np.ndarray = None, hz=30, vocab_size=262144,
                        token_dtype="uint32", extra_metadata=None, actions: np.ndarray = None, action_vectors: np.ndarray = None):
    """Write (num_images, s, s) tokens in the dataset layout (used by generate and by the tests); `actions`: (num_images,)
    per-frame action ids in [0, 65536) -> actions.bin (uint16); `action_vectors`: (num_images, A) finite floats -> states.bin (float32)
    and metadata["state_dim"] = A."""
    data_dir = Path(data_dir)
    data_dir.mkdir(parents=True, exist_ok=True)
    tokens = np.asarray(tokens)
    tokens.astype(np.dtype(token_dtype)).tofile(data_dir / "video.bin")
    if segment_ids is not None:
        np.asarray(segment_ids, dtype=np.int32).tofile(data_dir / "segment_ids.bin")
    if actions is not None:
        a = np.asarray(actions)
        if a.shape != (tokens.shape[0],) or (a.size and (a.min() < 0 or a.max() > 0xFFFF)):
            raise ValueError(f"actions must be ({tokens.shape[0]},) integers in [0, 65536), got shape {a.shape}")
        a.astype(np.uint16).tofile(data_dir / "actions.bin")
    meta = {"num_images": int(tokens.shape[0]), "s": int(tokens.shape[1]), "vocab_size": vocab_size, "hz": hz,
            "token_dtype": token_dtype}
    if action_vectors is not None:
        v = np.asarray(action_vectors)
        if v.ndim != 2 or v.shape[0] != tokens.shape[0] or v.shape[1] < 1 or not np.isfinite(v).all():
            raise ValueError(f"action_vectors must be ({tokens.shape[0]}, A >= 1) finite floats, got shape {v.shape}")
        v.astype(np.float32).tofile(data_dir / "states.bin")
        meta["state_dim"] = int(v.shape[1])
    meta.update(extra_metadata or {})
    with open(data_dir / "metadata.json", "w") as f:
        json.dump(meta, f)
    return meta


# ------------------------------------------------------------------ MaskGIT training collator (data.py:109-169)
class TorchDraws:
    """The collator's random draws, in the reference's call order, from torch's / Python's global generators."""

    def __init__(self, device):
        self.device = device

    def rand(self, shape):
        return torch.rand(tuple(shape), device=self.device)

    rand_like = rand

    def randint(self, high, shape):
        return torch.randint(low=0, high=high, size=tuple(shape), dtype=torch.long, device=self.device)

    def py_random(self):
        return random.random()

    def py_randint(self, a, b):
        return random.randint(a, b)

    def py_uniform(self, a, b):
        return random.uniform(a, b)


def maskgit_collate(input_ids, config, draws=None, action_ids=None, action_dropout=0.0, null_action=None, action_vectors=None):
    """(B, T*S) int64 clips -> {"input_ids", "labels"} following data.py:112-167 draw for draw.

    `draws` replays captured draws (parity tests); None draws fresh ones on the clips' device.  `action_ids` (B, T), if given,
    are passed through as batch["action_ids"] (int64, on the clips' device) and draw nothing.
    `action_dropout` > 0 (no reference counterpart) trains the null action of classifier-free guidance: after every other draw, ONE
    uniform per clip is drawn (draws.rand((B,))) and a clip whose draw is below `action_dropout` gets `null_action` at all T frames.
    At 0.0 nothing is drawn: the generator state and the batch are those of before.
    `action_vectors` (B, T, A) floats (a model with config.action_dim > 0) are passed through as batch["action_vectors"] in float32
    and draw nothing; with `action_dropout` > 0 the same ONE uniform per clip is drawn, after every other draw, and the batch carries
    batch["action_drop"], a (B,) bool: the trainer points a dropped clip's frames at the model's learned null row (no null_action)."""
    if not 0.0 <= action_dropout <= 1.0:
        raise ValueError(f"action_dropout must be in [0, 1], got {action_dropout!r}")
    if action_ids is not None and action_vectors is not None:
        raise ValueError("pass action_ids or action_vectors, not both")
    if action_dropout > 0.0 and action_vectors is None:
        if action_ids is None:
            raise ValueError("action_dropout needs action_ids or action_vectors")
        if null_action is None or not 0 <= int(null_action) < max(int(config.action_vocab_size), 1):
            raise ValueError(f"action_dropout needs null_action in [0, {config.action_vocab_size}), got {null_action!r}")
    ids = input_ids.to(torch.int64)
    dev = ids.device
    draws = draws or TorchDraws(dev)
    B = ids.shape[0]
    h = w = math.isqrt(config.S)
    nv, Vf = config.num_factored_vocabs, config.factored_vocab_size
    mask_token_id = config.image_vocab_size
    x_THW = ids.reshape(B, config.T, h, w)
    powers = Vf ** torch.arange(nv, device=dev)
    x_THWC = (x_THW.unsqueeze(-1) // powers) % Vf
    labels = x_THW.clone()

    def t(a, dtype):
        return torch.as_tensor(a, device=dev).to(dtype)

    r = t(draws.rand(x_THWC.shape), torch.float32)
    u01 = t(draws.rand(()), torch.float32)
    random_values = t(draws.randint(Vf, x_THWC.shape), torch.long)
    m = r < config.max_corrupt_rate * u01
    x_THWC = torch.where(m, random_values, x_THWC)
    if draws.py_random() < config.non_mlm_ratio:
        first = draws.py_randint(config.num_prompt_frames, config.T - 1)
        correct_rate = draws.py_uniform(0.25, 1.0)
        for i in range(config.T - first):
            correct_rate *= draws.py_uniform(0.9, 1.0)
            r = t(draws.rand((B, h, w, nv)), torch.float32)
            m = r > correct_rate
            x_THWC[:, first + i] = torch.where(m, random_values[:, first + i], x_THWC[:, first + i])
    else:
        first = 1
    while True:
        u = t(draws.rand((B, config.T - first, 1, 1)), torch.float32)
        prob = torch.cos(u * torch.pi / 2)
        r = t(draws.rand_like((B, config.T - first, h, w)), torch.float32)
        mask = r < prob
        if bool(mask.any()):
            break
    x = (x_THWC * powers).sum(-1)
    x[:, first:][mask] = mask_token_id
    out = {"input_ids": x.reshape(B, -1), "labels": labels.reshape(B, -1)}
    if action_ids is not None:
        out["action_ids"] = torch.as_tensor(action_ids).to(device=dev, dtype=torch.int64).reshape(B, config.T)
        if action_dropout > 0.0:
            drop = t(draws.rand((B,)), torch.float32) < action_dropout
            out["action_ids"] = torch.where(drop[:, None], int(null_action), out["action_ids"])
    if action_vectors is not None:
        out["action_vectors"] = torch.as_tensor(action_vectors).to(device=dev, dtype=torch.float32).reshape(B, config.T, -1)
        if action_dropout > 0.0:
            out["action_drop"] = t(draws.rand((B,)), torch.float32) < action_dropout
    return out


def get_maskgit_collator(config, action_dropout=0.0, null_action=None):
    """collate_fn(features: list of {"input_ids": (T*S,) tensor}) -> batch dict, as data.py:109; action_dropout / null_action as in
    maskgit_collate."""
    def collate_fn(features):
        acts = torch.stack([ex["action_ids"] for ex in features]) if "action_ids" in features[0] and not config.action_dim else None
        vecs = torch.stack([ex["action_vectors"] for ex in features]) if "action_vectors" in features[0] and config.action_dim else None
        return maskgit_collate(torch.stack([ex["input_ids"] for ex in features]), config, action_ids=acts,
                               action_dropout=action_dropout, null_action=null_action, action_vectors=vecs)
    return collate_fn
