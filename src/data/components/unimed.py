"""Mirror of reference src/data/components/unimed.py:14-19 (`collate_fn`) plus a synthetic stand-in for the UniMed
WebDataset shards (`jpg`/`txt`/`cls` tuples, unimed_datamodule.py:44-46) - there is no dataset and no network here.

The collated batch keeps the reference keys: `image` (list of decoded images), `caption` (list), `label` (LongTensor).
With the device preprocessing of medmoe_amd.data the `image` entries are uint8 [H,W,3] tensors instead of PIL images, and
`caption` entries are token-id rows (or strings when a tokenizer is hooked up, MedMoE.set_vocabulary)."""
from typing import Any, Dict, List

import torch
from torch.utils.data import Dataset


def collate_fn(batch: List[Any]) -> Dict[str, Any]:
    """unimed.py:14-19; samples that carry a segmentation mask (a tensor entry behind the class) add `mask` int8 [B, C, H, W],
    samples that carry grounding annotations (a dict entry) add its keys: `box` int32 [B, NB, 4] and `span` int64 [B, 2]."""
    out = {
        "image": [x[0] for x in batch],
        "caption": [x[1] for x in batch],
        "label": torch.tensor([x[2] for x in batch], dtype=torch.long),
    }
    for k in range(3, len(batch[0]) if batch else 0):
        if isinstance(batch[0][k], dict):
            for key in batch[0][k]:
                out[key] = torch.stack([x[k][key] for x in batch])
        else:
            out["mask"] = torch.stack([x[k] for x in batch])
    return out


def synthetic_mask(num_classes: int, size: int, ignore_frac: float, seed: int) -> torch.Tensor:
    """A seeded int8 [C, size, size] mask in {0, 1, -1}: one to three filled ellipses per class, then a share `ignore_frac` of the pixels
    set to -1 (ignored)."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(size, dtype=torch.float32).reshape(size, 1)
    xs = torch.arange(size, dtype=torch.float32).reshape(1, size)
    out = torch.zeros(num_classes, size, size, dtype=torch.int8)
    for c in range(num_classes):
        for _ in range(int(torch.randint(1, 4, (1,), generator=g))):
            cy, cx = (torch.rand(2, generator=g) * size).tolist()
            ry, rx = ((0.08 + 0.22 * torch.rand(2, generator=g)) * size).tolist()
            out[c][((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2 <= 1.0] = 1
    if ignore_frac > 0.0:
        out[torch.rand(num_classes, size, size, generator=g) < ignore_frac] = -1
    return out


def synthetic_boxes(num_boxes: int, size: int, n_tokens: int, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded grounding annotations of a sample: `box` int32 [num_boxes, 4] = (x0, y0, x1, y1), half-open rectangles inside the size x size
    frame, the first always present, each later one absent (all zero) with probability 1/2; `span` int64 [2], a half-open span of one to
    three WORDS of a caption of n_tokens tokens ([CLS] and [SEP] among them; every other token of the synthetic vocabulary is a word)."""
    g = torch.Generator().manual_seed(seed)
    box = torch.zeros(num_boxes, 4, dtype=torch.int32)
    for k in range(num_boxes):
        x0, y0 = (int(v) for v in torch.randint(0, max(1, size - 1), (2,), generator=g))
        w, h = (int(v) for v in torch.randint(1, max(2, size // 2), (2,), generator=g))
        keep = k == 0 or bool(torch.rand(1, generator=g) < 0.5)
        if keep:
            box[k] = torch.tensor([x0, y0, min(size, x0 + w), min(size, y0 + h)], dtype=torch.int32)
    words = max(1, n_tokens - 2)
    lo = int(torch.randint(0, words, (1,), generator=g))
    hi = min(words, lo + 1 + int(torch.randint(0, 3, (1,), generator=g)))
    return {"box": box, "span": torch.tensor([lo, hi], dtype=torch.long)}


class SyntheticUnimed(Dataset):
    """Seeded (image uint8 [H,W,3], token ids [T], class) tuples with the shapes of the UniMed shards: image sides vary
    (the reference resizes every PIL image to the model size), caption lengths U{8..T}."""

    def __init__(self, n: int = 1024, max_len: int = 77, vocab: int = 28996, n_classes: int = 5, seed: int = 12345,
                 min_side: int = 160, max_side: int = 320, masks: Any = None, boxes: Any = None):
        self.n, self.T, self.V, self.C, self.seed = n, max_len, vocab, n_classes, seed
        self.min_side, self.max_side = min_side, max_side
        # masks = {num_classes, size, ignore_frac}: every sample also yields a seeded segmentation mask, drawn from a generator
        # of its own - the image, caption and class of a sample are the same with and without the block
        self.masks = None
        if masks is not None:
            m = dict(masks)
            unknown = set(m) - {"num_classes", "size", "ignore_frac"}
            if unknown:
                raise KeyError(f"data.masks: unknown keys {sorted(unknown)} (num_classes, size, ignore_frac)")
            self.masks = (int(m.get("num_classes", 1)), int(m.get("size", 224)), float(m.get("ignore_frac", 0.0)))
            if self.masks[0] < 1 or self.masks[1] < 1 or not 0.0 <= self.masks[2] < 1.0:
                raise ValueError(f"data.masks: num_classes >= 1, size >= 1 and 0 <= ignore_frac < 1, got {m}")

        # boxes = {num_boxes, size}: every sample also yields seeded grounding annotations, again from a generator of their own
        self.boxes = None
        if boxes is not None:
            b = dict(boxes)
            unknown = set(b) - {"num_boxes", "size"}
            if unknown:
                raise KeyError(f"data.boxes: unknown keys {sorted(unknown)} (num_boxes, size)")
            self.boxes = (int(b.get("num_boxes", 2)), int(b.get("size", 224)))
            if not 1 <= self.boxes[0] <= 8 or self.boxes[1] < 2:
                raise ValueError(f"data.boxes: 1 <= num_boxes <= 8 and size >= 2, got {b}")

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int):
        g = torch.Generator().manual_seed(self.seed + i)
        h = int(torch.randint(self.min_side, self.max_side + 1, (1,), generator=g))
        w = int(torch.randint(self.min_side, self.max_side + 1, (1,), generator=g))
        img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        ln = int(torch.randint(min(8, self.T), self.T + 1, (1,), generator=g))
        ids = torch.zeros(self.T, dtype=torch.long)
        ids[:ln] = torch.randint(3, self.V, (ln,), generator=g)
        ids[0] = 1
        ids[ln - 1] = 2
        label = int(torch.randint(0, self.C, (1,), generator=g))
        out = (img, ids, label)
        if self.masks is not None:
            out = out + (synthetic_mask(*self.masks, seed=self.seed + i + 0x5E6),)
        if self.boxes is not None:
            out = out + (synthetic_boxes(*self.boxes, n_tokens=ln, seed=self.seed + i + 0xB0C5),)
        return out
