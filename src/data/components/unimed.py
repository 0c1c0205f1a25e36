"""Mirror of reference src/data/components/unimed.py:14-19 (`collate_fn`) plus a synthetic stand-in for the UniMed
WebDataset shards (`jpg`/`txt`/`cls` tuples, unimed_datamodule.py:44-46) - there is no dataset and no network here.

The collated batch keeps the reference keys: `image` (list of decoded images), `caption` (list), `label` (LongTensor).
With the device preprocessing of medmoe_amd.data the `image` entries are uint8 [H,W,3] tensors instead of PIL images, and
`caption` entries are token-id rows (or strings when a tokenizer is hooked up, MedMoE.set_vocabulary)."""
from typing import Any, Dict, List

import torch
from torch.utils.data import Dataset


def collate_fn(batch: List[Any]) -> Dict[str, Any]:
    """unimed.py:14-19; samples that carry a segmentation mask (a fourth entry) add `mask` int8 [B, C, H, W]."""
    out = {
        "image": [x[0] for x in batch],
        "caption": [x[1] for x in batch],
        "label": torch.tensor([x[2] for x in batch], dtype=torch.long),
    }
    if batch and len(batch[0]) > 3:
        out["mask"] = torch.stack([x[3] for x in batch])
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


class SyntheticUnimed(Dataset):
    """Seeded (image uint8 [H,W,3], token ids [T], class) tuples with the shapes of the UniMed shards: image sides vary
    (the reference resizes every PIL image to the model size), caption lengths U{8..T}."""

    def __init__(self, n: int = 1024, max_len: int = 77, vocab: int = 28996, n_classes: int = 5, seed: int = 12345,
                 min_side: int = 160, max_side: int = 320, masks: Any = None):
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
        if self.masks is None:
            return img, ids, label
        return img, ids, label, synthetic_mask(*self.masks, seed=self.seed + i + 0x5E6)
