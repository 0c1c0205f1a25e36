"""Phrase grounding: a word span of a caption becomes a heat map over the image regions (medmoe_amd.ops.ground_maps), the map is
upsampled and scored against the boxes that annotate the phrase (ops.ground_score) - the pointing game, the contrast-to-noise ratio and a
thresholded IoU / Dice, the MS-CXR-style evaluation.  Two launches of csrc/ground.hip; the records they leave are a few numbers per entry.

`GroundBank` keeps an evaluation epoch's sums on the device (int64 and float64, nothing is read back per batch; ranks add their banks with
a sum), `grounding_metrics` turns them into the reported numbers in float64 on the host.  `word_spans` maps token spans to the word rows of
ws["words"], `prepare_boxes` brings annotation boxes into the form the score launch takes."""
from typing import Dict, Optional, Sequence

import torch

from . import ops


def theta_key(theta: float) -> str:
    """0.5 -> "0.5", 1.0 -> "1": the suffix of the per-threshold metrics."""
    return f"{float(theta):g}"


class GroundBank:
    """Sums over the records of an evaluation epoch, on the device.
    ints int64 [4] = (entries, entries with a box (area > 0), hits among them, entries with a defined CNR);
    sums float64 [1 + 2 NTH] = (sum of CNR, sum of IoU at theta_0, sum of Dice at theta_0, ...), IoU and Dice over the entries with a box."""

    def __init__(self, thetas: Sequence[float], device):
        self.thetas = tuple(float(t) for t in thetas)
        if len(self.thetas) > ops.GROUND_MAX_THETAS:
            raise ValueError(f"GroundBank: at most {ops.GROUND_MAX_THETAS} thresholds, got {len(self.thetas)}")
        self.device = torch.device(device)
        self.ints = torch.zeros(4, device=self.device, dtype=torch.int64)
        self.sums = torch.zeros(1 + 2 * len(self.thetas), device=self.device, dtype=torch.float64)
        self.batches = 0

    def reset(self):
        self.ints.zero_()
        self.sums.zero_()
        self.batches = 0

    def __len__(self):
        return self.batches

    def add(self, records: Dict):
        """records: what ops.ground_score / Engine.ground return (rec_i, rec_d, "size", "thetas")."""
        rec_i, rec_d = records["rec_i"], records["rec_d"]
        nth = len(self.thetas)
        if tuple(float(t) for t in records["thetas"]) != self.thetas:
            raise ValueError(f"GroundBank.add: the records were scored at the thresholds {tuple(records['thetas'])}, the bank holds {self.thetas}")
        if rec_i.dim() != 2 or rec_i.shape[1] != 4 + 2 * nth or rec_i.dtype != torch.int32 or tuple(rec_d.shape) != (rec_i.shape[0], 4) \
                or rec_d.dtype != torch.float64:
            raise ValueError(f"GroundBank.add: expected rec_i int32 [n, {4 + 2 * nth}] and rec_d float64 [n, 4], got {rec_i.dtype} "
                             f"{tuple(rec_i.shape)} and {rec_d.dtype} {tuple(rec_d.shape)}")
        ints, sums = entry_sums(rec_i.to(self.device), rec_d.to(self.device), records["size"], nth)
        self.ints += ints
        self.sums += sums
        self.batches += 1


def entry_cnr(rec_i: torch.Tensor, rec_d: torch.Tensor, size) -> torch.Tensor:
    """float64 [n]: |mu_in - mu_out| / sqrt(var_in + var_out) of every entry from its four sums; NaN where the union is empty, where it fills
    the frame, or where the denominator is 0 (a constant map)."""
    HW = float(int(size[0]) * int(size[1]))
    area = rec_i[:, 3].to(torch.float64)
    d = rec_d.to(torch.float64)
    n_in, n_out = area.clamp(min=1.0), (HW - area).clamp(min=1.0)
    mu_in, mu_out = d[:, 0] / n_in, (d[:, 2] - d[:, 0]) / n_out
    var = (d[:, 1] / n_in - mu_in * mu_in).clamp(min=0.0) + ((d[:, 3] - d[:, 1]) / n_out - mu_out * mu_out).clamp(min=0.0)
    ok = (area > 0) & (area < HW) & (var > 0)
    return torch.where(ok, (mu_in - mu_out).abs() / var.clamp(min=1e-300).sqrt(), torch.full_like(var, float("nan")))


def entry_sums(rec_i: torch.Tensor, rec_d: torch.Tensor, size, nth: int):
    """(ints int64 [4], sums float64 [1 + 2 nth]) of a batch of records, in the layout of GroundBank."""
    area = rec_i[:, 3].to(torch.float64)
    boxed = area > 0
    cnr = entry_cnr(rec_i, rec_d, size)
    has = ~torch.isnan(cnr)
    ints = torch.stack([torch.tensor(rec_i.shape[0], device=rec_i.device), boxed.sum(), (rec_i[:, 2].to(torch.int64) * boxed).sum(), has.sum()]).to(torch.int64)
    parts = [torch.where(has, cnr, torch.zeros_like(cnr)).sum()]
    zero = torch.zeros_like(area)
    for k in range(nth):
        inter, pred = rec_i[:, 4 + 2 * k].to(torch.float64), rec_i[:, 5 + 2 * k].to(torch.float64)
        parts.append(torch.where(boxed, inter / (pred + area - inter).clamp(min=1.0), zero).sum())
        parts.append(torch.where(boxed, 2.0 * inter / (pred + area).clamp(min=1.0), zero).sum())
    return ints, torch.stack(parts).to(torch.float64)


def grounding_metrics(bank: GroundBank) -> Dict[str, float]:
    """{"pg_acc", "cnr_mean", "iou@<theta>", "dice@<theta>", "n_entries"} of a bank, in float64 on the host.  pg_acc: the mean `hit` over the
    entries with a box; cnr_mean: the mean over the entries whose CNR is defined; iou@ / dice@: the means of inter / (pred + area - inter) and
    2 inter / (pred + area) over the entries with a box.  A mean over no entry is NaN; an empty bank gives {}."""
    if len(bank) == 0:
        return {}
    ints, sums = bank.ints.cpu().tolist(), bank.sums.cpu().tolist()
    n, boxed, hits, n_cnr = ints
    mean = lambda s, c: float(s) / c if c else float("nan")
    out = {"pg_acc": mean(hits, boxed), "cnr_mean": mean(sums[0], n_cnr), "n_entries": int(n)}
    for k, t in enumerate(bank.thetas):
        out[f"iou@{theta_key(t)}"] = mean(sums[1 + 2 * k], boxed)
        out[f"dice@{theta_key(t)}"] = mean(sums[2 + 2 * k], boxed)
    return out


def word_spans(seg: torch.Tensor, tok_lo: torch.Tensor, tok_hi: torch.Tensor) -> torch.Tensor:
    """int64 [B, 2]: the half-open WORD spans (rows of ws["words"]) covered by the half-open token spans [tok_lo[b], tok_hi[b]) through the
    word-piece segment map seg [B, T] (VocabTables.segment_map: seg[b, t] = the word row token t is summed into, negative = the token is
    dropped - [CLS], [SEP], padding).  A span without a kept token is refused."""
    seg = torch.as_tensor(seg).detach().cpu().to(torch.int64)
    lo, hi = torch.as_tensor(tok_lo).detach().cpu().to(torch.int64).reshape(-1), torch.as_tensor(tok_hi).detach().cpu().to(torch.int64).reshape(-1)
    if seg.dim() != 2 or lo.numel() != seg.shape[0] or hi.numel() != seg.shape[0]:
        raise ValueError(f"word_spans: seg must be [B, T] with one token span per row, got {tuple(seg.shape)}, {lo.numel()} and {hi.numel()}")
    B, T = seg.shape
    if bool(((lo < 0) | (hi > T) | (lo >= hi)).any()):
        raise ValueError(f"word_spans: a token span is empty or lies outside [0, {T})")
    pos = torch.arange(T).reshape(1, T)
    kept = (pos >= lo.reshape(B, 1)) & (pos < hi.reshape(B, 1)) & (seg >= 0)
    if not bool(kept.any(dim=1).all()):
        b = int((~kept.any(dim=1)).nonzero()[0])
        raise ValueError(f"word_spans: the token span [{int(lo[b])}, {int(hi[b])}) of caption {b} holds no kept token")
    big = torch.full_like(seg, T + 1)
    w_lo = torch.where(kept, seg, big).min(dim=1).values
    w_hi = torch.where(kept, seg, -big).max(dim=1).values + 1
    return torch.stack([w_lo, w_hi], dim=1)


def prepare_boxes(boxes, size, from_size=None, xywh: bool = False, num_boxes: Optional[int] = None) -> torch.Tensor:
    """The boxes as the score launch takes them: int32 [B, NB, 4] = (x0, y0, x1, y1), half-open pixel rectangles of the size = (H, W) frame.
    boxes: [B, NB', 4] or [NB', 4] (one entry), any numeric dtype, xyxy or (x, y, w, h) with xywh=True, in the pixel units of `from_size` =
    (H', W') when given (rescaled by H / H' and W / W').  Edges are rounded OUTWARD (floor the low edge, ceil the high one), clipped to the
    frame, and the list is padded to `num_boxes` rectangles with absent ones (all zero); a rectangle that is empty before rounding stays
    absent."""
    b = torch.as_tensor(boxes).detach().cpu().to(torch.float64)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    if b.dim() != 3 or b.shape[2] != 4:
        raise ValueError(f"prepare_boxes: boxes must be [B, NB, 4] or [NB, 4], got {tuple(b.shape)}")
    H, W = int(size[0]), int(size[1])
    x0, y0, x1, y1 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    if xywh:
        x1, y1 = x0 + x1, y0 + y1
    present = (x1 > x0) & (y1 > y0)
    if from_size is not None:
        sy, sx = H / float(from_size[0]), W / float(from_size[1])
        x0, x1, y0, y1 = x0 * sx, x1 * sx, y0 * sy, y1 * sy
    out = torch.stack([x0.floor().clamp(0, W), y0.floor().clamp(0, H), x1.ceil().clamp(0, W), y1.ceil().clamp(0, H)], dim=-1)
    out = torch.where(present.unsqueeze(-1), out, torch.zeros_like(out)).to(torch.int32)
    nb = out.shape[1] if num_boxes is None else int(num_boxes)
    if not 1 <= nb <= ops.GROUND_MAX_BOXES or out.shape[1] > nb:
        raise ValueError(f"prepare_boxes: {out.shape[1]} rectangles per entry for num_boxes = {nb}; 1 <= num_boxes <= {ops.GROUND_MAX_BOXES}")
    if out.shape[1] < nb:
        out = torch.cat([out, torch.zeros(out.shape[0], nb - out.shape[1], 4, dtype=torch.int32)], dim=1)
    return out.contiguous()
