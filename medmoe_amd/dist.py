"""Data-parallel exchange steps of the hot path (torch.distributed plumbing; backend "nccl" is
RCCL over xGMI on MI355X, "gloo" in the CPU tests).

The reference's only collective call sites are src/utils/distributed.py:28-58 (gather_tensor,
used by losses.py:503-524) plus DDP's gradient all-reduce (configs/trainer/ddp.yaml:4).  Here:
  * ONE all-gather of cat([img_g, txt_g]) per step instead of two (losses.py:512-513) - the
    message is latency-bound (<= 0.8 MB/rank), so one hop on the xGMI mesh instead of two;
  * the backward of the gathered keys is ONE reduce-scatter (BackpropType.GLOBAL semantics of
    torch.distributed.nn.functional.all_gather: every rank's gradient for my slice is summed);
  * gradients: one all-reduce over the single flat fp32 gradient buffer of a store (flat.FlatArena.g32: ParamStore, and
    one more for TextStore / each FlatStore of the Swin encoder);
  * opt-in (MedMoEConfig.grad_comm_dtype = "bf16"): the same all-reduces over a bf16 copy of the gradient, scaled by
    1 / world and rounded on the chip before the exchange (what torch DDP's bf16_compress_hook does); half the bytes on the wire.
    `comm` below is the arena (flat.FlatArena) or anything with its `g16` buffer, `pack(lo, hi, scale)` and `g16_reduced` flag.
"""
import torch
import torch.distributed as dist


def is_dist() -> bool:
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


def gather_embeddings(img_g: torch.Tensor, txt_g: torch.Tensor):
    """[B,D],[B,D] -> (img_all [W*B,D], txt_all [W*B,D]) with rank r's rows at [r*B,(r+1)*B)."""
    B, D = img_g.shape
    W = dist.get_world_size()
    packed = torch.cat([img_g, txt_g], dim=1).contiguous()
    out = torch.empty(W * B, 2 * D, device=packed.device, dtype=packed.dtype)
    dist.all_gather_into_tensor(out, packed)
    return out[:, :D].contiguous(), out[:, D:].contiguous()


def gather_rows(t: torch.Tensor) -> torch.Tensor:
    """[B, ...] -> [W*B, ...] with rank r's rows at [r*B, (r+1)*B) (no gradient: frozen text features, caption lengths, similarities)."""
    t = t.contiguous()
    out = torch.empty((dist.get_world_size() * t.shape[0],) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    if t.is_cuda and dist.get_backend() != "nccl":
        torch.cuda.synchronize()                                  # gloo reads the buffer from the host right away (tests)
    dist.all_gather_into_tensor(out, t)
    return out


def scatter_key_grads(d_all: torch.Tensor) -> torch.Tensor:
    """Sum over ranks of d_all [W*B,D]; returns this rank's [B,D] slice (reduce-scatter)."""
    W = dist.get_world_size()
    B = d_all.shape[0] // W
    out = torch.empty(B, d_all.shape[1], device=d_all.device, dtype=d_all.dtype)
    dist.reduce_scatter_tensor(out, d_all.contiguous())
    return out


def _all_reduce_bf16(t: torch.Tensor, async_op: bool = False):
    """Sum a bf16 slice over the ranks in place; returns the work handle of an async call, else None.  RCCL sums bf16 on the device.  gloo
    (tests: two ranks sharing one GPU) stages device tensors through the host anyway and sums bf16 on host tensors only, so there the slice
    is reduced as a host copy and copied back."""
    if t.is_cuda and dist.get_backend() != "nccl":
        torch.cuda.synchronize()                                  # as for fp32: the producers have to be finished before the host reads
        host = t.cpu()
        dist.all_reduce(host)
        t.copy_(host)
        return None
    return dist.all_reduce(t, async_op=async_op) if async_op else dist.all_reduce(t)


def allreduce_mean_(flat_grad: torch.Tensor, comm=None):
    """Average an un-bucketed gradient arena over the ranks.  comm (bf16 exchange): `flat_grad` is packed into comm.g16 with the 1 / world
    scale, g16 is summed over the ranks and marked as the step's reduced gradient; flat_grad itself is not touched."""
    if comm is not None:
        allreduce_mean_start(flat_grad, comm).finish()
        return comm.g16
    if flat_grad.is_cuda and dist.get_backend() != "nccl":
        torch.cuda.synchronize()                                  # gloo reads the buffer from the host right away (tests)
    dist.all_reduce(flat_grad)
    flat_grad.div_(dist.get_world_size())
    return flat_grad


def allreduce_mean_start(flat_grad: torch.Tensor, comm=None) -> "BucketedAllReduce":
    """allreduce_mean_ in two halves, for an arena whose all-reduce runs underneath later work: the exchange of the whole arena is launched
    here (one bucket of a BucketedAllReduce, so the pack / reduce / flag protocol of the bf16 exchange lives in that class alone) and the
    caller joins it with `.finish()` on the returned reducer."""
    red = BucketedAllReduce(flat_grad, [0, flat_grad.numel()], comm=comm)
    red.ready(0)
    return red


def label_offset(local_batch: int) -> int:
    """labels = B_loc*rank + arange(B_loc)  (losses.py:516-518)."""
    return local_batch * dist.get_rank()


class BucketedAllReduce:
    """Overlaps the gradient all-reduce with the hand-scheduled backward: the flat fp32 gradient buffer is
    cut into contiguous buckets in the order the backward FINISHES them (MoE/router first, ViT layers
    L-1..0, embeddings last); `ready(i)` launches an async all-reduce of bucket i on RCCL's stream (it
    waits for the kernels already enqueued on the compute stream), `finish()` joins them and averages.
    One message per ViT layer (7.1 M fp32 = 28 MB): large enough to run at link rate on the xGMI mesh,
    small enough that only the last bucket is exposed.
    comm (bf16 exchange): `ready(i)` first packs bucket i into comm.g16 on the compute stream (bf16(g * 1 / world)) and all-reduces that
    slice; `finish()` joins, marks comm.g16 as the step's reduced gradient and leaves flat_grad alone - the scale went in before the
    rounding, so nothing is divided afterwards."""

    def __init__(self, flat_grad: torch.Tensor, boundaries, comm=None):
        # boundaries: ascending element offsets [0, ..., numel]; bucket i = [b[i], b[i+1])
        b = list(boundaries)
        if b[0] != 0 or b[-1] != flat_grad.numel() or any(b[i] >= b[i + 1] for i in range(len(b) - 1)):
            raise ValueError("bucket boundaries must cover the flat gradient exactly once")
        self.flat, self.b, self.work, self.comm = flat_grad, b, {}, comm

    @property
    def n_buckets(self):
        return len(self.b) - 1

    def ready(self, i: int):
        if i in self.work:
            raise RuntimeError(f"bucket {i} reduced twice")
        if self.comm is not None:
            lo, hi = self.b[i], self.b[i + 1]
            self.comm.pack(lo, hi, 1.0 / dist.get_world_size())
            self.work[i] = _all_reduce_bf16(self.comm.g16[lo:hi], async_op=True)
            return
        if self.flat.is_cuda and dist.get_backend() != "nccl":
            # RCCL enqueues the collective behind the kernels already on the compute stream; gloo reads the buffer
            # from the host right away, so the producers have to be finished first (tests / tools/two_rank_gpu.py)
            torch.cuda.synchronize()
        self.work[i] = dist.all_reduce(self.flat[self.b[i]: self.b[i + 1]], async_op=True)

    def finish(self):
        if len(self.work) != self.n_buckets:
            missing = [i for i in range(self.n_buckets) if i not in self.work]
            raise RuntimeError(f"gradient buckets never reduced: {missing}")
        for w in self.work.values():
            if w is not None:
                w.wait()
        self.work = {}
        if self.comm is not None:
            self.comm.g16_reduced = True
            return
        self.flat.div_(dist.get_world_size())
