"""Thin launch wrappers: torch tensors in, C-ABI calls on torch's CURRENT HIP stream out.

Every function checks dtypes/shapes on the host before the launch (a wrong shape must never
reach a hand-written kernel) and raises on a non-zero return code.  Nothing here computes.
"""
import ctypes
from typing import Optional

import torch

from ._lib import load_library

_c = ctypes
_vp = _c.c_void_p

EPI_NONE, EPI_GELU, EPI_RELU, EPI_MUL_DGELU, EPI_MUL_DRELU, EPI_GELU_DAUX, EPI_MUL_AUX = range(7)

# bench.py sets this to a list to time every launch with HIP events on the launch stream: entries are
# (kernel label, work, "flop" | "byte" | None, start event, end event, detail)
PROFILE = None
_NT_KERNELS = {0: "gemm_nt_kernel", 1: "gemm_nt256_kernel", 2: "gemm_nt512_kernel", 3: "gemm_nt512_kernel<GROUPED>", 4: "gemm_nt4w_kernel",
               5: "gemm_nt4w_kernel<GROUPED>", 6: "gemm_nt_direct_kernel"}


class _Timed:
    """`with _Timed(label, work, unit):` around one launch - HIP events on the current stream when PROFILE is a list, nothing otherwise.
    `label` may be a callable evaluated after the launch (the NT GEMM's kernel is chosen inside the library)."""
    __slots__ = ("label", "work", "unit", "detail", "ev0")

    def __init__(self, label, work=None, unit=None, detail=None):
        self.label, self.work, self.unit, self.detail, self.ev0 = label, work, unit, detail, None

    def __enter__(self):
        if PROFILE is not None:
            self.ev0 = torch.cuda.Event(enable_timing=True)
            self.ev0.record()
        return self

    def __exit__(self, et, ev, tb):
        if self.ev0 is not None and et is None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record()
            PROFILE.append((self.label() if callable(self.label) else self.label, self.work, self.unit, self.ev0, ev1, self.detail))
        return False


def _nt_label():
    return _NT_KERNELS.get(load_library().medmoe_last_gemm_nt_kernel(), "gemm_nt?")


TN_GENERATIONS = ("gemm_tn_kernel", "gemm_tn512_kernel", "gemm_tn4w_kernel")
TN_BUILDS = ("", "<MAPPED>", "<COLG>", "<COLG, SCALE>")


def tn_kernel_id(generation: int, build: int = 0, staged: bool = False) -> int:
    """The id medmoe_last_gemm_tn_kernel reports: generation 0 / 1 / 2 (128x128, tn512, tn4w), build 0..3 (plain, MAPPED, COLG, COLG + SCALE)."""
    return generation * 8 + build * 2 + (1 if staged else 0)


def last_gemm_tn_kernel():
    """medmoe_last_gemm_tn_kernel: (id, split, label) of the most recent TN launch of this process - id as tn_kernel_id (-1 before the first
    launch), split the launch's nsplit (the ROWS per range in the grouped four-wave form)."""
    f = _FN.get("last_gemm_tn_kernel")
    if f is None:
        f = load_library().medmoe_last_gemm_tn_kernel
        f.argtypes = [_c.POINTER(_c.c_int)]
        f.restype = _c.c_int
        _FN["last_gemm_tn_kernel"] = f
    split = _c.c_int(0)
    k = int(f(_c.byref(split)))
    if k < 0:
        return k, 0, "gemm_tn?"
    return k, int(split.value), TN_GENERATIONS[k >> 3] + TN_BUILDS[(k >> 1) & 3] + (" staged" if k & 1 else "")


def _ptr(t: Optional[torch.Tensor]):
    return _vp(0) if t is None else _vp(t.data_ptr())


_raw_stream, _cur_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice


def _stream_handle() -> int:
    """torch's current HIP stream of the current device as a raw handle (torch.cuda.current_stream().cuda_stream is the same value through
    several microseconds of Python per call - milliseconds per step at ~600 launches, tools/host_profile_swin.py)."""
    return _raw_stream(_cur_device())


def _stream():
    return _vp(_stream_handle())


def _chk(rc: int, name: str):
    if rc != 0:
        raise RuntimeError(f"medmoe_{name} failed with code {rc} (-1 bad argument, -2 bad shape, -3 launch error)")


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: medmoe_amd kernels only run on the GPU (no CPU fallback)")


def _need(t: torch.Tensor, dtype, name: str, contiguous_last=True):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    _require_gpu(t, name)
    if contiguous_last and t.stride(-1) != 1:
        raise ValueError(f"{name}: last dimension must be contiguous")


def gemm_nt(a, b, out, *, bias=None, residual=None, aux=None, a_rowmap=None, c_rowmap=None,
            tiles=None, tile_count=None, max_tiles=0, stride_b=0, stride_bias=0, alpha=1.0,
            epi=EPI_NONE, M=None, N=None, col_perm=False, tile_rows=128):
    """out[M,N] = epi(alpha * a[M,K] @ b[N,K]^T (+bias)) (+residual).  a, b bf16; out bf16/f32."""
    lib = load_library()
    _need(a, torch.bfloat16, "a"); _need(b, torch.bfloat16, "b")
    out_f32 = out.dtype == torch.float32
    if not out_f32:
        _need(out, torch.bfloat16, "out")
    K = a.shape[-1]
    if N is None:
        N = b.shape[-2]
    if b.shape[-1] != K:
        raise ValueError("gemm_nt: K mismatch")
    if M is None:
        M = out.shape[0]
    if (out.shape[-1] != N and not col_perm and c_rowmap is None) or out.shape[-1] < N:
        raise ValueError("gemm_nt: N mismatch")
    if a_rowmap is None and a.shape[0] < M:
        raise ValueError("gemm_nt: a has fewer rows than M")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    if residual is not None:
        _need(residual, torch.bfloat16, "residual")
    if aux is not None:
        _need(aux, torch.bfloat16, "aux")
    for t, nm in ((a_rowmap, "a_rowmap"), (c_rowmap, "c_rowmap"), (tiles, "tiles"), (tile_count, "tile_count")):
        if t is not None:
            _need(t, torch.int32, nm)
    fn = _nt_fn(tile_rows == 256)
    dp = lambda t: None if t is None else t.data_ptr()
    cargs = (a.data_ptr(), a.stride(-2), b.data_ptr(), b.stride(-2), out.data_ptr(), out.stride(-2), M, N, K, dp(bias), dp(residual),
             residual.stride(-2) if residual is not None else 0, dp(aux), aux.stride(-2) if aux is not None else 0, dp(a_rowmap), dp(c_rowmap),
             dp(tiles), dp(tile_count), max_tiles, stride_b, stride_bias, alpha, epi, 1 if out_f32 else 0, 1 if col_perm else 0)
    if PROFILE is None:
        rc = fn(*cargs, _stream_handle())
        if rc != 0:
            _chk(rc, "gemm_nt")
        return out
    nbytes = 2.0 * (M * K + N * K) + (4.0 if out_f32 else 2.0) * M * N * (1 + (aux is not None)) + 2.0 * M * N * (residual is not None)
    with _Timed(_nt_label, 2.0 * M * N * K, "flop", ("nt", M, N, K, epi, nbytes)):
        _chk(fn(*cargs, _stream_handle()), "gemm_nt")
    return out


_NT_FN = {}


def _nt_fn(tiles256: bool):
    f = _NT_FN.get(tiles256)
    if f is None:
        lib = load_library()
        f = lib.medmoe_gemm_nt_tiles256 if tiles256 else lib.medmoe_gemm_nt
        I, L, P = _c.c_int, _c.c_longlong, _vp
        f.argtypes = [P, I, P, I, P, I, I, I, I, P, P, I, P, I, P, P, P, P, I, L, L, _c.c_float, I, I, I, P]
        f.restype = I
        _NT_FN[tiles256] = f
    return f


def gemm_nt_rows(a, b, out, m_dev, *, bias=None, residual=None, aux=None, alpha=1.0, epi=EPI_NONE):
    """gemm_nt on the first *m_dev rows of `a` (m_dev: int32 device tensor of one element, 1 <= value <= a.shape[0]): packed variable-length
    batches without a device-to-host copy of the count.  Rows past the count are neither read for results nor written."""
    lib = load_library()
    _need(a, torch.bfloat16, "a"); _need(b, torch.bfloat16, "b"); _need(m_dev, torch.int32, "m_dev")
    out_f32 = out.dtype == torch.float32
    if not out_f32:
        _need(out, torch.bfloat16, "out")
    M, K, N = a.shape[0], a.shape[-1], b.shape[-2]
    if b.shape[-1] != K or out.shape[-1] != N or out.shape[0] < M:
        raise ValueError("gemm_nt_rows: shape mismatch")
    if bias is not None:
        _need(bias, torch.float32, "bias")
    # the row count lives on the device: the work is filled in by the caller's `rows_hint` (bench.py: the batch's token count) or left open
    with _Timed(_nt_label, 2.0 * ROWS_HINT * N * K if ROWS_HINT else None, "flop" if ROWS_HINT else None, ("nt_rows", M, N, K, epi)):
        rc = lib.medmoe_gemm_nt_rows(_ptr(a), _c.c_int(a.stride(-2)), _ptr(b), _c.c_int(b.stride(-2)), _ptr(out), _c.c_int(out.stride(-2)),
                                     _c.c_int(M), _c.c_int(N), _c.c_int(K), _ptr(bias), _ptr(residual),
                                     _c.c_int(residual.stride(-2) if residual is not None else 0), _ptr(aux),
                                     _c.c_int(aux.stride(-2) if aux is not None else 0), _c.c_float(alpha), _c.c_int(epi),
                                     _c.c_int(1 if out_f32 else 0), _ptr(m_dev), _stream())
        _chk(rc, "gemm_nt_rows")
    return out


ROWS_HINT = 0       # bench.py: the packed text tower's row count (known on the host there), so that gemm_nt_rows launches carry their flops


def current_stream_handle() -> int:
    """Raw handle of torch's current HIP stream on the current device."""
    return _stream_handle()


def stream_fork(src: int, dst: int):
    """Stream `dst` waits for everything enqueued on `src` so far (raw handles: torch.cuda.Stream.cuda_stream / current_stream_handle())."""
    f = _FN.get("stream_fork")
    if f is None:
        f = load_library().medmoe_stream_fork
        f.argtypes = [_vp, _vp]
        f.restype = _c.c_int
        _FN["stream_fork"] = f
    rc = f(src, dst)
    if rc != 0:
        _chk(rc, "stream_fork")


def set_option(key: int, value: int):
    """medmoe_set_option: kernel-selection switches (1 nt256, 2 nt512, 3 tn512, 4 grouped-wgrad rows, 5 max NT grid,
    6 scores512, 7 gemm_nt4w, 8 gemm_tn4w, 9 plain-wgrad rows per range, 10 grouped-wgrad rows per range on gemm_tn4w, 11 resident attention,
    12 score GEMM without its epilogue (measurement only), 13 scale_attn_bwd rows per wave, 15 attention threads per workgroup at 13 key tiles,
    16 LayerNorm one row per wave, 17 gemm_nt_direct for K % 64 == 32) - for tests and measurements; the defaults are the fastest measured.
    The NT GEMM switches: 1, 2, 7 and 17 take 0 / 1 (default 1), 5 takes the largest grid of the 256x256 kernels, 1 .. 256 (default 256)."""
    _chk(load_library().medmoe_set_option(_c.c_int(key), _c.c_int(value)), "set_option")


class DetScratch:
    """The scratch buffers of deterministic mode: one fp32 buffer per stream (launches on different streams may overlap), allocated on first
    use and grown on demand while that stream is current, so the allocator orders a buffer's reuse behind the launches that read it."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.bufs = {}

    def get(self, floats: int) -> torch.Tensor:
        key = _stream_handle() if self.device.type == "cuda" else 0
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < floats:
            self.bufs[key] = None                                   # release before allocating
            buf = self.bufs[key] = torch.empty(max(int(floats), 1024), device=self.device, dtype=torch.float32)
        return buf


def nondet_launches() -> int:
    """medmoe_nondet_launches: launches of this process so far that took an order-dependent form (atomic epilogues with several writers per
    element, atomic loss sums).  A step in deterministic mode leaves it unchanged."""
    f = _FN.get("nondet_launches")
    if f is None:
        f = load_library().medmoe_nondet_launches
        f.argtypes = []
        f.restype = _c.c_longlong
        _FN["nondet_launches"] = f
    return int(f())


def _ll_query(name: str, *ints) -> int:
    f = _FN.get(name)
    if f is None:
        f = getattr(load_library(), "medmoe_" + name)
        f.argtypes = [_c.c_longlong] * len(ints)
        f.restype = _c.c_longlong
        _FN[name] = f
    return int(f(*ints))


def lamb_chunk() -> int:
    """Elements per chunk of the LAMB moments launch: a segment leaves one record per chunk it touches (csrc/lamb_plan.h)."""
    return _ll_query("lamb_chunk")


def lamb_sum_shape():
    """(threads of a moments workgroup, threads of a ratios workgroup): with lamb_chunk() what the tests derive their summation bars from."""
    return _ll_query("lamb_threads"), _ll_query("lamb_ratio_threads")


def lamb_scratch_floats(n: int, n_segments: int) -> int:
    """fp32 elements of the record buffer the LAMB launches of an arena of n elements and n_segments segments need."""
    return _ll_query("lamb_scratch_floats", int(n), int(n_segments))


def lamb_coef_slot(n: int, n_segments: int) -> int:
    """Index into that buffer of the clip coefficient (grad_scale * min(1, clip / norm)) the moments launch leaves behind the records."""
    return _ll_query("lamb_coef_slot", int(n), int(n_segments))


def lamb_plan(seg_end: torch.Tensor, n: int) -> torch.Tensor:
    """seg_end: HOST int64 tensor of segment ends (ascending, last == n).  Returns the host int64 table of each segment's first record, by
    the enumeration the kernels use (csrc/lamb_plan.h through medmoe_lamb_plan)."""
    if seg_end.device.type != "cpu" or seg_end.dtype != torch.int64 or not seg_end.is_contiguous() or seg_end.dim() != 1:
        raise ValueError("lamb_plan: seg_end must be a contiguous host int64 vector")
    f = _FN.get("lamb_plan")
    if f is None:
        f = load_library().medmoe_lamb_plan
        f.argtypes = [_vp, _c.c_longlong, _c.c_longlong, _vp]
        f.restype = _c.c_longlong
        _FN["lamb_plan"] = f
    base = torch.zeros_like(seg_end)
    recs = int(f(seg_end.data_ptr(), seg_end.numel(), int(n), base.data_ptr()))
    if recs < 0:
        raise ValueError(f"lamb_plan: the segment table is not ascending or does not end at n = {n}")
    return base


def _scratch_query(name: str, *ints) -> int:
    f = _FN.get(name)
    if f is None:
        f = getattr(load_library(), "medmoe_" + name)
        f.argtypes = [_c.c_int] * len(ints)
        f.restype = _c.c_longlong
        _FN[name] = f
    return int(f(*ints))


def gemm_tn(g, x, dw, *, db=None, x_rowmap=None, g_rowmap=None, row_off=None, n_groups=1,
            stride_w=0, stride_db=0, nsplit=16, M=None, stream=None, scratch=None, det: Optional[DetScratch] = None):
    """dw[g][Nn,Kk] += g[M,Nn]^T @ x[M,Kk]; db[g][Nn] += colsum(g).  fp32 atomic accumulation.  stream: a raw stream handle to launch on
    instead of torch's current stream (the caller orders it: stream_fork).  scratch (fp32, plain operands only): medmoe_gemm_tn_staged -
    partial tiles stored there and summed by a second kernel instead of atomics on dw, when the shape allows; the caller must not hand the
    same scratch to launches that can overlap.  det (deterministic mode): medmoe_gemm_tn_det on the current stream with that stream's scratch -
    no order-dependent sum in dw or db, `nsplit` is not used."""
    lib = load_library()
    _need(g, torch.bfloat16, "g"); _need(x, torch.bfloat16, "x"); _need(dw, torch.float32, "dw")
    if M is None:
        M = g.shape[0]
    Nn, Kk = g.shape[-1], x.shape[-1]
    if dw.shape[-2] != Nn or dw.shape[-1] != Kk:
        raise ValueError("gemm_tn: dw shape mismatch")
    if db is not None:
        _need(db, torch.float32, "db")
    for t, nm in ((x_rowmap, "x_rowmap"), (g_rowmap, "g_rowmap"), (row_off, "row_off")):
        if t is not None:
            _need(t, torch.int32, nm)
    if det is not None:
        if stream is not None:
            raise ValueError("gemm_tn: deterministic launches run on the current stream (their scratch belongs to it)")
        fd = _TN_FN.get(2)
        if fd is None:
            fd = lib.medmoe_gemm_tn_det
            I, L, P = _c.c_int, _c.c_longlong, _vp
            fd.argtypes = [P, I, P, I, P, I, P, I, I, I, P, P, P, I, L, L, P, L, P]
            fd.restype = I
            _TN_FN[2] = fd
        need = _scratch_query("gemm_tn_det_scratch", M, Nn, Kk, int(x_rowmap is not None), int(g_rowmap is not None), int(row_off is not None), n_groups)
        sc = det.get(need)
        dp = lambda t: None if t is None else t.data_ptr()
        dargs = (g.data_ptr(), g.stride(-2), x.data_ptr(), x.stride(-2), dw.data_ptr(), dw.stride(-2), dp(db), M, Nn, Kk, dp(x_rowmap), dp(g_rowmap),
                 dp(row_off), n_groups, stride_w, stride_db, sc.data_ptr(), sc.numel())
        with _Timed("gemm_tn_det (wgrad, staged / single writer: gemm_tn4w_kernel + tn_reduce_det_kernel / gemm_tn_kernel)", 2.0 * M * Nn * Kk, "flop",
                    ("tn", M, Nn, Kk, n_groups)):
            _chk(fd(*dargs, _stream_handle()), "gemm_tn_det")
        return dw
    if scratch is not None and x_rowmap is None and g_rowmap is None and row_off is None and n_groups == 1:
        _need(scratch, torch.float32, "scratch")
        fs = _TN_FN.get(1)
        if fs is None:
            fs = lib.medmoe_gemm_tn_staged
            I, L, P = _c.c_int, _c.c_longlong, _vp
            fs.argtypes = [P, I, P, I, P, I, P, I, I, I, P, L, P]
            fs.restype = I
            _TN_FN[1] = fs
        sargs = (g.data_ptr(), g.stride(-2), x.data_ptr(), x.stride(-2), dw.data_ptr(), dw.stride(-2), None if db is None else db.data_ptr(),
                 M, Nn, Kk, scratch.data_ptr(), scratch.numel())
        if PROFILE is None or stream is not None:
            rc = fs(*sargs, _stream_handle() if stream is None else stream)
            if rc != 0:
                _chk(rc, "gemm_tn_staged")
            return dw
        with _Timed("gemm_tn (wgrad: gemm_tn4w_kernel / gemm_tn512_kernel / gemm_tn_kernel)", 2.0 * M * Nn * Kk, "flop", ("tn", M, Nn, Kk, n_groups)):
            _chk(fs(*sargs, _stream_handle()), "gemm_tn_staged")
        return dw
    fn = _TN_FN.get(0)
    if fn is None:
        fn = lib.medmoe_gemm_tn
        I, L, P = _c.c_int, _c.c_longlong, _vp
        fn.argtypes = [P, I, P, I, P, I, P, I, I, I, P, P, P, I, L, L, I, P]
        fn.restype = I
        _TN_FN[0] = fn
    dp = lambda t: None if t is None else t.data_ptr()
    cargs = (g.data_ptr(), g.stride(-2), x.data_ptr(), x.stride(-2), dw.data_ptr(), dw.stride(-2), dp(db), M, Nn, Kk, dp(x_rowmap), dp(g_rowmap),
             dp(row_off), n_groups, stride_w, stride_db, nsplit)
    if PROFILE is None or stream is not None:
        rc = fn(*cargs, _stream_handle() if stream is None else stream)
        if rc != 0:
            _chk(rc, "gemm_tn")
        return dw
    with _Timed("gemm_tn (wgrad: gemm_tn4w_kernel / gemm_tn512_kernel / gemm_tn_kernel)", 2.0 * M * Nn * Kk, "flop", ("tn", M, Nn, Kk, n_groups)):
        _chk(fn(*cargs, _stream_handle()), "gemm_tn")
    return dw


_TN_FN = {}


_LN_COL, _LN_ROW, _LN_X = "must hold D contiguous fp32 values", "must hold one contiguous fp32 value per row", "must be contiguous bf16 sized like x"


def _ln_bad(name, nm, what, t):
    if t.dtype != (torch.bfloat16 if what is _LN_X else torch.float32):
        raise TypeError(f"{name}: {nm} {what}, got {t.dtype}")
    raise ValueError(f"{name}: {nm} {what}, got {t.numel()} values{'' if t.is_contiguous() else ', not contiguous'}")


def _ln_check(name, rows, D, per_col, per_row, like_x=()):
    """What the LayerNorm kernels read and write without a bound of their own: per_col (gamma, beta, dgamma, dbeta) fp32, contiguous, D
    values; per_row (mean, rstd) fp32, contiguous, at least one value per row; like_x (add) bf16, contiguous, rows * D values.  Entries are
    (tensor, name); a tensor that is None stands for a null pointer the kernel accepts.  On the launch path: a few attribute reads each."""
    if D <= 0 or D % 8 or D > 2048:
        raise ValueError(f"{name}: D must be a multiple of 8 and <= 2048, got {D}")
    f32 = torch.float32
    for t, nm in per_col:
        if t is not None:
            if t.dtype is not f32 or t.numel() != D or not t.is_contiguous():
                _ln_bad(name, nm, _LN_COL, t)
            if not t.is_cuda:
                _require_gpu(t, nm)
    for t, nm in per_row:
        if t is not None:
            if t.dtype is not f32 or t.numel() < rows or not t.is_contiguous():
                _ln_bad(name, nm, _LN_ROW, t)
            if not t.is_cuda:
                _require_gpu(t, nm)
    for t, nm in like_x:
        if t is not None:
            if t.dtype is not torch.bfloat16 or t.numel() != rows * D or not t.is_contiguous():
                _ln_bad(name, nm, _LN_X, t)
            if not t.is_cuda:
                _require_gpu(t, nm)


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps):
    """mean / rstd may be None (the kernel then keeps the statistic to itself); y is bf16 or fp32."""
    lib = load_library()
    _need(x, torch.bfloat16, "x")
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    if not x.is_contiguous() or not y.is_contiguous() or y.numel() != x.numel():
        raise ValueError("layernorm_fwd: x/y must be contiguous and equally sized")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"layernorm_fwd: y must be bf16 or fp32, got {y.dtype}")
    _require_gpu(y, "y")
    _ln_check("layernorm_fwd", rows, D, ((gamma, "gamma"), (beta, "beta")), ((mean, "mean"), (rstd, "rstd")))
    if gamma is None or beta is None:
        raise ValueError("layernorm_fwd: gamma and beta are required")
    with _Timed("layernorm_fwd_kernel", 4.0 * rows * D, "byte"):
        rc = lib.medmoe_layernorm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd),
                                      _c.c_int(rows), _c.c_int(D), _c.c_float(eps),
                                      _c.c_int(1 if y.dtype == torch.float32 else 0), _stream())
        _chk(rc, "layernorm_fwd")
    return y


def layernorm_apply(x, mean, rstd, gamma, beta, y):
    """y = bf16((x - mean) * rstd * gamma + beta) from saved statistics: the y of the LayerNorm forward launch that wrote mean / rstd,
    bit for bit (medmoe_layernorm_apply; activation recomputation)."""
    for t, nm in ((x, "x"), (y, "y")):
        _need(t, torch.bfloat16, nm)
    for t, nm in ((mean, "mean"), (rstd, "rstd"), (gamma, "gamma"), (beta, "beta")):
        _need(t, torch.float32, nm)
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    if not x.is_contiguous() or not y.is_contiguous() or y.numel() != x.numel():
        raise ValueError("layernorm_apply: x / y must be contiguous and equally sized")
    if D % 8 or D > 2048:
        raise ValueError(f"layernorm_apply: D must be a multiple of 8 and <= 2048, got {D}")
    if gamma.numel() != D or beta.numel() != D or mean.numel() != rows or rstd.numel() != rows \
            or not all(t.is_contiguous() for t in (mean, rstd, gamma, beta)):
        raise ValueError("layernorm_apply: gamma / beta must hold D contiguous values, mean / rstd one per row")
    call("layernorm_apply", x, mean, rstd, gamma, beta, y, rows, D)
    return y


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dgamma=None, dbeta=None, add=None, det: Optional[DetScratch] = None, rows_dev=None):
    """det (deterministic mode): dgamma / dbeta leave as per-workgroup partial rows summed in workgroup order (medmoe_layernorm_bwd_det).
    rows_dev (int32 device tensor of one element): medmoe_layernorm_bwd_rows - the first min(rows, *rows_dev) rows only."""
    lib = load_library()
    for t, nm in ((dy, "dy"), (x, "x"), (dx, "dx")):
        _need(t, torch.bfloat16, nm)
        if not t.is_contiguous():
            raise ValueError(f"layernorm_bwd: {nm} must be contiguous")
    rows, D = x.numel() // x.shape[-1], x.shape[-1]
    if mean is None or rstd is None or gamma is None or (dgamma is None) != (dbeta is None):
        raise ValueError("layernorm_bwd: mean, rstd and gamma are required, dgamma and dbeta come together")
    _ln_check("layernorm_bwd", rows, D, ((gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")), ((mean, "mean"), (rstd, "rstd")),
              ((add, "add"),))
    if rows_dev is not None:
        if det is not None:
            raise ValueError("layernorm_bwd: no deterministic form with a device row count")
        _need(rows_dev, torch.int32, "rows_dev")
        call("layernorm_bwd_rows", dy, x, mean, rstd, gamma, add, dx, dgamma, dbeta, rows, D, rows_dev)
        return dx
    if det is not None and dgamma is not None:
        sc = det.get(_scratch_query("layernorm_bwd_det_scratch", D))
        with _Timed("layernorm_bwd_kernel + layernorm_bwd_reduce_kernel", (8.0 if add is not None else 6.0) * rows * D, "byte"):
            rc = lib.medmoe_layernorm_bwd_det(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(add), _ptr(dx),
                                              _ptr(dgamma), _ptr(dbeta), _c.c_int(rows), _c.c_int(D), _ptr(sc), _c.c_longlong(sc.numel()), _stream())
            _chk(rc, "layernorm_bwd_det")
        return dx
    with _Timed("layernorm_bwd_kernel", (8.0 if add is not None else 6.0) * rows * D, "byte"):
        rc = lib.medmoe_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(add), _ptr(dx),
                                      _ptr(dgamma), _ptr(dbeta), _c.c_int(rows), _c.c_int(D), _stream())
        _chk(rc, "layernorm_bwd")
    return dx


def attn_fwd(qkv, out, lse, key_mask, B, N, H):
    lib = load_library()
    _need(qkv, torch.bfloat16, "qkv"); _need(out, torch.bfloat16, "out"); _need(lse, torch.float32, "lse")
    D = H * 64
    if qkv.numel() != B * N * 3 * D or out.numel() != B * N * D or lse.numel() != B * H * N:
        raise ValueError("attn_fwd: buffer sizes do not match (B,N,H)")
    if key_mask is not None:
        _need(key_mask, torch.uint8, "key_mask")
        if key_mask.numel() != B * N:
            raise ValueError("attn_fwd: key_mask must be [B,N]")
    with _Timed("attn_fwd_kernel", 4.0 * N * N * 64 * B * H, "flop"):
        rc = lib.medmoe_attn_fwd(_ptr(qkv), _ptr(out), _ptr(lse), _ptr(key_mask), _c.c_int(B), _c.c_int(N),
                                 _c.c_int(H), _c.c_int(64), _stream())
        _chk(rc, "attn_fwd")
    return out


def attn_bwd(qkv, out, dout, lse, key_mask, dqkv, delta, B, N, H):
    lib = load_library()
    for t, nm in ((qkv, "qkv"), (out, "out"), (dout, "dout"), (dqkv, "dqkv")):
        _need(t, torch.bfloat16, nm)
    D = H * 64
    if qkv.numel() != B * N * 3 * D or dqkv.numel() != qkv.numel() or dout.numel() != B * N * D \
            or delta.numel() != B * H * N or lse.numel() != B * H * N:
        raise ValueError("attn_bwd: buffer sizes do not match (B,N,H)")
    with _Timed("attn_bwd (attn_bwd_dq_kernel + attn_bwd_dkv_kernel)", 10.0 * N * N * 64 * B * H, "flop"):
        rc = lib.medmoe_attn_bwd(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(key_mask), _ptr(dqkv), _ptr(delta),
                                 _c.c_int(B), _c.c_int(N), _c.c_int(H), _c.c_int(64), _stream())
        _chk(rc, "attn_bwd")
    return dqkv


def attn_bwd_varlen(qkv, out, dout, lse, seq_off, dqkv, delta, B, Nmax, H):
    """attn_bwd over a packed variable-length batch (attn_fwd_varlen's layout): qkv / dqkv [rows, 3D], out / dout [rows, D] hold the sequences
    back to back from row seq_off[b] on (rows >= seq_off[B]), lse / delta [B, H, Nmax]; Nmax <= 80."""
    for t, nm in ((qkv, "qkv"), (out, "out"), (dout, "dout"), (dqkv, "dqkv")):
        _need(t, torch.bfloat16, nm)
    _need(lse, torch.float32, "lse"); _need(delta, torch.float32, "delta"); _need(seq_off, torch.int32, "seq_off")
    D = H * 64
    if qkv.shape[-1] != 3 * D or dqkv.numel() != qkv.numel() or out.shape[-1] != D or dout.numel() != out.numel() \
            or out.numel() // D != qkv.numel() // (3 * D) or delta.numel() != B * H * Nmax or lse.numel() != B * H * Nmax or seq_off.numel() != B + 1:
        raise ValueError("attn_bwd_varlen: buffer sizes do not match (rows, B, Nmax, H)")
    call("attn_bwd_varlen", qkv, out, dout, lse, seq_off, dqkv, delta, B, Nmax, H, 64)
    return dqkv


# ---------------------------------------------------------------------------------------------
# dropout of the trainable text tower (csrc/dropout.hip): the mask is a function of (seed, step, site, element), see csrc/philox.h
# ---------------------------------------------------------------------------------------------
DROPOUT_SITE_EMBED = 0xFFFFFFFF      # the embedding LayerNorm's output; a layer's sites are 4 * layer + {0 attention probabilities, 1 after out_proj, 2 after FC2}


def dropout_thresh(p: float) -> int:
    """floor(p * 2^32): an element survives iff its 32-bit random word is >= this (p * 2^32 is exact in a double)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1), got {p}")
    return int(p * 4294967296.0)


def dropout_rng(seed: int, step: int, site: int, p: float):
    """The five by-value launch arguments every dropout kernel takes: (seed, step, site, thresh, scale = 1 / (1 - p))."""
    seed &= 0xFFFFFFFFFFFFFFFF
    if seed >= 1 << 63:
        seed -= 1 << 64              # the same 64 bits as a signed C long long
    return (seed, step & 0xFFFFFFFF, site & 0xFFFFFFFF, dropout_thresh(p), 1.0 / (1.0 - p))


def dropout_mask(out, rows, cols, cols_padded, rng):
    """out[rows, cols] uint8 = 1 where the element survives (tests / debugging: no product path stores a mask)."""
    _need(out, torch.uint8, "out")
    if out.numel() != rows * cols or not out.is_contiguous() or cols_padded % 4 or cols_padded < cols:
        raise ValueError("dropout_mask: out must be contiguous [rows, cols], cols_padded a multiple of 4 and >= cols")
    call("dropout_mask", out, rows, cols, cols_padded, *rng[:4])
    return out


def dropout_apply(x, y, rng):
    """y = keep * x / (1 - p) over the rows of a contiguous [rows, cols] bf16 / fp32 tensor (cols % 4 == 0); y may be x."""
    if x.dtype not in (torch.bfloat16, torch.float32) or y.dtype != x.dtype:
        raise TypeError("dropout_apply: x and y must both be bf16 or both fp32")
    _require_gpu(x, "dropout_apply"); _require_gpu(y, "dropout_apply")
    cols = x.shape[-1]
    if not x.is_contiguous() or not y.is_contiguous() or y.numel() != x.numel() or cols % 4:
        raise ValueError("dropout_apply: x / y must be contiguous, equally sized, with a last dimension that is a multiple of 4")
    call("dropout_apply", x, y, x.numel() // cols, cols, 1 if x.dtype == torch.float32 else 0, *rng)
    return y


def dropout_add_layernorm_fwd(z, residual, gamma, beta, x1, y, mean, rstd, eps, rng):
    """x1 = residual + keep * z / (1 - p); y = LayerNorm(x1); mean / rstd as layernorm_fwd leaves them (layernorm_bwd runs on x1)."""
    for t, nm in ((z, "z"), (residual, "residual"), (x1, "x1"), (y, "y")):
        _need(t, torch.bfloat16, nm)
        if not t.is_contiguous() or t.numel() != z.numel():
            raise ValueError(f"dropout_add_layernorm_fwd: {nm} must be contiguous and sized like z")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd")):
        _need(t, torch.float32, nm)
    D = z.shape[-1]
    rows = z.numel() // D
    if gamma.numel() != D or beta.numel() != D or mean.numel() < rows or rstd.numel() < rows:
        raise ValueError("dropout_add_layernorm_fwd: gamma / beta must hold D values, mean / rstd one per row")
    call("dropout_add_layernorm_fwd", z, residual, gamma, beta, x1, y, mean, rstd, rows, D, eps, *rng)
    return y


# stochastic depth of the image tower: site DROPOUT_SITE_VIT_DROP_PATH + 2 * layer + {0 attention branch, 1 feed-forward branch},
# one draw per sample - the keep bit of global sample g is element (0, g) of a one-row mask array
DROPOUT_SITE_VIT_DROP_PATH = 0x40000000
DROPOUT_SITE_AUGMENT = 0x20000000      # image augmentation: sample g owns the groups 4 g + {0, 1, 2} of this site
DROP_PATH_MAX_SITES = 128


def drop_path_scales(out, probs, B, sample0, seed, step, site0=DROPOUT_SITE_VIT_DROP_PATH):
    """out [len(probs), B] fp32 = 0 | fp32(1 / (1 - probs[s])): sample b survives at site s iff dropout_mask (one row, site site0 + s,
    dropout_thresh(probs[s])) keeps column sample0 + b.  The probabilities are host floats and travel by value: ONE launch, no read-back."""
    _need(out, torch.float32, "out")
    probs = [float(p) for p in probs]
    n = len(probs)
    if not 1 <= n <= DROP_PATH_MAX_SITES or B <= 0 or sample0 < 0 or out.numel() != n * B or not out.is_contiguous():
        raise ValueError(f"drop_path_scales: out must be contiguous [n_sites, B] with 1 <= n_sites <= {DROP_PATH_MAX_SITES}, sample0 >= 0")
    for p in probs:
        dropout_thresh(p)                                        # refuses a probability outside [0, 1)
    host = (_c.c_double * n)(*probs)
    seed = dropout_rng(seed, step, site0, 0.0)[0]
    fn = _fn("drop_path_scales")
    with _Timed("drop_path_scales_kernel", 4.0 * n * B, "byte"):
        _chk(fn(out.data_ptr(), _c.addressof(host), n, int(B), int(sample0), seed, step & 0xFFFFFFFF, site0 & 0xFFFFFFFF, _stream_handle()),
             "drop_path_scales")
    return out


def scale_add_layernorm_fwd(z, residual, scale, rows_per_sample, gamma, beta, x1, y, mean, rstd, eps):
    """x1 = bf16(residual + scale[row // rows_per_sample] * z); y = LayerNorm(x1); mean / rstd as layernorm_fwd leaves them.  A row whose
    scale is 0 copies residual (z is not read there).  D % 8 == 0, D <= 2048."""
    for t, nm in ((z, "z"), (residual, "residual"), (x1, "x1"), (y, "y")):
        _need(t, torch.bfloat16, nm)
        if not t.is_contiguous() or t.numel() != z.numel():
            raise ValueError(f"scale_add_layernorm_fwd: {nm} must be contiguous and sized like z")
    for t, nm in ((scale, "scale"), (gamma, "gamma"), (beta, "beta"), (mean, "mean"), (rstd, "rstd")):
        _need(t, torch.float32, nm)
    D = z.shape[-1]
    rows = z.numel() // D
    if D % 8 or D > 2048:
        raise ValueError(f"scale_add_layernorm_fwd: D must be a multiple of 8 and <= 2048, got {D}")
    if rows_per_sample <= 0 or rows % rows_per_sample or scale.numel() != rows // rows_per_sample or not scale.is_contiguous():
        raise ValueError(f"scale_add_layernorm_fwd: scale must hold one contiguous value per sample ({rows} rows / {rows_per_sample} per sample), "
                         f"got {scale.numel()}")
    if gamma.numel() != D or beta.numel() != D or mean.numel() < rows or rstd.numel() < rows:
        raise ValueError("scale_add_layernorm_fwd: gamma / beta must hold D values, mean / rstd one per row")
    call("scale_add_layernorm_fwd", z, residual, scale, rows_per_sample, gamma, beta, x1, y, mean, rstd, rows, D, eps)
    return y


def _attn_drop_check(name, qkv, out, lse, key_mask, B, N, H):
    _need(qkv, torch.bfloat16, "qkv"); _need(out, torch.bfloat16, "out"); _need(lse, torch.float32, "lse")
    D = H * 64
    if qkv.numel() != B * N * 3 * D or out.numel() != B * N * D or lse.numel() != B * H * N:
        raise ValueError(f"{name}: buffer sizes do not match (B,N,H)")
    if key_mask is not None:
        _need(key_mask, torch.uint8, "key_mask")
        if key_mask.numel() != B * N:
            raise ValueError(f"{name}: key_mask must be [B,N]")


def attn_drop_fwd(qkv, out, lse, key_mask, B, N, H, rng, head_dim=64):
    """attn_fwd for N <= 80 with dropout on the probabilities (lse: of the undropped softmax)."""
    _attn_drop_check("attn_drop_fwd", qkv, out, lse, key_mask, B, N, H)
    call("attn_drop_fwd", qkv, out, lse, key_mask, B, N, H, head_dim, *rng)
    return out


def attn_drop_bwd(qkv, out, dout, lse, key_mask, dqkv, delta, B, N, H, rng, head_dim=64):
    """attn_bwd for N <= 80 under the forward's dropout mask, regenerated from the same (seed, step, site): one kernel."""
    _attn_drop_check("attn_drop_bwd", qkv, out, lse, key_mask, B, N, H)
    _need(dout, torch.bfloat16, "dout"); _need(dqkv, torch.bfloat16, "dqkv"); _need(delta, torch.float32, "delta")
    if dqkv.numel() != qkv.numel() or dout.numel() != out.numel() or delta.numel() != lse.numel():
        raise ValueError("attn_drop_bwd: buffer sizes do not match (B,N,H)")
    call("attn_drop_bwd", qkv, out, dout, lse, key_mask, dqkv, delta, B, N, H, head_dim, *rng)
    return dqkv


# ---------------------------------------------------------------------------------------------
# LoRA adapters on the text tower's fused q / k / v projection (csrc/lora.hip; medmoe_amd/text_lora.py holds the arena)
# ---------------------------------------------------------------------------------------------
LORA_RANK_PAD = 16                   # adapters are stored at rank 16: pad rows of A / pad columns of B are zero and stay zero
LORA_TARGETS = ("query", "key", "value")
DROPOUT_SITE_LORA = 3                # + 4 * layer: the fourth site of a layer, one mask shared by the layer's targets
DROPOUT_SITE_VIT_LORA = 0x50000000   # + layer: the image tower's adapters, clear of every other site of csrc/philox.h
_NO_DROP = (0, 0, 0, 0, 1.0)


def lora_cols(targets, D: int):
    """Column offsets of the targets in a fused [q | k | v] row, padded to three launch arguments."""
    c = [LORA_TARGETS.index(t) * D for t in targets]
    return tuple(c + [0] * (3 - len(c)))


def _lora_check(name, M, D, n, u_like, **bf16):
    if not 1 <= n <= 3 or D % 64 or M <= 0:
        raise ValueError(f"{name}: 1..3 targets, D a multiple of 64, M > 0 (got n={n}, D={D}, M={M})")
    for nm, t in bf16.items():
        if t is not None:
            _need(t, torch.bfloat16, nm)
            if not t.is_contiguous():
                raise ValueError(f"{name}: {nm} must be contiguous")
    if u_like is not None and u_like.numel() != M * n * LORA_RANK_PAD:
        raise ValueError(f"{name}: U / dU must be [M, n * {LORA_RANK_PAD}]")


def _rows_dev(rows_dev):
    if rows_dev is not None:
        _need(rows_dev, torch.int32, "rows_dev")
    return rows_dev


def lora_fwd(x, A, Bw, U, qkv, targets, s, rng=None, rows_dev=None):
    """U = dropout(x) A^T (stored bf16 [M, n*16]); qkv[:, c_t : c_t + D] += s U_t B_t^T in place.  A [n*16, D], Bw [n*D, 16] bf16.
    rows_dev (here and in the two backward launches; int32 device tensor of one element): the *_rows entry point - the first
    min(M, *rows_dev) rows only."""
    M, D, n = x.shape[0], x.shape[1], len(targets)
    _lora_check("lora_fwd", M, D, n, U, x=x, A=A, Bw=Bw, U=U, qkv=qkv)
    if A.numel() != n * LORA_RANK_PAD * D or Bw.numel() != A.numel() or qkv.shape[0] != M or qkv.shape[-1] != 3 * D:
        raise ValueError("lora_fwd: A [n*16, D], Bw [n*D, 16], qkv [M, 3D]")
    a = (x, A, Bw, U, qkv, qkv.stride(-2), M, D, n, *lora_cols(targets, D), s, *(rng or _NO_DROP))
    if _rows_dev(rows_dev) is None:
        call("lora_fwd", *a)
    else:
        call("lora_fwd_rows", *a, rows_dev)
    return qkv


def lora_bwd_dx(dqkv, Bt, At, dU, dy, targets, s, rng=None, rows_dev=None):
    """dU_t = s dqkv_t B_t (stored bf16 [M, n*16]); dy [M, D] += dropout mask * (dU A) (dy None: skipped).  Bt [16, n*D], At [D, n*16] bf16."""
    M, D, n = dqkv.shape[0], dqkv.shape[-1] // 3, len(targets)
    _lora_check("lora_bwd_dx", M, D, n, dU, dqkv=dqkv, Bt=Bt, At=At, dU=dU, dy=dy)
    if Bt.numel() != n * LORA_RANK_PAD * D or At.numel() != Bt.numel() or dqkv.shape[-1] != 3 * D or (dy is not None and dy.numel() != M * D):
        raise ValueError("lora_bwd_dx: Bt [16, n*D], At [D, n*16], dqkv [M, 3D], dy [M, D]")
    a = (dqkv, dqkv.stride(-2), Bt, At, dU, dy, M, D, n, *lora_cols(targets, D), s, *(rng or _NO_DROP))
    if _rows_dev(rows_dev) is None:
        call("lora_bwd_dx", *a)
    else:
        call("lora_bwd_dx_rows", *a, rows_dev)
    return dU


def lora_wgrad_scratch(M: int, D: int, n: int) -> int:
    return _scratch_query("lora_wgrad_scratch", M, D, n)


def lora_bwd_wgrad(dqkv, x, U, dU, gA, gB, scratch, targets, s, rng=None, rows_dev=None):
    """gB [n*D, 16] += s dqkv_t^T U_t, gA [n*16, D] += dU_t^T dropout(x) (fp32): per-chunk partial sums in `scratch`, summed in a fixed order."""
    M, D, n = x.shape[0], x.shape[1], len(targets)
    _lora_check("lora_bwd_wgrad", M, D, n, U, dqkv=dqkv, x=x, U=U, dU=dU)
    for t, nm in ((gA, "gA"), (gB, "gB"), (scratch, "scratch")):
        _need(t, torch.float32, nm)
    if gA.numel() != n * LORA_RANK_PAD * D or gB.numel() != gA.numel() or dU.numel() != U.numel() or dqkv.shape[0] != M or dqkv.shape[-1] != 3 * D \
            or not gA.is_contiguous() or not gB.is_contiguous() or scratch.numel() < lora_wgrad_scratch(M, D, n):
        raise ValueError("lora_bwd_wgrad: gA [n*16, D], gB [n*D, 16] contiguous, dqkv [M, 3D], scratch of lora_wgrad_scratch(M, D, n) floats")
    a = (dqkv, dqkv.stride(-2), x, U, dU, gA, gB, scratch, scratch.numel(), M, D, n, *lora_cols(targets, D), s, *(rng or _NO_DROP))
    if _rows_dev(rows_dev) is None:
        call("lora_bwd_wgrad", *a)
    else:
        call("lora_bwd_wgrad_rows", *a, rows_dev)


def lora_wgrad_runs_scratch(M: int, D: int, n: int, run: int) -> int:
    return _scratch_query("lora_wgrad_runs_scratch", M, D, n, run)


def lora_bwd_wgrad_runs(dqkv, x, U, dU, gA, gB, scratch, targets, s, run, rng=None):
    """lora_bwd_wgrad at the image tower's row counts: a workgroup keeps accumulating over `run` consecutive 256-row chunks
    before it stores one partial; the partials are summed in run order.  run = 1: the bits of lora_bwd_wgrad."""
    M, D, n = x.shape[0], x.shape[1], len(targets)
    _lora_check("lora_bwd_wgrad_runs", M, D, n, U, dqkv=dqkv, x=x, U=U, dU=dU)
    for t, nm in ((gA, "gA"), (gB, "gB"), (scratch, "scratch")):
        _need(t, torch.float32, nm)
    if int(run) != run or run < 1:
        raise ValueError(f"lora_bwd_wgrad_runs: run must be an integer >= 1, got {run!r}")
    if gA.numel() != n * LORA_RANK_PAD * D or gB.numel() != gA.numel() or dU.numel() != U.numel() or dqkv.shape[0] != M or dqkv.shape[-1] != 3 * D \
            or not gA.is_contiguous() or not gB.is_contiguous() or scratch.numel() < lora_wgrad_runs_scratch(M, D, n, int(run)):
        raise ValueError("lora_bwd_wgrad_runs: gA [n*16, D], gB [n*D, 16] contiguous, dqkv [M, 3D], scratch of lora_wgrad_runs_scratch(M, D, n, run) "
                         "floats")
    call("lora_bwd_wgrad_runs", dqkv, dqkv.stride(-2), x, U, dU, gA, gB, scratch, scratch.numel(), M, D, n, *lora_cols(targets, D), int(run), s,
         *(rng or _NO_DROP))


def lora_merge(W, A, Bw, targets, s):
    """W [3D, D] bf16 (a COPY of the fused projection's weight): rows of target t = bf16(W + s B_t A_t)."""
    D, n = W.shape[1], len(targets)
    _lora_check("lora_merge", 1, D, n, None, W=W, A=A, Bw=Bw)
    if W.shape[0] != 3 * D or A.numel() != n * LORA_RANK_PAD * D or Bw.numel() != A.numel():
        raise ValueError("lora_merge: W [3D, D], A [n*16, D], Bw [n*D, 16]")
    call("lora_merge", W, W.stride(0), A, Bw, D, n, *lora_cols(targets, D), s)
    return W


# ---------------------------------------------------------------------------------------------
# generic caller for the remaining entry points: sig chars  p=pointer(tensor|None) i=int l=int64 u=unsigned f=float d=double
# ---------------------------------------------------------------------------------------------
_SIGS = {
    "patchify": "ppiiiiii", "patchify_ld": "ppiiiiiii", "init_tokens": "pppiii", "pos_cls_grad": "pppiii",
    "text_embed_ln": "ppppppppiiiif", "text_aggregate": "ppppippppiii",
    "mean_tokens": "ppiiiii", "broadcast_tokens": "ppiiiiif",
    "router_fwd": "pppppppppiiiii", "router_bwd": "pppppppfpppiiii", "router_eval": "pppii",
    "sgemm": "pppiiilllllff", "dispatch": "piiiiippppppip",
    "scale_attn_fwd": "pppppippiii", "combine_fwd": "ppppiiii",
    "scale_attn_bwd": "ppppppppppiipppppiii", "stage_grad_add": "pppiiiii",
    "ce_strided": "ppiilliffip", "soft_xent_strided": "pppiillffffip", "hardneg_strided": "ppiillffip", "rownorm": "ppii", "cos_scale": "pppiif", "cos_scale_bwd": "ppppppiif",
    "add_rowscaled": "pppii", "words_prep": "pppiiii", "unpad_cast": "ppiiii",
    "local_pair": "pppppppppppppiiiiifffi", "local_scores": "pppppiiiii", "local_pair2": "ppppppppppiiiifff", "scale_blocks": "pppiiii",
    "words_prep_ragged": "pppiiiippl", "local_scores_ragged": "pppppiiiiipiill",
    "local_pair2_ragged": "pppppppppiiiifffpiill", "scale_blocks_ragged": "pppiiipl",
    "local_pair3": "ppppppppppppliiiifffpiilllip", "local_pair3_wgrad": "ppppppppppppliiiifffpiilllipp", "local_scores_t": "pppppiiiiipiilll", "local_sim_fwd": "ppppppiiiiifffpii", "local_sim_pairs": "pppppppippiiiiifffi", "gemm_tn_cols": "pipipiiiiilllil", "gemm_tn_gram": "piplipiiiill",
    "local_gen_fwd_a": "pppiiiiiifl", "local_gen_cos": "pppppppiiiiiffl", "local_gen_dwctx": "ppppppppiiiiiffl",
    "local_gen_dwords": "pppppppppiiiiiffl",
    "local_gen_bwd_s": "ppppiiiiiifl", "unpad_cast2": "pppiiii",
    "quant_rows_e4m3": "pipppippii", "quant_weights_e4m3": "ppppiii", "gemm_fp8_grouped": "ppppppippppiiillli",
    "quant_rows_mx": "pipppii", "quant_weights_mx": "pppppiii", "gemm_mx_grouped": "ppppppippppppiiillli",
    "lerp_tokens_fwd": "ppiiii", "lerp_tokens_bwd": "pppiiii", "lerp_tokens_bwd2": "ppppiiii",
    "text_pack": "pppppii", "segment_map": "pippppiiii", "text_aggregate_bwd": "ppppiii", "text_embed_ln_bwd": "pppppppppppiiiif", "text_embed_ln_packed": "ppppppppiiiifpp", "text_aggregate_packed": "ppppipppppiii",
    "layernorm_fwd_rows": "ppppppiifip", "attn_fwd_varlen": "ppppiiii", "layernorm_apply": "ppppppii",
    "win_attn_fwd": "ppppiiiiii", "win_attn_bwd": "ppppppiiiiii", "patch_merge": "ppiiiii", "drop_path": "ppppil",
    "dropout_mask": "pliillll", "dropout_apply": "ppliillllf", "dropout_add_layernorm_fwd": "ppppppppiifllllf",
    "attn_drop_fwd": "ppppiiiillllf", "attn_drop_bwd": "pppppppiiiillllf",
    "drop_path_scales": "ppiillll", "scale_add_layernorm_fwd": "pppippppppiif",
    # image augmentation (csrc/augment.hip); the wrappers live in medmoe_amd/data.py.  mean3 / std3 of augment_apply are host arrays
    "augment_params": "pillliiiuffffffffff", "augment_apply": "pppiiiifpp",
    "gemm_tn_cols_det": "pipipiiiiilllilpl", "gemm_tn_gram_det": "piplipiiiill", "scale_attn_bwd_det": "ppppppppppiipppppiiipipl",
    "router_bwd_det": "pppppppfpppiiiip", "ce_strided_det": "ppiilliffipp", "soft_xent_strided_det": "pppiillffffipp", "hardneg_strided_det": "ppiillffipp",
    "cos_scale_bwd_det": "ppppppiif",
    "sumsq": "plp", "sumsq_det": "plpp", "adam_step": "pppppldddddipff", "adam_groups_step": "ppppplpppidddddiipff", "cast_bf16": "ppl", "transpose_many": "pppii",
    "lora_fwd": "pppppiiiiiiifllllf", "lora_bwd_dx": "pippppiiiiiifllllf", "lora_bwd_wgrad": "pippppppliiiiiifllllf",
    "lora_bwd_wgrad_runs": "pippppppliiiiiiifllllf", "lora_merge": "pippiiiiif",
    "attn_bwd_varlen": "pppppppiiii", "layernorm_bwd_rows": "pppppppppiip", "text_aggregate_bwd_packed": "ppppppiii",
    "text_embed_ln_bwd_packed": "pppppppppppiiiifpp",
    "lora_fwd_rows": "pppppiiiiiiifllllfp", "lora_bwd_dx_rows": "pippppiiiiiifllllfp", "lora_bwd_wgrad_rows": "pippppppliiiiiifllllfp",
    "grad_pack_bf16": "pplf", "sumsq_det_bf16": "plpp", "adam_step_g16": "pppppldddddipff", "adam_groups_step_g16": "ppppplpppidddddiipff",
    # the four optimiser steps with the weight EMA: their sibling's arguments + (ema, one_minus_decay)
    "adam_step_ema": "pppppldddddipffpf", "adam_groups_step_ema": "ppppplpppidddddiipffpf",
    "adam_step_ema_g16": "pppppldddddipffpf", "adam_groups_step_ema_g16": "ppppplpppidddddiipffpf",
    # LAMB (csrc/lamb.hip): three launches per arena - moments (fp32 / bf16 gradient), ratios, apply (plain / with the weight EMA)
    "lamb_moments": "pppplpppiplddddipff", "lamb_moments_g16": "pppplpppiplddddipff", "lamb_ratios": "plpppildiip",
    "lamb_apply": "pppplpppipdddddi", "lamb_apply_ema": "pppplpppipdddddipf",
    # retrieval and zero-shot evaluation (csrc/retrieval.hip)
    "l2_normalize": "ppiif", "sim_topk": "ppiiiipppl", "sim_rank": "pppiiippl",
    # supervised classification (csrc/classify.hip)
    "cls_head_logits": "ppppiii", "cls_head_step": "pppppiffpppppppliii", "auroc_counts": "pppii",
    # masked-language-model objective (csrc/mlm.hip)
    "mlm_mask": "ppppppppiiiiiiillll", "rows_gather": "ppppii", "rows_scatter_add": "ppppii", "rows_mul": "ppppii",
    "vocab_ce_fwd": "pppppfpppppliii", "vocab_ce_bwd_dx": "ppppppfpiii", "vocab_ce_bwd_dw": "ppppppfppiii",
    # semantic segmentation (csrc/segment.hip)
    "seg_head_fwd": "ppppiii", "seg_loss": "pppffffppppliiiii", "seg_head_bwd": "pppppppliii", "seg_predict": "pppiiiii",
    # phrase grounding (csrc/ground.hip)
    "ground_maps": "pppppiiiiiiiff", "ground_score": "pppppppiiiiii",
}


_CTYPES = {"p": _vp, "i": _c.c_int, "l": _c.c_longlong, "u": _c.c_uint, "d": _c.c_double, "f": _c.c_float}
_FN = {}


def _fn(name: str):
    """The library entry with its argument types declared once: ctypes then converts plain Python ints / floats itself."""
    f = _FN.get(name)
    if f is None:
        f = getattr(load_library(), "medmoe_" + name)
        f.argtypes = [_CTYPES[ch] for ch in _SIGS[name]] + [_vp]
        f.restype = _c.c_int
        _FN[name] = f
    return f


def call(name: str, *args):
    """Launch medmoe_<name> on the current stream.  Tensors must already be validated by the caller."""
    sig = _SIGS[name]
    if len(args) != len(sig):
        raise TypeError(f"medmoe_{name}: expected {len(sig)} arguments, got {len(args)}")
    cargs = []
    for ch, a in zip(sig, args):
        if ch == "p":
            if a is None:
                cargs.append(None)
            else:
                if not a.is_cuda:
                    _require_gpu(a, "medmoe_" + name)
                cargs.append(a.data_ptr())
        elif ch == "i" or ch == "l" or ch == "u":
            cargs.append(int(a))
        else:
            cargs.append(float(a))
    if PROFILE is None:
        rc = _fn(name)(*cargs, _stream_handle())
        if rc != 0:
            _chk(rc, name)
        return
    cost = _COSTS.get(name)
    label, work, unit = cost(args) if cost is not None else (name + "_kernel", None, None)
    with _Timed(label, work, unit):
        _chk(_fn(name)(*cargs, _stream_handle()), name)


def _cost_scores(a):        # (ctx, words, cap_lens, X, lse, B, Bc, P, T, Do, members, n_c, ntt, cbase, ld, bs): B*P region rows x n_c captions of 16*ntt words
    return "scores512_kernel<NTT, true> (score GEMM + word softmax)", 2.0 * a[5] * a[7] * a[11] * 16 * a[12] * a[9], "flop"


def _cost_pair3(a):         # (X, dS, AT, UT, lse, gm, wn, caps, gsim, sim, att, stats, srows, B, Bc, P, T, t1, t2, eps, members, n_c, ntt, cbase, ld, bs, HWq, d2)
    elems = float(a[13]) * a[26] * a[21] * 16 * a[22]           # (image, region column, caption word row) of the class
    if a[1] is None:
        return "local_pair3_kernel<196, NTT, false> (forward)", 4.0 * elems, "byte"      # reads log-probabilities, writes A
    return "local_pair3_kernel<196, NTT, true> (backward)", 6.0 * elems, "byte"          # reads lp + A, writes dS


def _cost_local_sim(a):     # (ctx, words, caps, gm, wn, sim, B, Bc, P, T, Do, t1, t2, eps, members, n_c, ntt)
    return "local_sim_fwd_kernel<196, NTT> (scores + pair stage, forward only)", 2.0 * a[6] * a[8] * a[15] * 16 * a[16] * a[10], "flop"


def _cost_local_pairs(a):   # (ctx, words, caps, gm, wn, out, units, n_units, pair_cap, pair_slot, B, Bc, P, T, Do, t1, t2, eps, ntt): work unknown here (the entry count is the tables')
    return "local_sim_fwd_kernel<196, NTT, PAIRS> (listed pairs)", None, None


def _cost_tn_cols(a):       # (g, ldg, x, ldx, dw, ldw, M, Nn, Kk, n_groups, ...)
    return "gemm_tn4w_kernel<false, COLG, false> (local-loss dC)", 2.0 * a[6] * a[7] * a[8] * max(1, a[9]), "flop"


def _cost_tn_gram(a):       # (AT, ld, d2, srows, 1, out, ldo, Kp, HWq, B, bs, ostride)
    return "gemm_tn4w_kernel<false, COLG, SCALE> (weighted Gram)", 2.0 * a[7] * a[8] * a[8] * a[9], "flop"


_COSTS = {
    "local_scores_t": _cost_scores, "local_pair3": _cost_pair3, "local_pair3_wgrad": _cost_pair3, "local_sim_fwd": _cost_local_sim, "local_sim_pairs": _cost_local_pairs, "gemm_tn_cols": _cost_tn_cols, "gemm_tn_gram": _cost_tn_gram,
    "gemm_tn_cols_det": _cost_tn_cols, "gemm_tn_gram_det": _cost_tn_gram,
    "adam_step": lambda a: ("adam_kernel", 34.0 * a[5], "byte"),                                   # p, g, m, v read; p, m, v, bf16 copy written
    "adam_groups_step": lambda a: ("adam_groups_kernel", 34.0 * a[5], "byte"),                     # the same traffic: the run table stays on chip
    "adam_step_g16": lambda a: ("adam_kernel<bf16>", 32.0 * a[5], "byte"),                           # the gradient read as bf16: 2 B/param less
    "adam_groups_step_g16": lambda a: ("adam_groups_kernel<LDS, bf16>", 32.0 * a[5], "byte"),
    "adam_step_ema": lambda a: ("adam_kernel<float, EMA>", 42.0 * a[5], "byte"),                  # + the average read and written
    "adam_groups_step_ema": lambda a: ("adam_groups_kernel<LDS, float, EMA>", 42.0 * a[5], "byte"),
    "adam_step_ema_g16": lambda a: ("adam_kernel<bf16, EMA>", 40.0 * a[5], "byte"),
    "adam_groups_step_ema_g16": lambda a: ("adam_groups_kernel<LDS, bf16, EMA>", 40.0 * a[5], "byte"),
    "lamb_moments": lambda a: ("lamb_moments_kernel", 24.0 * a[4], "byte"),                        # p, g, m, v read; m, v written
    "lamb_moments_g16": lambda a: ("lamb_moments_kernel<LDS, bf16>", 22.0 * a[4], "byte"),
    "lamb_apply": lambda a: ("lamb_apply_kernel", 18.0 * a[4], "byte"),                            # p, m, v read; p, bf16 copy written
    "lamb_apply_ema": lambda a: ("lamb_apply_kernel<LDS, EMA>", 26.0 * a[4], "byte"),
    "grad_pack_bf16": lambda a: ("grad_pack_bf16_kernel", 6.0 * a[2], "byte"),                     # fp32 read, bf16 written
    "scale_attn_bwd": lambda a: ("scale_attn_bwd_kernel", 2.0 * a[17] * (4 * (2 * a[18] + 2 * a[19]) + 2 * a[18]), "byte"),    # G, dG, H1, dH1 x 4 scales + eout, d_img_l rows
    "scale_attn_bwd_det": lambda a: ("scale_attn_bwd_kernel<DET> + scale_attn_bwd_reduce_kernel", 2.0 * a[17] * (4 * (2 * a[18] + 2 * a[19]) + 2 * a[18]), "byte"),
    "scale_attn_fwd": lambda a: ("scale_attn_fwd_kernel", 2.0 * a[8] * (4 * (a[9] + a[10]) + a[9]), "byte"),
    "dropout_add_layernorm_fwd": lambda a: ("dropout_add_layernorm_fwd_kernel", 8.0 * a[8] * a[9], "byte"),    # z, residual read; x1, y written
    "scale_add_layernorm_fwd": lambda a: ("scale_add_layernorm_fwd_kernel", 8.0 * a[10] * a[11], "byte"),       # z, residual read; x1, y written
    "attn_drop_fwd": lambda a: ("attn_drop_fwd_kernel", 4.0 * a[5] * a[5] * 64 * a[4] * a[6], "flop"),
    "attn_drop_bwd": lambda a: ("attn_drop_bwd_kernel", 10.0 * a[8] * a[8] * 64 * a[7] * a[9], "flop"),
    # the adapters' own algorithmic traffic (a = the launch arguments): X once, the targeted qkv / dqkv columns, U / dU, dy
    "lora_fwd": lambda a: ("lora_fwd_kernel", 2.0 * a[6] * (a[7] + 2 * a[8] * a[7] + a[8] * 16), "byte"),
    "lora_bwd_dx": lambda a: ("lora_bwd_dx_kernel", 2.0 * a[6] * (a[8] * a[7] + a[8] * 16 + (2 * a[7] if a[5] is not None else 0)), "byte"),
    "lora_bwd_wgrad": lambda a: ("lora_bwd_wgrad_kernel + lora_wgrad_reduce_kernel", 2.0 * a[9] * (a[11] * a[10] + a[10] + 2 * a[11] * 16), "byte"),
    "lora_bwd_wgrad_runs": lambda a: ("lora_bwd_wgrad_runs_kernel + lora_wgrad_reduce_kernel", 2.0 * a[9] * (a[11] * a[10] + a[10] + 2 * a[11] * 16), "byte"),
    "lora_fwd_rows": lambda a: ("lora_fwd_kernel (rows)", 2.0 * (ROWS_HINT or a[6]) * (a[7] + 2 * a[8] * a[7] + a[8] * 16), "byte"),
    "lora_bwd_dx_rows": lambda a: ("lora_bwd_dx_kernel (rows)", 2.0 * (ROWS_HINT or a[6]) * (a[8] * a[7] + a[8] * 16 + (2 * a[7] if a[5] is not None else 0)), "byte"),
    "lora_bwd_wgrad_rows": lambda a: ("lora_bwd_wgrad_kernel + lora_wgrad_reduce_kernel (rows)", 2.0 * (ROWS_HINT or a[9]) * (a[11] * a[10] + a[10] + 2 * a[11] * 16), "byte"),
    "layernorm_bwd_rows": lambda a: ("layernorm_bwd_kernel (rows)", (8.0 if a[5] is not None else 6.0) * (ROWS_HINT or a[9]) * a[10], "byte"),
    "attn_bwd_varlen": lambda a: ("attn_bwd_varlen (attn_bwd_dq_kernel + attn_bwd_dkv_kernel)", None, None),
    "layernorm_fwd_rows": lambda a: ("layernorm_fwd_kernel", 4.0 * (ROWS_HINT or a[6]) * a[7], "byte"),
    "layernorm_apply": lambda a: ("layernorm_apply_kernel", 4.0 * a[6] * a[7], "byte"),                         # x read, y written
    "l2_normalize": lambda a: ("l2_normalize_kernel", 12.0 * a[2] * a[3], "byte"),                              # x read twice, y written
    "sim_topk": lambda a: ("sim_stream_kernel<D / 64, TOPK> (+ topk_merge_kernel)", 2.0 * a[2] * a[3] * a[4], "flop"),
    "sim_rank": lambda a: ("sim_stream_kernel<D / 64, RANK> (+ rank_sum_kernel)", 2.0 * a[3] * a[4] * a[5], "flop"),
    "cls_head_logits": lambda a: ("cls_row_kernel<J4, -, false>", 4.0 * a[4] * (a[5] + a[6]), "byte"),                 # x read, z written
    # x read twice (rows, dW), dx written when asked for, z and dz written, dz read
    "cls_head_step": lambda a: ("cls_row_kernel<J4, TASK, true> + cls_wgrad_kernel (+ count, sums)",
                                4.0 * a[16] * ((3 if a[9] is not None else 2) * a[17] + 3 * a[18]), "byte"),
    "auroc_counts": lambda a: ("auroc_kernel", 2.0 * a[3] * a[3] * a[4], "flop"),                                        # at most N^2 C pairs, two compares each
}


def gemm_tn_cols(G, ldg, X, ldx, dW, ldw, M, Nn, Kk, n_groups, gcol_stride, xcol_stride, stride_w, g_chunk_w, g_chunk_stride,
                 det: Optional[DetScratch] = None):
    """medmoe_gemm_tn_cols; det (deterministic mode): medmoe_gemm_tn_cols_det with the current stream's scratch."""
    a = (G, ldg, X, ldx, dW, ldw, M, Nn, Kk, n_groups, gcol_stride, xcol_stride, stride_w, g_chunk_w, g_chunk_stride)
    if det is None:
        return call("gemm_tn_cols", *a)
    sc = det.get(_scratch_query("gemm_tn_cols_det_scratch", M, Nn, Kk, n_groups))
    call("gemm_tn_cols_det", *a, sc, sc.numel())


def gemm_tn_gram(*a, det: Optional[DetScratch] = None):
    """medmoe_gemm_tn_gram; det (deterministic mode): its single-writer form medmoe_gemm_tn_gram_det."""
    call("gemm_tn_gram" if det is None else "gemm_tn_gram_det", *a)


def local_fast_path(HW: int, T: int) -> bool:
    return bool(load_library().medmoe_local_fast_path(_c.c_int(HW), _c.c_int(T)))


def local_pair3_chunks(n: int):
    _chk(load_library().medmoe_local_pair3_chunks(_c.c_int(n)), "local_pair3_chunks")


def local_sim_chunks(n: int):
    _chk(load_library().medmoe_local_sim_chunks(_c.c_int(n)), "local_sim_chunks")


def local_pair3_supported(HW: int, T: int) -> bool:
    return bool(load_library().medmoe_local_pair3_supported(_c.c_int(HW), _c.c_int(T)))


def local_geometry(HW: int, T: int):
    lib = load_library()
    a, b, c = _c.c_int(0), _c.c_int(0), _c.c_int(0)
    rc = lib.medmoe_local_geometry(_c.c_int(HW), _c.c_int(T), _c.byref(a), _c.byref(b), _c.byref(c))
    _chk(rc, "local_geometry")
    return a.value, b.value, c.value


def local_sim_pairs(ctx, words, cap_lens, gm, wnorm, out, units, pair_cap, pair_slot, *, P: int, ntt: int, temp1: float, temp2: float,
                    cap_lens_host, eps: float = 1e-8):
    """medmoe_local_sim_pairs (csrc/local_eval.hip): out.view(-1)[pair_slot[e]] = the local similarity (before temp3) of image
    units[u][0] and caption pair_cap[e], for every entry e of every unit u = (image, first entry, entry count, 0).  ctx bf16 [B*P, D], words
    bf16 [Bc, T, D], cap_lens int32 [Bc] and wnorm fp32 [Bc, T] on the device, gm bf16 [B*GR, GR] as for local_sim_fwd; all captions listed
    are of length class ntt.  units / pair_cap / pair_slot and cap_lens_host are HOST tables (numpy or CPU tensors): the kernel trusts
    them, so every index is checked here, before anything is uploaded or launched - an index of -1 (sim_topk's padding) never reaches
    the device.  Slots no entry names keep their value.  Returns out."""
    import numpy as np
    name = "local_sim_pairs"
    _need(ctx, torch.bfloat16, "ctx"); _need(words, torch.bfloat16, "words"); _need(gm, torch.bfloat16, "gm")
    _need(cap_lens, torch.int32, "cap_lens"); _need(wnorm, torch.float32, "wnorm"); _need(out, torch.float32, "out")
    if words.dim() != 3 or ctx.dim() != 2 or not (ctx.is_contiguous() and words.is_contiguous() and gm.is_contiguous() and out.is_contiguous()
                                                   and wnorm.is_contiguous() and cap_lens.is_contiguous()):
        raise ValueError(f"{name}: ctx [B*P, D], words [Bc, T, D], gm, wnorm, cap_lens and out must be contiguous")
    Bc, T, D = words.shape
    P, ntt = int(P), int(ntt)
    if ctx.shape[1] != D or ctx.shape[0] % P or ctx.shape[0] == 0:
        raise ValueError(f"{name}: ctx must be [B*{P}, {D}], got {tuple(ctx.shape)}")
    B, GR = ctx.shape[0] // P, (P + 31) // 32 * 32
    if D % 64 or D < 64 or not 1 <= ntt <= 5 or not local_pair3_supported(P, 16 * ntt) or 16 * ntt > (T + 15) // 16 * 16:
        raise ValueError(f"{name}: {P} regions x length class {ntt} (T = {T}) at D = {D} has no kernel: 196 regions with classes 1..5 or 64 "
                         "regions with class 1, D a multiple of 64 (local_pair3_supported)")
    if gm.numel() != B * GR * GR or wnorm.numel() != Bc * T or cap_lens.numel() != Bc:
        raise ValueError(f"{name}: gm must hold [{B}*{GR}, {GR}], wnorm [{Bc}, {T}] and cap_lens [{Bc}] elements")
    tab = [np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).astype(np.int64) for t in (units, pair_cap, pair_slot)]
    units_h, cap_h, slot_h = tab[0].reshape(-1, 4), tab[1].reshape(-1), tab[2].reshape(-1)
    lens_h = np.asarray(cap_lens_host.cpu().numpy() if torch.is_tensor(cap_lens_host) else cap_lens_host, dtype=np.int64).reshape(-1)
    if lens_h.shape[0] != Bc:
        raise ValueError(f"{name}: cap_lens_host holds {lens_h.shape[0]} lengths, words {Bc} captions")
    if slot_h.shape[0] != cap_h.shape[0]:
        raise ValueError(f"{name}: pair_cap holds {cap_h.shape[0]} entries, pair_slot {slot_h.shape[0]}")
    n_units, n_e = units_h.shape[0], cap_h.shape[0]
    if n_units == 0:
        return out
    if units_h[:, 0].min() < 0 or units_h[:, 0].max() >= B:
        raise ValueError(f"{name}: a unit's image lies outside [0, {B})")
    if units_h[:, 1].min() < 0 or units_h[:, 2].min() < 0 or (units_h[:, 1] + units_h[:, 2]).max() > n_e:
        raise ValueError(f"{name}: a unit's entries lie outside the list of {n_e}")
    if n_e and (cap_h.min() < 0 or cap_h.max() >= Bc):
        raise ValueError(f"{name}: a pair_cap entry lies outside [0, {Bc}) (drop the -1 padding of sim_topk before building the list)")
    if n_e and (slot_h.min() < 0 or slot_h.max() >= out.numel()):
        raise ValueError(f"{name}: a pair_slot entry lies outside [0, {out.numel()})")
    if np.unique(slot_h).shape[0] != n_e:
        raise ValueError(f"{name}: pair_slot names a slot twice - every written slot has one owner")
    cls = (np.clip(lens_h[cap_h], 1, T) + 15) // 16
    if n_e and (cls != ntt).any():
        raise ValueError(f"{name}: a listed caption is not of length class {ntt} (16 (ntt - 1) < length <= 16 ntt)")
    meta = torch.from_numpy(np.concatenate((units_h.reshape(-1), cap_h, slot_h)).astype(np.int32)).to(ctx.device, non_blocking=True)
    call(name, ctx, words, cap_lens, gm, wnorm, out, meta[:4 * n_units], n_units, meta[4 * n_units:4 * n_units + n_e], meta[4 * n_units + n_e:],
         B, Bc, P, T, D, temp1, temp2, eps, ntt)
    return out


# ---------------------------------------------------------------------------------------------
# retrieval and zero-shot evaluation (csrc/retrieval.hip)
# ---------------------------------------------------------------------------------------------
SIM_TOPK_MAX = 16
L2_EPS = 1e-8                        # the clamp of medmoe_cos_scale


def sim_topk_splits(n: int):
    """Tests: force the number of key splits of sim_topk / sim_rank (0 = automatic).  The results do not depend on it."""
    _chk(load_library().medmoe_sim_topk_splits(_c.c_int(n)), "sim_topk_splits")


def l2_normalize(x, out=None, eps: float = L2_EPS):
    """out = x / max(|x|_2, eps) per row of a contiguous fp32 [rows, D] tensor; out may be x (in place), default a new tensor."""
    _need(x, torch.float32, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError("l2_normalize: x must be a contiguous [rows, D] tensor")
    if out is None:
        out = torch.empty_like(x)
    _need(out, torch.float32, "out")
    if out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
        raise ValueError("l2_normalize: out must be contiguous, shaped like x and on its device")
    call("l2_normalize", x, out, x.shape[0], x.shape[1], eps)
    return out


def _sim_check(name, q, keys):
    _need(q, torch.float32, "q"); _need(keys, torch.float32, "keys")
    if q.dim() != 2 or keys.dim() != 2 or not q.is_contiguous() or not keys.is_contiguous():
        raise ValueError(f"{name}: q and keys must be contiguous [rows, D] tensors")
    if q.shape[1] != keys.shape[1]:
        raise ValueError(f"{name}: q has D = {q.shape[1]}, keys D = {keys.shape[1]}")
    if q.shape[1] % 64 or q.shape[1] == 0:
        raise ValueError(f"{name}: D must be a multiple of 64, got {q.shape[1]}")
    if q.shape[0] == 0 or keys.shape[0] == 0:
        raise ValueError(f"{name}: q and keys must each hold at least one row")
    if q.device != keys.device:
        raise ValueError(f"{name}: q and keys must be on one device")
    return q.shape[0], keys.shape[0], q.shape[1]


def _sim_scratch(Nq, Nk, D, K, device):
    need = _scratch_query("sim_topk_scratch", Nq, Nk, D, K)
    return (torch.empty(need, device=device, dtype=torch.float32), need) if need else (None, 0)


def sim_topk(q, keys, K: int):
    """(val fp32 [Nq, K], idx int32 [Nq, K]): the K best rows of `keys` for every row of `q` by fp32 dot product, ordered (score descending,
    key index ascending); positions past min(K, Nk) hold -inf / -1.  The [Nq, Nk] matrix is never stored.  1 <= K <= 16, D % 64 == 0."""
    if int(K) != K or not 1 <= K <= SIM_TOPK_MAX:
        raise ValueError(f"sim_topk: K must be an integer in 1 .. {SIM_TOPK_MAX}, got {K!r}")
    Nq, Nk, D = _sim_check("sim_topk", q, keys)
    val = torch.empty(Nq, int(K), device=q.device, dtype=torch.float32)
    idx = torch.empty(Nq, int(K), device=q.device, dtype=torch.int32)
    sc, n = _sim_scratch(Nq, Nk, D, int(K), q.device)
    call("sim_topk", q, keys, Nq, Nk, D, int(K), val, idx, sc, n)
    return val, idx


def sim_rank(q, keys, target):
    """rank int32 [Nq]: the number of rows of `keys` ordered before keys[target[i]] for query i under sim_topk's order (0 = the target is the
    best key).  target: int32 [Nq] with values in [0, Nk) - the caller's contract, a value outside it is scored as a zero row."""
    Nq, Nk, D = _sim_check("sim_rank", q, keys)
    _need(target, torch.int32, "target")
    if target.dim() != 1 or target.numel() != Nq or not target.is_contiguous() or target.device != q.device:
        raise ValueError("sim_rank: target must be a contiguous int32 [Nq] tensor on q's device")
    rank = torch.empty(Nq, device=q.device, dtype=torch.int32)
    sc, n = _sim_scratch(Nq, Nk, D, 1, q.device)
    call("sim_rank", q, keys, target, Nq, Nk, D, rank, sc, n)
    return rank


# ---------------------------------------------------------------------------------------------
# supervised classification (csrc/classify.hip)
# ---------------------------------------------------------------------------------------------
CLS_TASKS = {"multiclass": 0, "multilabel": 1}
CLS_MAX_CLASSES = 64
CLS_MAX_D = 2048


def _cls_f32(name, arg, t, shape=None, align=False):
    """A contiguous fp32 tensor (of `shape`, 16-byte aligned when asked): ValueError naming the argument otherwise."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{name}: {arg} must be an fp32 tensor, got {getattr(t, 'dtype', type(t))}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {arg} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {arg} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if align and t.data_ptr() % 16:
        raise ValueError(f"{name}: {arg} must start at a 16-byte boundary")


def _cls_head_check(name, x, W, b):
    for arg, t in (("x", x), ("W", W), ("b", b)):
        _cls_f32(name, arg, t, align=arg != "b")
    if x.dim() != 2 or W.dim() != 2 or b.dim() != 1:
        raise ValueError(f"{name}: x must be [N, D], W [C, D] and b [C]")
    N, D = x.shape
    C = W.shape[0]
    if D % 64 or not 64 <= D <= CLS_MAX_D:
        raise ValueError(f"{name}: x has D = {D}; D must be a multiple of 64 in 64 .. {CLS_MAX_D}")
    if not 1 <= C <= CLS_MAX_CLASSES:
        raise ValueError(f"{name}: W has C = {C} rows; 1 <= C <= {CLS_MAX_CLASSES}")
    if W.shape[1] != D:
        raise ValueError(f"{name}: W has {W.shape[1]} columns, x has D = {D}")
    if b.shape[0] != C:
        raise ValueError(f"{name}: b holds {b.shape[0]} values, W has C = {C} rows")
    if N < 1:
        raise ValueError(f"{name}: x must hold at least one row")
    return N, D, C


def _cls_same_device(name, ref, **tensors):
    for arg, t in tensors.items():
        if t is not None:
            _require_gpu(t, f"{name}: {arg}")
            if t.device != ref.device:
                raise ValueError(f"{name}: {arg} is on {t.device}, x on {ref.device}")


def cls_head_scratch(N: int, D: int, C: int) -> int:
    return _scratch_query("cls_head_scratch", N, D, C)


def cls_head_logits(x, W, b, z=None):
    """z [N, C] = x [N, D] @ W [C, D]^T + b [C], all fp32 (medmoe_cls_head_logits): the evaluation form of the head."""
    N, D, C = _cls_head_check("cls_head_logits", x, W, b)
    if z is None:
        z = torch.empty((N, C), device=x.device, dtype=torch.float32)
    _cls_f32("cls_head_logits", "z", z, (N, C))
    _require_gpu(x, "cls_head_logits: x")
    _cls_same_device("cls_head_logits", x, W=W, b=b, z=z)
    call("cls_head_logits", x, W, b, z, N, D, C)
    return z


def cls_head_step(x, W, b, targets, dW, db, task: str = "multiclass", label_smoothing: float = 0.0, pos_weight=None, loss_scale: float = 1.0,
                  z=None, dx=None, loss=None, counts=None, scratch=None):
    """Forward, loss and backward of the linear head (medmoe_cls_head_step; the formulas are in include/medmoe_hip.h).
    targets: int32 [N] (multiclass, -1 = not counted) or int8 [N, C] in {0, 1, -1} (multilabel).  dW [C, D] and db [C] are ACCUMULATED into;
    dx [N, D], when given, is written.  Returns (z [N, C], loss fp32 [1], counts int32 [2] = (n_valid, n_correct)) - device tensors, nothing
    is read back.  z / loss / counts / scratch may be handed in to reuse buffers (scratch: cls_head_scratch(N, D, C) floats)."""
    name = "cls_head_step"
    N, D, C = _cls_head_check(name, x, W, b)
    if task not in CLS_TASKS:
        raise ValueError(f"{name}: task must be one of {sorted(CLS_TASKS)}, got {task!r}")
    want_dtype, want_shape = (torch.int32, (N,)) if task == "multiclass" else (torch.int8, (N, C))
    if not isinstance(targets, torch.Tensor) or targets.dtype != want_dtype:
        raise ValueError(f"{name}: targets must be {want_dtype} for task {task!r}, got {getattr(targets, 'dtype', type(targets))}")
    if tuple(targets.shape) != want_shape or not targets.is_contiguous():
        raise ValueError(f"{name}: targets must be contiguous with shape {want_shape}, got {tuple(targets.shape)}")
    if targets.data_ptr() % 16:
        raise ValueError(f"{name}: targets must start at a 16-byte boundary")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"{name}: label_smoothing must be in [0, 1), got {label_smoothing}")
    if task == "multilabel" and float(label_smoothing) != 0.0:
        raise ValueError(f"{name}: label_smoothing is defined for the multiclass task only")
    if pos_weight is not None:
        if task != "multilabel":
            raise ValueError(f"{name}: pos_weight is defined for the multilabel task only")
        _cls_f32(name, "pos_weight", pos_weight, (C,))
    _cls_f32(name, "dW", dW, (C, D))
    _cls_f32(name, "db", db, (C,))
    if dx is not None:
        _cls_f32(name, "dx", dx, (N, D), align=True)
    _require_gpu(x, f"{name}: x")
    dev = x.device
    if z is None:
        z = torch.empty((N, C), device=dev, dtype=torch.float32)
    if loss is None:
        loss = torch.empty(1, device=dev, dtype=torch.float32)
    if counts is None:
        counts = torch.empty(2, device=dev, dtype=torch.int32)
    need = cls_head_scratch(N, D, C)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.float32)
    _cls_f32(name, "z", z, (N, C))
    _cls_f32(name, "loss", loss, (1,))
    _cls_f32(name, "scratch", scratch, align=True)
    if scratch.numel() < need:
        raise ValueError(f"{name}: scratch holds {scratch.numel()} floats, cls_head_scratch({N}, {D}, {C}) = {need}")
    if counts.dtype != torch.int32 or counts.numel() != 2 or not counts.is_contiguous():
        raise ValueError(f"{name}: counts must be a contiguous int32 tensor of 2 elements")
    _cls_same_device(name, x, W=W, b=b, targets=targets, pos_weight=pos_weight, dW=dW, db=db, dx=dx, z=z, loss=loss, counts=counts, scratch=scratch)
    call(name, x, W, b, targets, pos_weight, CLS_TASKS[task], float(label_smoothing), float(loss_scale), z, dx, dW, db, loss, counts, scratch,
         scratch.numel(), N, D, C)
    return z, loss, counts


def auroc_counts(scores, targets):
    """int64 [C, 4] = (n_pos, n_neg, n_less, n_equal) per class (medmoe_auroc_counts): scores fp32 [N, C] (finite), targets int8 [N, C] in
    {0, 1, -1}; n_less / n_equal count the (positive i, negative j) pairs with s_j < s_i / s_j == s_i.  Exact integers, no [N, N] matrix."""
    name = "auroc_counts"
    _cls_f32(name, "scores", scores)
    if scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError(f"{name}: scores must be [N, C] with N >= 1 and C >= 1, got {tuple(scores.shape)}")
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int8:
        raise ValueError(f"{name}: targets must be int8, got {getattr(targets, 'dtype', type(targets))}")
    if tuple(targets.shape) != tuple(scores.shape) or not targets.is_contiguous():
        raise ValueError(f"{name}: targets must be contiguous and shaped like scores {tuple(scores.shape)}, got {tuple(targets.shape)}")
    N, C = scores.shape
    if C > 65535:
        raise ValueError(f"{name}: at most 65535 classes, got {C}")
    _require_gpu(scores, f"{name}: scores")
    _cls_same_device(name, scores, targets=targets)
    out = torch.empty((C, 4), device=scores.device, dtype=torch.int64)
    call(name, scores, targets, out, N, C)
    return out


# ---------------------------------------------------------------------------------------------
# semantic segmentation on the region features (csrc/segment.hip)
# ---------------------------------------------------------------------------------------------
SEG_MAX_CLASSES = 8
SEG_MAX_D = 2048
SEG_MAX_GRID = 64                       # patches per axis


def _seg_tensor(name, arg, t, dtype, shape=None, align=False):
    """A contiguous tensor of `dtype` (of `shape`, 16-byte aligned when asked): ValueError naming the argument otherwise."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name}: {arg} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {arg} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {arg} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if align and t.data_ptr() % 16:
        raise ValueError(f"{name}: {arg} must start at a 16-byte boundary")


def _seg_head_check(name, feat, W, b=None):
    _seg_tensor(name, "feat", feat, torch.bfloat16, align=True)
    _seg_tensor(name, "W", W, torch.float32, align=True)
    if b is not None:
        _seg_tensor(name, "b", b, torch.float32)
    if feat.dim() != 2 or W.dim() != 2 or (b is not None and b.dim() != 1):
        raise ValueError(f"{name}: feat must be [N, D], W [C, D] and b [C]")
    N, D = feat.shape
    C = W.shape[0]
    if D % 64 or not 64 <= D <= SEG_MAX_D:
        raise ValueError(f"{name}: feat has D = {D}; D must be a multiple of 64 in 64 .. {SEG_MAX_D}")
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: W has C = {C} rows; 1 <= C <= {SEG_MAX_CLASSES}")
    if W.shape[1] != D:
        raise ValueError(f"{name}: W has {W.shape[1]} columns, feat has D = {D}")
    if b is not None and b.shape[0] != C:
        raise ValueError(f"{name}: b holds {b.shape[0]} values, W has C = {C} rows")
    if N < 1:
        raise ValueError(f"{name}: feat must hold at least one row")
    return N, D, C


def _seg_map_check(name, z, size):
    """(B, g, H, W, C) of patch logits z fp32 [B, g*g, C] against the mask size (H, W)."""
    _seg_tensor(name, "z", z, torch.float32)
    if z.dim() != 3 or z.shape[0] < 1:
        raise ValueError(f"{name}: z must be [B, P, C] with B >= 1, got {tuple(z.shape)}")
    B, P, C = z.shape
    g = int(round(P ** 0.5))
    if g * g != P or not 1 <= g <= SEG_MAX_GRID:
        raise ValueError(f"{name}: z has P = {P} patches; P must be a square g * g with 1 <= g <= {SEG_MAX_GRID}")
    if not 1 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: z has C = {C} classes; 1 <= C <= {SEG_MAX_CLASSES}")
    H, W = int(size[0]), int(size[1])
    if H < g:
        raise ValueError(f"{name}: H = {H} is smaller than the patch grid g = {g}; the head upsamples only")
    if W < g:
        raise ValueError(f"{name}: W = {W} is smaller than the patch grid g = {g}; the head upsamples only")
    return B, g, H, W, C


def _seg_same_device(name, ref, **tensors):
    _require_gpu(ref, name)
    for arg, t in tensors.items():
        if t is not None:
            _require_gpu(t, f"{name}: {arg}")
            if t.device != ref.device:
                raise ValueError(f"{name}: {arg} is on {t.device}, the first argument on {ref.device}")


def seg_scratch(B: int, g: int, H: int, W: int, D: int, C: int) -> int:
    return _scratch_query("seg_scratch", B, g, H, W, D, C)


def seg_head_bwd_scratch(N: int, D: int, C: int) -> int:
    return _scratch_query("seg_head_bwd_scratch", N, D, C)


def seg_head_fwd(feat, W, b, z=None):
    """z fp32 [N, C] = feat bf16 [N, D] @ W fp32 [C, D]^T + b [C] in fp32 arithmetic (medmoe_seg_head_fwd): the patch logits."""
    name = "seg_head_fwd"
    N, D, C = _seg_head_check(name, feat, W, b)
    if z is None:
        z = torch.empty((N, C), device=feat.device, dtype=torch.float32)
    _seg_tensor(name, "z", z, torch.float32)
    if z.numel() != N * C:
        raise ValueError(f"{name}: z must hold {N} x {C} values, got {tuple(z.shape)}")
    _seg_same_device(name, feat, W=W, b=b, z=z)
    call(name, feat, W, b, z, N, D, C)
    return z


def seg_loss(z, masks, *, pos_weight=None, w_bce: float = 1.0, w_dice: float = 1.0, dice_eps: float = 1.0, loss_scale: float = 1.0, dz=None,
             loss=None, counts=None, scratch=None):
    """BCE + batch-Dice loss of the patch logits z fp32 [B, g*g, C] against masks int8 [B, C, H, W] in {0, 1, -1} (medmoe_seg_loss; the
    formulas are in include/medmoe_hip.h).  dz [B, g*g, C], when given, is WRITTEN with d loss / d z.  Returns (loss fp32 [1], counts int64
    [C, 4] = (n_valid, TP, FP, FN)) - device tensors, nothing is read back."""
    name = "seg_loss"
    _seg_tensor(name, "masks", masks, torch.int8, align=True)
    if masks.dim() != 4:
        raise ValueError(f"{name}: masks must be [B, C, H, W], got {tuple(masks.shape)}")
    B, g, H, W, C = _seg_map_check(name, z, masks.shape[2:])
    if tuple(masks.shape[:2]) != (B, C):
        raise ValueError(f"{name}: masks must have shape ({B}, {C}, H, W) for z {tuple(z.shape)}, got {tuple(masks.shape)}")
    if pos_weight is not None:
        _seg_tensor(name, "pos_weight", pos_weight, torch.float32, (C,))
    if not float(dice_eps) >= 0.0:
        raise ValueError(f"{name}: dice_eps must be >= 0, got {dice_eps}")
    dev = z.device
    if dz is not None:
        _seg_tensor(name, "dz", dz, torch.float32, tuple(z.shape))
    if loss is None:
        loss = torch.empty(1, device=dev, dtype=torch.float32)
    if counts is None:
        counts = torch.empty((C, 4), device=dev, dtype=torch.int64)
    need = seg_scratch(B, g, H, W, 64, C)
    if scratch is None:
        scratch = torch.empty(need, device=dev, dtype=torch.float32)
    _seg_tensor(name, "loss", loss, torch.float32, (1,))
    _seg_tensor(name, "counts", counts, torch.int64, (C, 4))
    _seg_tensor(name, "scratch", scratch, torch.float32, align=True)
    if scratch.numel() < need:
        raise ValueError(f"{name}: scratch holds {scratch.numel()} floats, seg_scratch({B}, {g}, {H}, {W}, 64, {C}) = {need}")
    _seg_same_device(name, z, masks=masks, pos_weight=pos_weight, dz=dz, loss=loss, counts=counts, scratch=scratch)
    call(name, z, masks, pos_weight, float(w_bce), float(w_dice), float(dice_eps), float(loss_scale), dz, loss, counts, scratch, scratch.numel(),
         B, g, H, W, C)
    return loss, counts


def seg_head_bwd(dz, feat, W, dW, db, dfeat=None, scratch=None):
    """The head's backward (medmoe_seg_head_bwd): dfeat bf16 [N, D] = dz W, when given, is WRITTEN; dW [C, D] and db [C] are ACCUMULATED into
    (records per row range, added in range order)."""
    name = "seg_head_bwd"
    N, D, C = _seg_head_check(name, feat, W)
    _seg_tensor(name, "dz", dz, torch.float32)
    if dz.numel() != N * C:
        raise ValueError(f"{name}: dz must hold {N} x {C} values, got {tuple(dz.shape)}")
    _seg_tensor(name, "dW", dW, torch.float32, (C, D))
    _seg_tensor(name, "db", db, torch.float32, (C,))
    if dfeat is not None:
        _seg_tensor(name, "dfeat", dfeat, torch.bfloat16, align=True)
        if dfeat.numel() != N * D:
            raise ValueError(f"{name}: dfeat must hold {N} x {D} values, got {tuple(dfeat.shape)}")
    need = seg_head_bwd_scratch(N, D, C)
    if scratch is None:
        scratch = torch.empty(need, device=feat.device, dtype=torch.float32)
    _seg_tensor(name, "scratch", scratch, torch.float32, align=True)
    if scratch.numel() < need:
        raise ValueError(f"{name}: scratch holds {scratch.numel()} floats, seg_head_bwd_scratch({N}, {D}, {C}) = {need}")
    _seg_same_device(name, feat, dz=dz, W=W, dW=dW, db=db, dfeat=dfeat, scratch=scratch)
    call(name, dz, feat, W, dfeat, dW, db, scratch, scratch.numel(), N, D, C)


def seg_predict(z, size, masks=None, want_logits: bool = False):
    """masks uint8 [B, C, H, W] = (zf > 0) of the patch logits z fp32 [B, g*g, C] upsampled to size = (H, W) (medmoe_seg_predict); with
    want_logits also zf fp32 [B, C, H, W].  Returns masks, or (masks, zf)."""
    name = "seg_predict"
    B, g, H, W, C = _seg_map_check(name, z, size)
    if masks is None:
        masks = torch.empty((B, C, H, W), device=z.device, dtype=torch.uint8)
    _seg_tensor(name, "masks", masks, torch.uint8, (B, C, H, W), align=True)
    zf = torch.empty((B, C, H, W), device=z.device, dtype=torch.float32) if want_logits else None
    _seg_same_device(name, z, masks=masks)
    call(name, z, masks, zf, B, g, H, W, C)
    return (masks, zf) if want_logits else masks


# ---------------------------------------------------------------------------------------------
# phrase grounding: word-region heat maps scored against boxes (csrc/ground.hip)
# ---------------------------------------------------------------------------------------------
GROUND_MAX_GRID = 32                    # regions per axis
GROUND_MAX_T = 80                       # word rows of a caption
GROUND_MAX_D = 2048
GROUND_MAX_TEMP1 = 64.0                 # exp(temp1 (s - 1)) runs without a running maximum
GROUND_MAX_BOXES = 8
GROUND_MAX_THETAS = 4
GROUND_MODES = {"attention": 0, "cosine": 1}


def _ground_host_table(name, arg, t, cols):
    """An integer table as a host int64 array [n, *cols] (tensor on any device, numpy array or nested list)."""
    import numpy as np
    if isinstance(t, torch.Tensor):
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"{name}: {arg} must be an integer table, got {t.dtype}")
        t = t.detach().cpu().numpy()
    a = np.asarray(t)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{name}: {arg} must be an integer table, got {a.dtype}")
    try:
        return np.ascontiguousarray(a.astype(np.int64).reshape((-1,) + tuple(cols)))
    except ValueError:
        raise ValueError(f"{name}: {arg} must be [n, {', '.join(str(c) for c in cols)}], got {tuple(a.shape)}") from None


def ground_maps(ctx, words, cap_lens, entries, mode: str = "attention", temp1: float = 4.0, eps: float = 1e-8, cap_lens_host=None):
    """h fp32 [n, P]: the heat map over the P = g * g regions of image b for the words [word_lo, word_hi) of caption i, for every entry
    (b, i, word_lo, word_hi) of `entries` (medmoe_ground_maps).  ctx bf16 [B, P, D], words bf16 [Bc, T, D] and cap_lens int32 [Bc] as
    Engine.embed leaves them in the workspace; word positions are the rows of `words`.  mode "attention": the region attention of the
    local loss (softmax over the caption's words, then softmax over the regions at temp1), averaged over the span - each map sums to 1;
    "cosine": cos(ctx_p, sum of the span's word vectors).  `entries` is a HOST table (tensor, numpy array or list): the kernel trusts
    it, so every image, caption and span is checked here against cap_lens (cap_lens_host, when given, spares the read-back) before anything
    is uploaded or launched.  n = 0 returns an empty map without a launch."""
    import numpy as np
    name = "ground_maps"
    _seg_tensor(name, "ctx", ctx, torch.bfloat16, align=True)
    _seg_tensor(name, "words", words, torch.bfloat16, align=True)
    _seg_tensor(name, "cap_lens", cap_lens, torch.int32)
    if ctx.dim() != 3 or words.dim() != 3 or ctx.shape[0] < 1 or words.shape[0] < 1:
        raise ValueError(f"{name}: ctx must be [B, P, D] and words [Bc, T, D], got {tuple(ctx.shape)} and {tuple(words.shape)}")
    B, P, D = ctx.shape
    Bc, T, Dw = words.shape
    g = int(round(P ** 0.5))
    if g * g != P or not 1 <= g <= GROUND_MAX_GRID:
        raise ValueError(f"{name}: ctx has P = {P} regions; P must be a square g * g with 1 <= g <= {GROUND_MAX_GRID}")
    if D % 64 or not 64 <= D <= GROUND_MAX_D:
        raise ValueError(f"{name}: ctx has D = {D}; D must be a multiple of 64 in 64 .. {GROUND_MAX_D}")
    if Dw != D:
        raise ValueError(f"{name}: words has D = {Dw}, ctx has D = {D}")
    if not 1 <= T <= GROUND_MAX_T:
        raise ValueError(f"{name}: words has T = {T} rows per caption; 1 <= T <= {GROUND_MAX_T}")
    if cap_lens.numel() != Bc:
        raise ValueError(f"{name}: cap_lens holds {cap_lens.numel()} lengths, words {Bc} captions")
    if mode not in GROUND_MODES:
        raise ValueError(f"{name}: mode must be one of {sorted(GROUND_MODES)}, got {mode!r}")
    if not 0.0 <= float(temp1) <= GROUND_MAX_TEMP1:
        raise ValueError(f"{name}: temp1 = {temp1} lies outside [0, {GROUND_MAX_TEMP1:g}] (the region softmax runs without a running maximum)")
    if not float(eps) >= 0.0:
        raise ValueError(f"{name}: eps must be >= 0, got {eps}")
    tab = _ground_host_table(name, "entries", entries, (4,))
    n = tab.shape[0]
    if n:
        lens_h = _ground_host_table(name, "cap_lens_host", cap_lens if cap_lens_host is None else cap_lens_host, ())
        if lens_h.shape[0] != Bc:
            raise ValueError(f"{name}: cap_lens_host holds {lens_h.shape[0]} lengths, words {Bc} captions")
        if tab[:, 0].min() < 0 or tab[:, 0].max() >= B:
            raise ValueError(f"{name}: entries names an image outside [0, {B})")
        if tab[:, 1].min() < 0 or tab[:, 1].max() >= Bc:
            raise ValueError(f"{name}: entries names a caption outside [0, {Bc})")
        lens_e = lens_h[tab[:, 1]]
        if lens_e.min() < 1 or lens_e.max() > T:
            raise ValueError(f"{name}: cap_lens of a listed caption lies outside [1, {T}]")
        bad = (tab[:, 2] < 0) | (tab[:, 2] >= tab[:, 3]) | (tab[:, 3] > lens_e)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f"{name}: entries[{k}] has the word span [{tab[k, 2]}, {tab[k, 3]}); a span must satisfy 0 <= word_lo < word_hi <= "
                             f"cap_lens[{tab[k, 1]}] = {lens_e[k]}")
    _seg_same_device(name, ctx, words=words, cap_lens=cap_lens)
    h = torch.empty((n, P), device=ctx.device, dtype=torch.float32)
    if n == 0:
        return h
    ent = torch.from_numpy(tab.astype(np.int32)).to(ctx.device, non_blocking=True)
    call(name, ctx, words, cap_lens, ent, h, n, B, Bc, P, T, D, GROUND_MODES[mode], float(temp1), float(eps))
    return h


def ground_score(h, boxes, size, thetas=(), want_map: bool = False):
    """Scores grid maps h fp32 [n, g * g] (any map) against boxes int [n, NB, 4] = (x0, y0, x1, y1), half-open pixel rectangles of the
    size = (H, W) frame, 1 <= NB <= 8; a rectangle with x1 <= x0 or y1 <= y0 is absent; boxes are clipped to the frame here
    (medmoe_ground_score).  hf is the bilinear upsample of h to (H, W), the map of seg_loss, recomputed per pixel.  Returns a dict of device
    tensors: rec_f fp32 [n, 2 + NTH] = (max, min, thr_k = min + theta_k (max - min)), rec_i int32 [n, 4 + 2 NTH] = (y, x, hit, area, inter_0,
    pred_0, ...) with (y, x) the first maximal pixel in row-major order, rec_d fp64 [n, 4] = the sums of hf and hf^2 over the union of the
    boxes and over the frame, "size" and "thetas"; with want_map also "hf" fp32 [n, H, W], bit for bit the values the records saw."""
    name = "ground_score"
    _seg_tensor(name, "h", h, torch.float32)
    if h.dim() != 2:
        raise ValueError(f"{name}: h must be [n, P], got {tuple(h.shape)}")
    n, P = h.shape
    g = int(round(P ** 0.5))
    if g * g != P or not 1 <= g <= GROUND_MAX_GRID:
        raise ValueError(f"{name}: h has P = {P} regions; P must be a square g * g with 1 <= g <= {GROUND_MAX_GRID}")
    if not isinstance(boxes, torch.Tensor) or boxes.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: boxes must be an int32 or int64 tensor, got {getattr(boxes, 'dtype', type(boxes))}")
    if boxes.dim() != 3 or boxes.shape[0] != n or boxes.shape[2] != 4:
        raise ValueError(f"{name}: boxes must be [{n}, NB, 4], got {tuple(boxes.shape)}")
    NB = boxes.shape[1]
    if not 1 <= NB <= GROUND_MAX_BOXES:
        raise ValueError(f"{name}: boxes has NB = {NB} rectangles per entry; 1 <= NB <= {GROUND_MAX_BOXES}")
    th = [float(t) for t in thetas]
    if len(th) > GROUND_MAX_THETAS:
        raise ValueError(f"{name}: thetas holds NTH = {len(th)} thresholds; 0 <= NTH <= {GROUND_MAX_THETAS}")
    H, W = int(size[0]), int(size[1])
    if H < g:
        raise ValueError(f"{name}: H = {H} is smaller than the region grid g = {g}; the map is upsampled only")
    if W < g:
        raise ValueError(f"{name}: W = {W} is smaller than the region grid g = {g}; the map is upsampled only")
    if H * W > 1 << 30:
        raise ValueError(f"{name}: size = ({H}, {W}) holds more than 2^30 pixels")
    _require_gpu(h, name)
    dev = h.device
    hi = torch.tensor([W, H, W, H], dtype=torch.int64)
    bx = torch.minimum(boxes.detach().cpu().to(torch.int64).clamp(min=0), hi).to(torch.int32).contiguous().to(dev, non_blocking=True)
    NTH = len(th)
    theta = torch.tensor(th, dtype=torch.float32).to(dev, non_blocking=True) if NTH else None
    out = {"rec_f": torch.empty((n, 2 + NTH), device=dev, dtype=torch.float32), "rec_i": torch.empty((n, 4 + 2 * NTH), device=dev, dtype=torch.int32),
           "rec_d": torch.empty((n, 4), device=dev, dtype=torch.float64), "size": (H, W), "thetas": tuple(th)}
    hf = torch.empty((n, H, W), device=dev, dtype=torch.float32) if want_map else None
    if n:
        call(name, h, bx, theta, hf, out["rec_f"], out["rec_i"], out["rec_d"], n, g, H, W, NB, NTH)
    if want_map:
        out["hf"] = hf
    return out


# ---------------------------------------------------------------------------------------------
# masked-language-model objective of the text tower (csrc/mlm.hip)
# ---------------------------------------------------------------------------------------------
DROPOUT_SITE_MLM = 0x60000000          # token t of global sample g owns the group g * T + t of this site (csrc/philox.h)
VOCAB_CE_MAX_D = 1024
VOCAB_CE_TILE = 256                    # vocabulary entries per forward tile: a row leaves ceil(V / 256) (max, sum) pairs


def _mlm_int32(name, arg, t, numel=None):
    _need(t, torch.int32, f"{name}: {arg}")
    if not t.is_contiguous() or (numel is not None and t.numel() < numel):
        raise ValueError(f"{name}: {arg} must be contiguous" + (f" and hold at least {numel} elements" if numel is not None else ""))


def mlm_mask(ids, attn, *, cls_id: int, sep_id: int, pad_id: int, mask_id: int, vocab: int, seed: int, step: int, p: float,
             sample_offset: int = 0, tok_row=None, out=None):
    """The step's MLM mask (medmoe_mlm_mask; the rule is in include/medmoe_hip.h).  ids int32 [B, T], attn uint8 [B, T]; tok_row (int32
    [B * T], text_pack) makes `rows` name packed rows.  Returns (ids_masked [B, T], labels [B, T], rows [B * T], row_labels [B * T],
    count [1]) - device tensors, nothing is read back; `out` may hand the same five in to reuse buffers."""
    name = "mlm_mask"
    _need(ids, torch.int32, f"{name}: ids"); _need(attn, torch.uint8, f"{name}: attn")
    if ids.dim() != 2 or tuple(attn.shape) != tuple(ids.shape) or not ids.is_contiguous() or not attn.is_contiguous():
        raise ValueError(f"{name}: ids and attn must be contiguous [B, T] tensors of one shape")
    B, T = ids.shape
    if B < 1 or T < 1 or B * T >= 1 << 31:
        raise ValueError(f"{name}: B * T must be in 1 .. 2^31 - 1")
    if not 0.0 < float(p) < 1.0:
        raise ValueError(f"{name}: p must be in (0, 1), got {p}")
    if vocab < 2 or not 0 <= mask_id < vocab:
        raise ValueError(f"{name}: mask_id must be in [0, vocab = {vocab}), got {mask_id}")
    if sample_offset < 0:
        raise ValueError(f"{name}: sample_offset must be >= 0")
    if tok_row is not None:
        _mlm_int32(name, "tok_row", tok_row, B * T)
    dev = ids.device
    if out is None:
        out = (torch.empty_like(ids), torch.empty_like(ids), torch.empty(B * T, device=dev, dtype=torch.int32),
               torch.empty(B * T, device=dev, dtype=torch.int32), torch.empty(1, device=dev, dtype=torch.int32))
    ids_masked, labels, rows, row_labels, count = out
    for arg, t, n in (("ids_masked", ids_masked, B * T), ("labels", labels, B * T), ("rows", rows, B * T), ("row_labels", row_labels, B * T),
                      ("count", count, 1)):
        _mlm_int32(name, arg, t, n)
    rng = dropout_rng(seed, step, DROPOUT_SITE_MLM, float(p))
    call(name, ids, attn, tok_row, ids_masked, labels, rows, row_labels, count, B, T, vocab, cls_id, sep_id, pad_id, mask_id, sample_offset,
         rng[0], rng[1], rng[3])
    return ids_masked, labels, rows, row_labels, count


def _rows_check(name, count, M_bound, D, **bf16):
    for arg, t in bf16.items():
        _need(t, torch.bfloat16, f"{name}: {arg}")
        if not t.is_contiguous() or t.shape[-1] != D or t.data_ptr() % 16:
            raise ValueError(f"{name}: {arg} must be contiguous [rows, {D}] and 16-byte aligned")
    _mlm_int32(name, "count", count, 1)
    if D % 8 or M_bound < 1:
        raise ValueError(f"{name}: D must be a multiple of 8 and M_bound >= 1")


def rows_gather(src, rows, count, dst):
    """dst[k] = src[rows[k]] for k < min(count, dst.shape[0]) (bf16 rows; count and rows live on the device)."""
    M_bound, D = dst.shape
    _rows_check("rows_gather", count, M_bound, D, src=src, dst=dst)
    _mlm_int32("rows_gather", "rows", rows, M_bound)
    call("rows_gather", src, rows, count, dst, M_bound, D)
    return dst


def rows_scatter_add(src, rows, count, dst):
    """dst[rows[k]] += src[k] for k < min(count, src.shape[0]); the listed rows are distinct (one writer each)."""
    M_bound, D = src.shape
    _rows_check("rows_scatter_add", count, M_bound, D, src=src, dst=dst)
    _mlm_int32("rows_scatter_add", "rows", rows, M_bound)
    call("rows_scatter_add", src, rows, count, dst, M_bound, D)
    return dst


def rows_mul(a, b, count, dst):
    """dst[k] = a[k] * b[k] for k < count, 0 for the rows from count to dst.shape[0]."""
    M_bound, D = dst.shape
    _rows_check("rows_mul", count, M_bound, D, a=a, b=b, dst=dst)
    if a.shape[0] < M_bound or b.shape[0] < M_bound:
        raise ValueError("rows_mul: a and b must hold at least dst.shape[0] rows")
    call("rows_mul", a, b, count, dst, M_bound, D)
    return dst


def vocab_ce_scratch(M_bound: int, V: int, D: int) -> int:
    return _scratch_query("vocab_ce_scratch", M_bound, V, D)


def _vocab_ce_check(name, z, E, bias, row_labels, count):
    _need(z, torch.bfloat16, f"{name}: z"); _need(E, torch.bfloat16, f"{name}: E"); _need(bias, torch.float32, f"{name}: bias")
    if z.dim() != 2 or E.dim() != 2 or not z.is_contiguous() or not E.is_contiguous() or not bias.is_contiguous():
        raise ValueError(f"{name}: z must be a contiguous [M_bound, D], E a contiguous [V, D] and bias a contiguous [V]")
    M_bound, D = z.shape
    V = E.shape[0]
    if D % 64 or not 64 <= D <= VOCAB_CE_MAX_D:
        raise ValueError(f"{name}: z has D = {D}; D must be a multiple of 64 in 64 .. {VOCAB_CE_MAX_D}")
    if E.shape[1] != D:
        raise ValueError(f"{name}: E has {E.shape[1]} columns, z has D = {D}")
    if V < 2 or bias.numel() != V:
        raise ValueError(f"{name}: V = {V} must be >= 2 and bias must hold V values, got {bias.numel()}")
    if M_bound < 1:
        raise ValueError(f"{name}: z must hold at least one row")
    if z.data_ptr() % 16 or E.data_ptr() % 16:
        raise ValueError(f"{name}: z and E must start at a 16-byte boundary")
    _mlm_int32(name, "row_labels", row_labels, M_bound)
    _mlm_int32(name, "count", count, 1)
    return M_bound, V, D


def _vocab_ce_f32(name, arg, t, numel):
    _need(t, torch.float32, f"{name}: {arg}")
    if not t.is_contiguous() or t.numel() < numel:
        raise ValueError(f"{name}: {arg} must be contiguous and hold at least {numel} floats")


def vocab_ce_fwd(z, E, bias, row_labels, count, loss_scale: float = 1.0, lse=None, terms=None, loss=None, counts=None, scratch=None):
    """Decoder + cross-entropy in one pass (medmoe_vocab_ce_fwd): logits = z [M_bound, D] @ E [V, D]^T + bias are never stored.  The first
    `count` (int32 device tensor) rows of z are live.  Returns (loss fp32 [1] = loss_scale * mean over the live rows of lse - logit[target],
    counts int32 [2] = (live rows, rows whose target is the arg max), lse fp32 [M_bound], terms fp32 [M_bound])."""
    name = "vocab_ce_fwd"
    M_bound, V, D = _vocab_ce_check(name, z, E, bias, row_labels, count)
    dev = z.device
    lse = torch.empty(M_bound, device=dev, dtype=torch.float32) if lse is None else lse
    terms = torch.empty(M_bound, device=dev, dtype=torch.float32) if terms is None else terms
    loss = torch.empty(1, device=dev, dtype=torch.float32) if loss is None else loss
    counts = torch.empty(2, device=dev, dtype=torch.int32) if counts is None else counts
    need = vocab_ce_scratch(M_bound, V, D)
    scratch = torch.empty(need, device=dev, dtype=torch.float32) if scratch is None else scratch
    _vocab_ce_f32(name, "lse", lse, M_bound); _vocab_ce_f32(name, "terms", terms, M_bound); _vocab_ce_f32(name, "loss", loss, 1)
    _vocab_ce_f32(name, "scratch", scratch, need)
    _mlm_int32(name, "counts", counts, 2)
    call(name, z, E, bias, row_labels, count, float(loss_scale), lse, terms, loss, counts, scratch, scratch.numel(), M_bound, V, D)
    return loss, counts, lse, terms


def vocab_ce_bwd(z, E, bias, row_labels, lse, count, loss_scale: float = 1.0, dz=None, dE=None, dbias=None):
    """Backward of vocab_ce_fwd from its lse (medmoe_vocab_ce_bwd_dx / _dw): dz (bf16 [M_bound, D]) is WRITTEN on the live rows when given;
    dE (fp32 [V, D]) and dbias (fp32 [V]) are ACCUMULATED into when given (both or neither).  No atomics, nothing of size [M, V]."""
    name = "vocab_ce_bwd"
    M_bound, V, D = _vocab_ce_check(name, z, E, bias, row_labels, count)
    _vocab_ce_f32(name, "lse", lse, M_bound)
    if dz is None and dE is None:
        raise ValueError(f"{name}: nothing to compute (dz and dE are both None)")
    if (dE is None) != (dbias is None):
        raise ValueError(f"{name}: dE and dbias come together")
    if dz is not None:
        _need(dz, torch.bfloat16, f"{name}: dz")
        if tuple(dz.shape) != (M_bound, D) or not dz.is_contiguous():
            raise ValueError(f"{name}: dz must be a contiguous [{M_bound}, {D}]")
        call("vocab_ce_bwd_dx", z, E, bias, row_labels, lse, count, float(loss_scale), dz, M_bound, V, D)
    if dE is not None:
        _vocab_ce_f32(name, "dE", dE, V * D); _vocab_ce_f32(name, "dbias", dbias, V)
        if tuple(dE.shape) != (V, D):
            raise ValueError(f"{name}: dE must be [{V}, {D}]")
        call("vocab_ce_bwd_dw", z, E, bias, row_labels, lse, count, float(loss_scale), dE, dbias, M_bound, V, D)
    return dz, dE, dbias
