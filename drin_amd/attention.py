"""A multi-head attention that trains on the HIP library: `attention_core` (the softmax-attention core between the in- and
out-projections, forward `drin_attention_dropout_fwd`, backward `drin_attention_dropout_bwd`) and `MultiheadAttention`, a drop-in
`nn.MultiheadAttention` (torch's parameters, state-dict keys and initial draw) whose projections run through
`drin_linear_fwd` / `drin_linear_bwd`.  This is the block GHMFC runs four times per forward (`baselines/ghmfc.py:96-110`);
`drin_amd.ghmfc.Model` itself still scores only; `drin_amd.ghmfc_train.TrainableModel` trains.  `core="mfma"` moves the core
onto the matrix pipes in split-bf16 arithmetic (`drin_attention_mfma_fwd` / `_bwd`).  Attention dropout in training
mode is an opt-in: a `DropoutStream` handed to the module selects the library's own counter-based mask
(`drin_attention_dropout_fwd` / `_bwd`).  What the kernels compute and what is left: DESIGN.md sections 16, 18 and 11.

GPU only: there is no CPU fallback and no torch math between the module's input and its output.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
from torch import nn

from . import _lib
from ._lib import _ptr, _scratch, _stream

PRECISIONS = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
MAX_KEYS, MAX_HEAD_DIM = 512, 256          # check_attention_shape of the library
CORES = ("fma", "mfma")                    # the softmax-attention core: fp32 FMA (the default) | split-bf16 MFMA (attention_core)
ORDERED_DW_SCRATCH = 28                    # drin_linear_bwd: scratch floats per weight element of the ordered dW reduction


def _check_core(core: str) -> str:
    if core not in CORES:
        raise ValueError(f"core {core!r} not in {list(CORES)}")
    return core


def _require_gpu_f32(name: str, t: torch.Tensor) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"drin_amd.attention runs on the GPU only (no CPU fallback): {name} is on {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"drin_amd.attention takes float32 operands: {name} is {t.dtype}")


def _row_stride(t: torch.Tensor, width: int) -> Optional[int]:
    """Row stride of a [B, L, >= width] view read as B L rows, or None when it is not one (the caller copies)."""
    B, L = t.shape[0], t.shape[1]
    if t.stride(2) != 1 and t.shape[2] > 1:
        return None
    ld = t.stride(1) if L > 1 else (t.stride(0) if B > 1 else max(width, t.shape[2]))
    if ld < width or (B > 1 and L > 1 and t.stride(0) != L * ld):
        return None
    return ld


def _as_rows(t: torch.Tensor, width: int) -> Tuple[torch.Tensor, int]:
    ld = _row_stride(t, width)
    if ld is None:
        t = t.contiguous()
        ld = t.shape[2]
    return t, ld


# ---- dropout --------------------------------------------------------------------------------------------
class DropoutStream:
    """The numbering of the library's attention-dropout draws: a `seed` that keys the generator and a counter that gives every
    forward its own `call` number (csrc/dropout_mask.h: the mask is a pure function of seed, call and element index, not
    torch's random stream).  Modules that share one stream draw distinct masks.  `log` keeps (call, B, H, Lq, Lk) of the most
    recent draws, which is what `drin_attention_dropout_keep` needs to regenerate a mask on the host; setting `counter` back
    reproduces the draws from there."""
    LOG_LENGTH = 64

    def __init__(self, seed: int = 0):
        self.seed = int(seed) & (2 ** 64 - 1)
        self.counter = 0
        self.log = []

    def draw(self, B: int, H: int, Lq: int, Lk: int) -> int:
        call = self.counter
        self.counter += 1
        self.log.append((call, B, H, Lq, Lk))
        del self.log[:-self.LOG_LENGTH]
        return call

    def draw_rows(self, rows: int, width: int) -> int:
        """The draw of a row dropout (`row_ops.act_dropout`) over [rows, width]: the mask of geometry (rows, 1, 1, width)."""
        return self.draw(rows, 1, 1, width)


def dropout_keep(seed: int, call: int, B: int, H: int, Lq: int, Lk: int, p: float) -> torch.Tensor:
    """The keep mask of one draw, bool [B, H, Lq, Lk] on the CPU, from the library's host function (no GPU)."""
    keep = torch.empty(B, H, Lq, Lk, dtype=torch.uint8)
    _lib.check(_lib.load().drin_attention_dropout_keep(seed, call, B, H, Lq, Lk, p, C.c_void_p(keep.data_ptr())))
    return keep.bool()


# ---- the core ---------------------------------------------------------------------------------------------
class _CoreCall:
    """One forward (+ backward) of the core through the library: geometry, operands with their row strides and the mask; the
    forward's (out, lse) are the autograd node's saved tensors.  `packed`: k is a [B, Lk, 2 E] buffer K | V and the gradient comes
    back the same way.  `core`: "fma" (drin_attention_dropout_fwd / _bwd) or "mfma" (drin_attention_mfma_fwd / _bwd).  `drop`:
    (p, seed, call) of the draw, or None, which goes as p = 0: the library's plain path, the undropped entry points' bits."""

    def __init__(self, q: torch.Tensor, k: torch.Tensor, v: Optional[torch.Tensor], key_mask: Optional[torch.Tensor], num_heads: int,
                 drop: Optional[Tuple[float, int, int]] = None, core: str = "fma"):
        lib = _lib.load()
        self.fwd, self.bwd = {"fma": (lib.drin_attention_dropout_fwd, lib.drin_attention_dropout_bwd),
                              "mfma": (lib.drin_attention_mfma_fwd, lib.drin_attention_mfma_bwd)}[_check_core(core)]
        self.drop = drop or (0.0, 0, 0)
        self.packed = v is None
        for name, t in (("q", q), ("k", k)) + (() if self.packed else (("v", v),)):
            _require_gpu_f32(name, t)
            if t.dim() != 3:
                raise RuntimeError(f"attention_core: {name} must be [batch, length, width], got {tuple(t.shape)}")
        B, Lq, E = q.shape
        Lk = k.shape[1]
        if E % num_heads or k.shape[0] != B or k.shape[2] != (2 * E if self.packed else E) or (
                not self.packed and tuple(v.shape) != tuple(k.shape)):
            raise RuntimeError(f"attention_core: q {tuple(q.shape)}, k {tuple(k.shape)}, v {None if v is None else tuple(v.shape)} "
                               f"do not fit {num_heads} heads")
        self.device = q.device
        self.B, self.H, self.Lq, self.Lk, self.E, self.dh = B, num_heads, Lq, Lk, E, E // num_heads
        self.q, self.ldq = _as_rows(q, E)
        if self.packed:
            self.kv, self.ldk = _as_rows(k, 2 * E)
            self.k, self.v, self.ldv = self.kv, self.kv[..., E:], self.ldk
        else:
            (self.k, self.ldk), (self.v, self.ldv) = _as_rows(k, E), _as_rows(v, E)
        if key_mask is not None:
            if tuple(key_mask.shape) != (B, Lk):
                raise RuntimeError(f"attention_core: key_mask {tuple(key_mask.shape)} is not [batch, k_len] = {(B, Lk)}")
            key_mask = key_mask.to(self.device, torch.int64).contiguous()
        self.mask = key_mask

    def _geometry(self):
        return self.B, self.H, self.Lq, self.Lk, self.dh, _stream(self.device)

    def forward(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(out [B, Lq, E], lse [B, H, Lq]): what the backward needs beside the operands."""
        out = torch.empty(self.B, self.Lq, self.E, dtype=torch.float32, device=self.device)
        lse = torch.empty(self.B, self.H, self.Lq, dtype=torch.float32, device=self.device)
        B, H, Lq, Lk, dh, stream = self._geometry()
        _lib.check(self.fwd(_ptr(self.q), self.ldq, _ptr(self.k), self.ldk, _ptr(self.v), self.ldv, _ptr(self.mask), _ptr(out), self.E,
                            _ptr(lse), B, H, Lq, Lk, dh, *self.drop, stream))
        return out, lse

    def backward(self, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, need_q: bool, need_kv: bool):
        """(dq, dk, dv), or (dq, dkv, None) in the packed form; None where not asked for."""
        E = self.E
        dout, lddo = _as_rows(dout, E)
        dq = torch.empty(self.B, self.Lq, E, dtype=torch.float32, device=self.device) if need_q else None
        dk = dv = dkv = None
        ldd = E
        if need_kv and self.packed:
            dkv = torch.empty(self.B, self.Lk, 2 * E, dtype=torch.float32, device=self.device)
            dk, dv, ldd = dkv, dkv[..., E:], 2 * E
        elif need_kv:
            dk, dv = (torch.empty(self.B, self.Lk, E, dtype=torch.float32, device=self.device) for _ in range(2))
        delta = torch.empty(self.B, self.H, self.Lq, dtype=torch.float32, device=self.device)
        B, H, Lq, Lk, dh, stream = self._geometry()
        _lib.check(self.bwd(_ptr(self.q), self.ldq, _ptr(self.k), self.ldk, _ptr(self.v), self.ldv, _ptr(self.mask), _ptr(out), E, _ptr(lse),
                            _ptr(dout), lddo, _ptr(dq), E, _ptr(dk), ldd, _ptr(dv), ldd, _ptr(delta), B, H, Lq, Lk, dh, *self.drop, stream))
        return (dq, dkv, None) if self.packed else (dq, dk, dv)


class _CoreFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_mask, num_heads, drop=None, core="fma"):
        call = _CoreCall(q.detach(), k.detach(), None if v is None else v.detach(), key_mask, num_heads, drop, core)
        out, lse = call.forward()
        ctx.call = call
        ctx.save_for_backward(out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        out, lse = ctx.saved_tensors
        dq, dk, dv = ctx.call.backward(out, lse, dout, need_q, need_k or need_v)
        return dq, dk if need_k else None, dv if need_v else None, None, None, None, None


def attention_core(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_mask: Optional[torch.Tensor], num_heads: int,
                   drop: Optional[Tuple[float, int, int]] = None, core: str = "fma") -> torch.Tensor:
    """out [B, Lq, E] = softmax over the kept keys of (q k^T / sqrt(E / num_heads)) v per head, differentiable in q, k, v.
    q [B, Lq, E], k, v [B, Lk, E]: float32 on the GPU; views with a contiguous last dimension and one row stride (a column
    slice of a wider buffer) are read in place.  key_mask: [B, Lk], nonzero = keep, or None.  A query row with no kept key
    gives zeros and passes no gradient.  k_len <= 512, head dim <= 256.  drop = (p, seed, call): the weights go through the
    library's dropout mask of that draw (csrc/dropout_mask.h), forward and backward.
    core: "fma" (the default) is the fp32 FMA core.  "mfma" runs every product of the forward and the backward on the matrix
    pipes in split-bf16 arithmetic (each fp32 operand as bf16 hi + lo, three MFMA passes, fp32 accumulation; softmax in fp32):
    close to fp32 but not exact - against fp64 within 1e-4 of max|out| and 2e-4 of the gradient scale on standard-normal
    operands.  Same domain, mask, dropout draws and ownership (no atomics, the same bits every run).
    Measured faster than "fma" at all four GHMFC shapes (Lq, Lk, dh) at B = 64, H = 8 (tools/attention_core_bench.py):
    (128, 49, 96) and (128, 128, 96) 6.5 - 9.0 x forward and 3.9 - 4.6 x backward, (49, 128, 256) and (49, 49, 256) 2.8 - 3.1 x
    and 1.7 - 1.8 x.  "fma" stays the default: the choice changes every bit downstream."""
    return _CoreFunction.apply(q, k, v, key_mask, num_heads, drop, _check_core(core))


def attention_core_packed(q: torch.Tensor, kv: torch.Tensor, key_mask: Optional[torch.Tensor], num_heads: int,
                          drop: Optional[Tuple[float, int, int]] = None, core: str = "fma") -> torch.Tensor:
    """attention_core with K | V side by side in one [B, Lk, 2 E] buffer; its gradient comes back as one buffer dK | dV."""
    return _CoreFunction.apply(q, kv, None, key_mask, num_heads, drop, _check_core(core))


# ---- the projections ----------------------------------------------------------------------------------------
_linear_pool = {}                          # _lib._scratch: the ordered dW reduction of drin_linear_bwd


class _LinearFunction(torch.autograd.Function):
    """y = x w^T + b through drin_linear_fwd; dx written, dw and db accumulated into fresh zeros by drin_linear_bwd with the
    scratch that selects its ordered weight-gradient reduction (the same bits every run)."""

    @staticmethod
    def forward(ctx, x, w, b, precision):
        rows, k = x.shape
        n = w.shape[0]
        y = torch.empty(rows, n, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().drin_linear_fwd(_ptr(x), _ptr(w), _ptr(b), _ptr(y), rows, n, k, precision, _stream(x.device)))
        ctx.save_for_backward(x, w)
        ctx.precision, ctx.has_bias = precision, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        rows, k = x.shape
        n = w.shape[0]
        dy = dy.contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.zeros_like(w) if need_w else None
        db = torch.zeros(n, dtype=torch.float32, device=x.device) if need_b and ctx.has_bias else None
        stream = _stream(x.device)
        scratch = _scratch(_linear_pool, x.device, stream.value or 0, ORDERED_DW_SCRATCH * n * k)
        _lib.check(_lib.load().drin_linear_bwd(_ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), rows, n, k, ctx.precision,
                                               _ptr(scratch), scratch.numel(), stream))
        return dx, dw, db, None


def _linear(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], precision: int) -> torch.Tensor:
    return _LinearFunction.apply(x.contiguous(), w.contiguous(), None if b is None else b.contiguous(), precision)


def multihead_attention_forward(query, key, value, key_padding_mask=None, *, embed_dim, num_heads, kdim, vdim, in_proj_weight,
                                q_proj_weight, k_proj_weight, v_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, precision,
                                dropout=0.0, dropout_stream=None, core="fma") -> torch.Tensor:
    """`MultiheadAttention.forward` on parameter tensors, wherever they live (the module's own, or torch's
    `nn.TransformerEncoderLayer.self_attn`): out [B, Lq, E].  `in_proj_weight` is None when the three widths differ (then
    `q_proj_weight`, `k_proj_weight`, `v_proj_weight` are read).  `dropout` is the rate that applies to this call (0 outside
    training); a rate > 0 takes one draw from `dropout_stream`.  `core`: the softmax-attention core (`attention_core`),
    whatever the projections' `precision`."""
    _check_core(core)
    _require_gpu_f32("the module (out_proj.weight)", out_proj_weight)
    for name, t in (("query", query), ("key", key), ("value", value)):
        _require_gpu_f32(name, t)
        if t.dim() != 3:
            raise RuntimeError(f"drin_amd.attention.MultiheadAttention: {name} must be [batch, length, width], got {tuple(t.shape)}")
    B, Lq, E = query.shape
    Lk = key.shape[1]
    if E != embed_dim or key.shape[2] != kdim or value.shape[2] != vdim or key.shape[0] != B or (
            tuple(value.shape[:2]) != (B, Lk)):
        raise RuntimeError(f"drin_amd.attention.MultiheadAttention: query {tuple(query.shape)}, key {tuple(key.shape)}, value "
                           f"{tuple(value.shape)} do not fit embed_dim={embed_dim}, kdim={kdim}, vdim={vdim}")
    if Lk > MAX_KEYS:
        raise NotImplementedError(f"drin_amd.attention.MultiheadAttention: {Lk} keys exceed {MAX_KEYS}")
    mask = None
    if key_padding_mask is not None:           # torch: bool, True = drop (a float mask is additive: not implemented)
        if key_padding_mask.dtype != torch.bool:
            raise NotImplementedError("drin_amd.attention.MultiheadAttention: key_padding_mask must be bool (True = drop)")
        if tuple(key_padding_mask.shape) != (B, Lk):
            raise RuntimeError(f"key_padding_mask {tuple(key_padding_mask.shape)} is not [batch, k_len] = {(B, Lk)}")
        mask = (~key_padding_mask).to(query.device, torch.int64)
    drop = None
    if dropout > 0:
        if not 0.0 < dropout < 1.0:
            raise ValueError(f"drin_amd.attention.MultiheadAttention: dropout {dropout} is not in [0, 1)")
        stream = dropout_stream
        drop = (float(dropout), stream.seed, stream.draw(B, num_heads, Lq, Lk))
    prec = PRECISIONS[precision]
    bias = in_proj_bias
    bq, bk, bv = (None, None, None) if bias is None else (bias[:E], bias[E:2 * E], bias[2 * E:])
    xq = query.reshape(B * Lq, E)
    if in_proj_weight is not None:
        w = in_proj_weight
        q = _linear(xq, w[:E], bq, prec).view(B, Lq, E)
        if key is value:                       # K | V: one product, one [rows, 2 E] buffer, one backward
            kv = _linear(key.reshape(B * Lk, E), w[E:], None if bias is None else bias[E:], prec)
            ctx = attention_core_packed(q, kv.view(B, Lk, 2 * E), mask, num_heads, drop, core)
        else:
            k = _linear(key.reshape(B * Lk, E), w[E:2 * E], bk, prec).view(B, Lk, E)
            v = _linear(value.reshape(B * Lk, E), w[2 * E:], bv, prec).view(B, Lk, E)
            ctx = attention_core(q, k, v, mask, num_heads, drop, core)
    else:
        q = _linear(xq, q_proj_weight, bq, prec).view(B, Lq, E)
        k = _linear(key.reshape(B * Lk, kdim), k_proj_weight, bk, prec).view(B, Lk, E)
        v = _linear(value.reshape(B * Lk, vdim), v_proj_weight, bv, prec).view(B, Lk, E)
        ctx = attention_core(q, k, v, mask, num_heads, drop, core)
    out = _linear(ctx.view(B * Lq, E), out_proj_weight, out_proj_bias, prec)
    return out.view(B, Lq, E)


# ---- the module ---------------------------------------------------------------------------------------------
class MultiheadAttention(nn.MultiheadAttention):
    """`nn.MultiheadAttention(..., batch_first=True)` on the HIP library, forward and backward.  The constructor takes
    torch's arguments plus `precision`: "bf16x3" (split-bf16 projections, the default) or "f32" (exact fp32 MFMA), and
    `core`: "fma" (the fp32 FMA softmax-attention core, the default) or "mfma" (the split-bf16 matrix-core one: `attention_core`),
    chosen independently of `precision`.  `forward(query, key, value, key_padding_mask=None, need_weights=False)` returns
    `(out [B, Lq, E], None)`; gradients reach every parameter that requires one and `query` / `key` / `value` when they do.
    With one embedding width and `key is value`, K | V are one product on rows E .. 3 E of `in_proj_weight` and the core's
    packed dK | dV goes back through one.  Refused, each with the reason: CPU tensors, `batch_first=False`, `attn_mask`,
    `need_weights=True`, `add_bias_kv`, `add_zero_attn`, widths that are no multiple of 4, and `dropout > 0` in training
    mode without a `dropout_stream`.  With `dropout_stream=DropoutStream(seed)` a training-mode
    forward draws one call number from the stream and drops attention weights with the library's own mask (not torch's
    random stream); `eval()` ignores dropout either way."""

    def __init__(self, embed_dim, num_heads, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None,
                 batch_first=False, device=None, dtype=None, precision: str = "bf16x3",
                 dropout_stream: Optional[DropoutStream] = None, core: str = "fma"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r} not in {sorted(PRECISIONS)}")
        _check_core(core)
        if not batch_first:
            raise NotImplementedError("drin_amd.attention.MultiheadAttention: batch_first=False is not implemented; the library "
                                      "reads [batch, length, width] rows (pass batch_first=True)")
        if add_bias_kv or add_zero_attn:
            raise NotImplementedError("drin_amd.attention.MultiheadAttention: add_bias_kv / add_zero_attn are not implemented "
                                      "(they append a key the kernels have no row for)")
        if dtype not in (None, torch.float32):
            raise NotImplementedError(f"drin_amd.attention.MultiheadAttention: float32 parameters only, not {dtype}")
        widths = {"embed_dim": embed_dim, "kdim": embed_dim if kdim is None else kdim, "vdim": embed_dim if vdim is None else vdim}
        bad = {n: w for n, w in widths.items() if w % 4}
        if bad:
            raise NotImplementedError(f"drin_amd.attention.MultiheadAttention: widths must be multiples of 4 (16-byte lane accesses "
                                      f"of the projections), got {bad}")
        if embed_dim % num_heads == 0 and embed_dim // num_heads > MAX_HEAD_DIM:
            raise NotImplementedError(f"drin_amd.attention.MultiheadAttention: head dim {embed_dim // num_heads} exceeds {MAX_HEAD_DIM}")
        super().__init__(embed_dim, num_heads, dropout=dropout, bias=bias, add_bias_kv=False, add_zero_attn=False, kdim=kdim,
                         vdim=vdim, batch_first=True, device=device, dtype=dtype)
        self.precision = precision
        self.dropout_stream = dropout_stream
        self.core = core

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None, average_attn_weights=True,
                is_causal=False):
        if need_weights:
            raise NotImplementedError("drin_amd.attention.MultiheadAttention: need_weights=True is not implemented (the kernels "
                                      "never store the attention weights)")
        if attn_mask is not None or is_causal:
            raise NotImplementedError("drin_amd.attention.MultiheadAttention: attn_mask / is_causal are not implemented; only "
                                      "key_padding_mask is")
        if self.training and self.dropout > 0 and self.dropout_stream is None:
            raise NotImplementedError(f"drin_amd.attention.MultiheadAttention: attention dropout ({self.dropout}) in training mode is "
                                      "not implemented (DESIGN.md section 11); call eval() or build the module with dropout=0")
        return multihead_attention_forward(
            query, key, value, key_padding_mask, embed_dim=self.embed_dim, num_heads=self.num_heads, kdim=self.kdim, vdim=self.vdim,
            in_proj_weight=self.in_proj_weight, q_proj_weight=self.q_proj_weight, k_proj_weight=self.k_proj_weight,
            v_proj_weight=self.v_proj_weight, in_proj_bias=self.in_proj_bias, out_proj_weight=self.out_proj.weight,
            out_proj_bias=self.out_proj.bias, precision=self.precision, dropout=self.dropout if self.training else 0.0,
            dropout_stream=self.dropout_stream, core=self.core), None
