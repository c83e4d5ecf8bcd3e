"""GHMFC's row operations as differentiable functions on the HIP library: LayerNorm with a fused residual, the max over a
sequence, the gate, the cosine against the candidates and the entity token mean - one `torch.autograd.Function` per pair of
entry points (`drin_layernorm_res_train_fwd` / `_bwd`, `drin_seq_max_train_fwd` / `_bwd`, `drin_gate_mix_fwd` / `_bwd`,
`drin_cosine_rows_fwd` / `_bwd`, `drin_entity_token_mean`).  What the kernels compute: DESIGN.md section 18.  For GHMFC's other
mention encoders (section 20): the FFN activation with row dropout (`drin_act_dropout_fwd` / `_bwd`) and the mean over the
mention span (`drin_span_mean_fwd` / `_bwd`).

GPU only, float32, contiguous rows; there is no CPU fallback and no torch math inside.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import _ptr, _scratch, _stream
from .attention import _require_gpu_f32

_row_pool = {}                             # _lib._scratch: the ordered column sums of the row backwards


def _rows(name: str, t: torch.Tensor) -> torch.Tensor:
    _require_gpu_f32(name, t)
    return t.detach().contiguous()


class _LayerNormRes(torch.autograd.Function):
    """y = LayerNorm(x [+ res]); the gradient of the pre-norm sum goes to x and to res alike."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        x, gamma, beta = _rows("x", x), _rows("gamma", gamma), _rows("beta", beta)
        res = None if res is None else _rows("res", res)
        if res is not None and res.shape != x.shape:
            raise RuntimeError(f"layer_norm_res: x {tuple(x.shape)} and res {tuple(res.shape)} differ")
        E = x.shape[-1]
        rows = x.numel() // E
        y = torch.empty_like(x)
        mean, rstd = (torch.empty(rows, dtype=torch.float32, device=x.device) for _ in range(2))
        _lib.check(_lib.load().drin_layernorm_res_train_fwd(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd),
                                                            rows, E, eps, _stream(x.device)))
        ctx.save_for_backward(x, res, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, gamma, mean, rstd = ctx.saved_tensors
        need_x, need_res, need_g, need_b = ctx.needs_input_grad[:4]
        if not (need_x or need_res or need_g or need_b):
            return None, None, None, None, None
        lib = _lib.load()
        E = x.shape[-1]
        rows = x.numel() // E
        dy = dy.contiguous()
        dh = torch.empty_like(x)
        dgamma = torch.empty_like(gamma) if need_g else None
        dbeta = torch.empty_like(gamma) if need_b else None
        stream = _stream(x.device)
        floats = lib.drin_layernorm_res_bwd_scratch_floats(rows, E) if (need_g or need_b) else 0
        scratch = _scratch(_row_pool, x.device, stream.value or 0, floats) if floats else None
        _lib.check(lib.drin_layernorm_res_bwd(_ptr(x), _ptr(res), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dy), _ptr(dh), _ptr(dgamma),
                                              _ptr(dbeta), _ptr(scratch), floats, rows, E, stream))
        return dh if need_x else None, dh if (need_res and res is not None) else None, dgamma, dbeta, None


def layer_norm_res(x: torch.Tensor, res: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """LayerNorm(x + res) over the last dimension (res may be None), widths that are multiples of 4 up to 2048."""
    return _LayerNormRes.apply(x, res, gamma, beta, eps)


class _SeqMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _rows("x", x)
        B, S, E = x.shape
        out = torch.empty(B, E, dtype=torch.float32, device=x.device)
        idx = torch.empty(B, E, dtype=torch.int32, device=x.device)
        _lib.check(_lib.load().drin_seq_max_train_fwd(_ptr(x), _ptr(out), _ptr(idx), B, S, E, _stream(x.device)))
        ctx.save_for_backward(idx)
        ctx.seq_len = S
        ctx.mark_non_differentiable(idx)
        return out, idx

    @staticmethod
    def backward(ctx, dout, _didx):
        (idx,) = ctx.saved_tensors
        B, E = idx.shape
        dout = dout.contiguous()
        dx = torch.empty(B, ctx.seq_len, E, dtype=torch.float32, device=idx.device)
        _lib.check(_lib.load().drin_seq_max_bwd(_ptr(dout), _ptr(idx), _ptr(dx), B, ctx.seq_len, E, _stream(idx.device)))
        return dx


def seq_max(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(max over dim 1 of x [B, S, E], idx int32 [B, E]): idx is the lowest position that attains the maximum (the lowest NaN
    position when the column holds one); the gradient goes to that position alone."""
    return _SeqMax.apply(x)


class _GateMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tl, vl, ws, bs):
        tl, vl, ws, bs = _rows("tl", tl), _rows("vl", vl), _rows("ws", ws), _rows("bs", bs)
        B, D = tl.shape
        if tuple(vl.shape) != (B, D) or tuple(ws.shape) != (2, 2 * D) or tuple(bs.shape) != (2,):
            raise RuntimeError(f"gate_mix: tl {tuple(tl.shape)}, vl {tuple(vl.shape)}, ws {tuple(ws.shape)}, bs {tuple(bs.shape)} do not fit")
        out = torch.empty_like(tl)
        _lib.check(_lib.load().drin_gate_mix_fwd(_ptr(tl), _ptr(vl), _ptr(ws), _ptr(bs), _ptr(out), B, D, _stream(tl.device)))
        ctx.save_for_backward(tl, vl, ws, bs)
        return out

    @staticmethod
    def backward(ctx, dout):
        tl, vl, ws, bs = ctx.saved_tensors
        need_t, need_v, need_w, need_b = ctx.needs_input_grad
        if not any(ctx.needs_input_grad):
            return None, None, None, None
        lib = _lib.load()
        B, D = tl.shape
        dout = dout.contiguous()
        dtl, dvl = torch.empty_like(tl), torch.empty_like(vl)
        dws = torch.empty_like(ws) if need_w else None
        dbs = torch.empty(2, dtype=torch.float32, device=tl.device) if need_b else None
        stream = _stream(tl.device)
        floats = lib.drin_gate_mix_bwd_scratch_floats(B, D) if (need_w or need_b) else 0
        scratch = _scratch(_row_pool, tl.device, stream.value or 0, floats) if floats else None
        _lib.check(lib.drin_gate_mix_bwd(_ptr(tl), _ptr(vl), _ptr(ws), _ptr(bs), _ptr(dout), _ptr(dtl), _ptr(dvl), _ptr(dws), _ptr(dbs),
                                         _ptr(scratch), floats, B, D, stream))
        return dtl if need_t else None, dvl if need_v else None, dws, dbs


def gate_mix(tl: torch.Tensor, vl: torch.Tensor, ws: torch.Tensor, bs: torch.Tensor) -> torch.Tensor:
    """s0 gelu(tl) + s1 gelu(vl) with s = softmax([gelu(tl) | gelu(vl)] ws^T + bs): tl, vl [B, D], ws [2, 2 D], bs [2]."""
    return _GateMix.apply(tl, vl, ws, bs)


class _CosineRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, eps):
        x, y = _rows("x", x), _rows("y", y)
        B, D = x.shape
        if y.dim() != 3 or y.shape[0] != B or y.shape[2] != D:
            raise RuntimeError(f"cosine_rows: x {tuple(x.shape)} and y {tuple(y.shape)} do not fit")
        N = y.shape[1]
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().drin_cosine_rows_fwd(_ptr(x), _ptr(y), _ptr(out), B, N, D, eps, _stream(x.device)))
        ctx.save_for_backward(x, y)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y = ctx.saved_tensors
        need_x, need_y = ctx.needs_input_grad[:2]
        if not (need_x or need_y):
            return None, None, None
        B, N, D = y.shape
        dout = dout.contiguous()
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        stream = _stream(x.device)
        scratch = _scratch(_row_pool, x.device, stream.value or 0, 3 * B * N)
        _lib.check(_lib.load().drin_cosine_rows_bwd(_ptr(x), _ptr(y), _ptr(dout), _ptr(dx), _ptr(dy), _ptr(scratch), scratch.numel(), B, N, D,
                                                    ctx.eps, stream))
        return dx if need_x else None, dy if need_y else None, None


def cosine_rows(x: torch.Tensor, y: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """out [B, N] = cos(x[b], y[b, n]) with nn.CosineSimilarity's clamp: x [B, D], y [B, N, D]."""
    return _CosineRows.apply(x, y, eps)


class _ActDropout(torch.autograd.Function):
    """y = act(x) m / (1 - p); the backward recomputes act' from x (plain dropout keeps nothing)."""

    @staticmethod
    def forward(ctx, x, act, drop):
        x = _rows("x", x)
        if act not in _lib.ROW_ACT:
            raise ValueError(f"act_dropout: act {act!r} not in {sorted(_lib.ROW_ACT)}")
        width = x.shape[-1]
        rows = x.numel() // width
        p, seed, call = drop if drop is not None else (0.0, 0, 0)
        y = torch.empty_like(x)
        _lib.check(_lib.load().drin_act_dropout_fwd(_ptr(x), _ptr(y), rows, width, _lib.ROW_ACT[act], p, seed, call, _stream(x.device)))
        ctx.save_for_backward(*(() if act == "none" else (x,)))
        ctx.setup = (rows, width, _lib.ROW_ACT[act], p, seed, call)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        x = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _lib.check(_lib.load().drin_act_dropout_bwd(_ptr(x), _ptr(dy), _ptr(dx), *ctx.setup, _stream(dy.device)))
        return dx, None, None


def act_dropout(x: torch.Tensor, act: str = "none", drop: Optional[Tuple[float, int, int]] = None) -> torch.Tensor:
    """act(x) m / (1 - p) over the last dimension's rows: act "none" | "relu" | "gelu" (exact erf), drop = (p, seed, call) of a
    `DropoutStream.draw_rows(rows, width)` or None for no dropout.  Widths that are multiples of 4."""
    return _ActDropout.apply(x, act, drop)


class _SpanMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seq, start, end):
        seq = _rows("seq", seq)
        B, L, D = seq.shape
        start, end = (torch.as_tensor(t).to(seq.device, torch.int64).contiguous() for t in (start, end))
        if tuple(start.shape) != (B,) or tuple(end.shape) != (B,):
            raise RuntimeError(f"span_mean: start {tuple(start.shape)} / end {tuple(end.shape)} are not [batch] = {(B,)}")
        out = torch.empty(B, D, dtype=torch.float32, device=seq.device)
        _lib.check(_lib.load().drin_span_mean_fwd(_ptr(seq), _ptr(start), _ptr(end), _ptr(out), B, L, D, _stream(seq.device)))
        ctx.save_for_backward(start, end)
        ctx.seq_len = L
        return out

    @staticmethod
    def backward(ctx, dout):
        start, end = ctx.saved_tensors
        dout = dout.contiguous()
        B, D = dout.shape
        dseq = torch.empty(B, ctx.seq_len, D, dtype=torch.float32, device=dout.device)
        _lib.check(_lib.load().drin_span_mean_bwd(_ptr(dout), _ptr(start), _ptr(end), _ptr(dseq), B, ctx.seq_len, D, _stream(dout.device)))
        return dseq, None, None


def span_mean(seq: torch.Tensor, start: torch.Tensor, end: torch.Tensor) -> torch.Tensor:
    """[B, D] = mean of seq[b, start[b] : end[b]] (seq [B, L, D]) with Python's slice clipping; an empty span gives a NaN row
    forward, as the reference's `Avg.avg`, and passes a zero gradient."""
    return _SpanMean.apply(seq, start, end)


def entity_token_mean(feat: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[B, N, D] = mean of tokens 1 : ntok - 1 of feat [B, N, T, D], ntok = mask.sum(-1) (mask [B, N, T]); an entity with
    fewer than 3 tokens gives a NaN row, as the reference's empty mean.  An input: no gradient."""
    feat = _rows("entity_feature", feat)
    B, N, T, D = feat.shape
    mask = mask.to(feat.device, torch.int64).contiguous()
    out = torch.empty(B, N, D, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().drin_entity_token_mean(_ptr(feat), _ptr(mask), _ptr(out), B * N, T, D, _stream(feat.device)))
    return out


def entity_token_pool(feat: torch.Tensor, mask: torch.Tensor, pooling: str) -> torch.Tensor:
    """[B, N, D] = the mean ("avg": `entity_token_mean`, its call and bits) or the maximum ("max", `drin_entity_token_pool`) over
    tokens 1 : ntok - 1 of feat [B, N, T, D].  The maximum is exact, a NaN inside the slice wins as in `torch.max`, and an entity with
    fewer than 3 tokens gives a NaN row - where the reference's max raises IndexError.  An input: no gradient."""
    if pooling not in _lib.ENTITY_POOLINGS:
        raise ValueError(f"pooling {pooling!r} is none of {tuple(_lib.ENTITY_POOLINGS)}")
    if pooling == "avg":
        return entity_token_mean(feat, mask)
    feat = _rows("entity_feature", feat)
    B, N, T, D = feat.shape
    mask = mask.to(feat.device, torch.int64).contiguous()
    out = torch.empty(B, N, D, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.load().drin_entity_token_pool(_ptr(feat), _ptr(mask), _ptr(out), B * N, T, D, _lib.ENTITY_POOLINGS[pooling],
                                                  _stream(feat.device)))
    return out
