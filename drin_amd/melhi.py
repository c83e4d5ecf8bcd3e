"""The reference's MELHI baseline (`baselines/melhi.py`, WikiDiverse only) on the HIP library: `Model(nn.Module)` with the
reference's 10 state-dict keys and initialisation order, scored and trained by `drin_melhi_forward` / `drin_melhi_backward`.

What the port computes, and why only the time-0 cells and one recurrence per side are needed, is in DESIGN.md section 14.
The one host-side step is the length order of the packed context sequences: torch's own CPU sort (not stable), exactly
the call `pack_sequence(..., enforce_sorted=False)` makes, so that ties land where the reference puts them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import _ptr, _stream

PRECISIONS = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}


@dataclass
class MelhiConfig:
    """Geometry of `common/args.py` that MELHI reads (`bert_embed_dim`, `resnet_embed_dim`, `resnet_num_region`,
    `max_mention_sentence_len`, `num_candidates_model`, `thres_tmim`, `thres_imie`)."""
    dataset_name: str = "wikidiverse"
    num_candidates: int = 11
    embed_dim: int = 768
    image_dim: int = 2048
    mention_tokens: int = 128
    image_regions: int = 49
    thres_tmim: float = 0.3
    thres_imie: float = 0.3
    cosine_eps: float = 1e-8

    def __post_init__(self):
        if self.dataset_name != "wikidiverse":   # melhi.py refuses the other dataset at import
            raise NotImplementedError(
                "melhi is only implemented for wikidiverse; the result of wikimel can be found in its paper")

    @property
    def hidden(self) -> int:
        return 3 * self.embed_dim


def config_from_reference_args(args) -> MelhiConfig:
    """MelhiConfig from a `common.args` module (or any object with its names)."""
    return MelhiConfig(dataset_name=args.dataset_name, num_candidates=args.num_candidates_model, embed_dim=args.bert_embed_dim,
                       image_dim=args.resnet_embed_dim, mention_tokens=args.max_mention_sentence_len,
                       image_regions=args.resnet_num_region, thres_tmim=getattr(args, "thres_tmim", 0.3),
                       thres_imie=getattr(args, "thres_imie", 0.3))


def context_lengths(start: torch.Tensor, end: torch.Tensor, mention_mask: torch.Tensor, L: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Lengths of the two packed sequences of every mention, on the CPU: the left context tokens 1 .. start - 1 and the right
    context tokens end .. sum(mask) - 1 (Python slice rules), or 1 for the all-zero placeholder row of an empty context."""
    start, end = start.detach().cpu().long(), end.detach().cpu().long()
    mlen = mention_mask.detach().cpu().long().sum(-1)
    left = torch.where(start > 1, torch.clamp(start, max=L) - 1, torch.ones_like(start))
    right = torch.where(mlen > end, mlen - end, torch.ones_like(end))
    return left, right


def torch_order(lengths) -> torch.Tensor:
    """The permutation `pack_padded_sequence` sorts by: torch.sort of the int64 CPU lengths, descending (not stable)."""
    return torch.sort(torch.as_tensor(lengths, dtype=torch.int64, device="cpu"), descending=True)[1]


def orders_and_lengths(start, end, mention_mask, L: int) -> Tuple[np.ndarray, np.ndarray]:
    """int32 [2, B] host arrays `order`, `lengths` of drin_melhi_forward (row 0 left, row 1 right)."""
    left, right = context_lengths(start, end, mention_mask, L)
    order = np.stack([torch_order(left).numpy(), torch_order(right).numpy()]).astype(np.int32)
    lengths = np.stack([left.numpy(), right.numpy()]).astype(np.int32)
    return np.ascontiguousarray(order), np.ascontiguousarray(lengths)


class _Call:
    """One forward (+ backward) through the library: the C structs, the host order arrays and the kept workspace."""

    def __init__(self, cfg: MelhiConfig, precision: int, batch: Sequence[torch.Tensor], params: Sequence[torch.Tensor]):
        self.lib = _lib.load()
        mf, mmask, start, end, mimage, ef, eimage = batch
        B = mf.shape[0]
        self.device = mf.device
        c = _lib.DrinMelhiConfigC()
        c.batch, c.num_candidates, c.embed_dim, c.image_dim = B, cfg.num_candidates, cfg.embed_dim, cfg.image_dim
        c.mention_tokens, c.image_regions, c.precision = cfg.mention_tokens, cfg.image_regions, precision
        c.cosine_eps, c.thres_tmim, c.thres_imie = cfg.cosine_eps, cfg.thres_tmim, cfg.thres_imie
        self.cfg = c
        self.tensors = list(batch) + list(params)   # keep every pointer alive for the call
        self.batch = _lib.DrinMelhiBatchC(*[_ptr(t) for t in batch])
        self.params = _lib.DrinMelhiParamsC(*[_ptr(t) for t in params])
        self.order, self.lengths = orders_and_lengths(start, end, mmask, cfg.mention_tokens)
        self.ws_bytes = self.lib.drin_melhi_workspace_bytes(C.byref(c), 1)
        if self.ws_bytes == 0:
            _lib.check(_lib.E_SHAPE)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.B, self.N = B, cfg.num_candidates

    def forward(self) -> torch.Tensor:
        scores = torch.empty(self.B, self.N, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.drin_melhi_forward(C.byref(self.cfg), C.byref(self.batch), C.byref(self.params),
                                               self.order.ctypes.data_as(C.c_void_p), self.lengths.ctypes.data_as(C.c_void_p),
                                               _ptr(self.ws), self.ws_bytes, _ptr(scores), _stream(self.device)))
        return scores

    def backward(self, grad_scores: torch.Tensor, needs: Sequence[bool]) -> list:
        params = self.tensors[7:]
        grads = [torch.zeros_like(p) if need else None for p, need in zip(params, needs)]
        gc = _lib.DrinMelhiParamGradsC(*[_ptr(g) for g in grads])
        g = grad_scores.detach().to(torch.float32).contiguous()
        _lib.check(self.lib.drin_melhi_backward(C.byref(self.cfg), C.byref(self.batch), C.byref(self.params),
                                                self.order.ctypes.data_as(C.c_void_p), self.lengths.ctypes.data_as(C.c_void_p),
                                                _ptr(self.ws), self.ws_bytes, _ptr(g), C.byref(gc), _stream(self.device)))
        return grads


class _MelhiFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, precision, mf, mmask, start, end, mimage, ef, eimage, *params):
        call = _Call(cfg, precision, (mf, mmask, start, end, mimage, ef, eimage), params)
        ctx.call = call
        return call.forward()

    @staticmethod
    def backward(ctx, grad_scores):
        needs = ctx.needs_input_grad[9:]
        grads = ctx.call.backward(grad_scores, needs)
        ctx.call = None
        return (None,) * 9 + tuple(grads)


class _MentionEncoder(nn.Module):
    def __init__(self, cfg: MelhiConfig):
        super().__init__()
        H = cfg.hidden
        self.mention_lstm = nn.LSTM(H, H)
        self.mention_final_map = nn.Linear(2 * H, cfg.embed_dim)


class Model(nn.Module):
    """melhi.py's `Model`: the same modules, created in the same order (so `torch.manual_seed(s); Model()` draws the
    reference's weights) and the same 10 state-dict keys.  `forward(batch)` takes the reference's 8-item WikiDiverse batch
    and returns scores [B, N]; autograd reaches the parameters (not the batch tensors).  `precision`: "bf16x3" (split-bf16
    contractions, the default) or "f32" (exact fp32 MFMA); the recurrence is fp32 FMA in both."""

    def __init__(self, cfg: MelhiConfig | None = None, precision: str = "bf16x3"):
        super().__init__()
        cfg = cfg or MelhiConfig()
        if cfg.dataset_name != "wikidiverse":
            raise NotImplementedError("melhi is only implemented for wikidiverse")
        if precision not in PRECISIONS:
            raise ValueError(f"precision {precision!r} not in {sorted(PRECISIONS)}")
        self.cfg, self.precision = cfg, precision
        self.image_map_text = nn.Linear(cfg.image_dim, cfg.embed_dim)
        self.mention_encoder = _MentionEncoder(cfg)
        self.entity_final_map = nn.Linear(2 * cfg.embed_dim, cfg.embed_dim)

    def param_list(self) -> list:
        """The parameters in drin_melhi_params order."""
        lstm = self.mention_encoder.mention_lstm
        return [self.image_map_text.weight, self.image_map_text.bias, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0,
                lstm.bias_hh_l0, self.mention_encoder.mention_final_map.weight, self.mention_encoder.mention_final_map.bias,
                self.entity_final_map.weight, self.entity_final_map.bias]

    def forward(self, batch) -> torch.Tensor:
        mf, mmask, start, end, mimage, ef, _entity_mask, eimage = batch[:8]
        dev = self.image_map_text.weight.device
        if dev.type != "cuda":
            raise RuntimeError("drin_amd.melhi.Model runs on the GPU only (no CPU fallback): move it with .cuda()")
        f = lambda t: t.to(dev, torch.float32).contiguous()          # noqa: E731
        i = lambda t: torch.as_tensor(t).to(dev, torch.int64).contiguous()   # noqa: E731
        return _MelhiFunction.apply(self.cfg, PRECISIONS[self.precision], f(mf), i(mmask), i(start), i(end), f(mimage), f(ef),
                                    f(eimage), *[p.contiguous() for p in self.param_list()])
