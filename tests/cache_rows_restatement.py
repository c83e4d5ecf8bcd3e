"""Test infrastructure (plain torch, no GPU, never imported by the product): the rows of the per-entity cache
(`drin_build_entity_cache`, csrc/entity_cache.hip) restated field by field from the reference's own formulas, and the two storage
layouts of a row decoded and encoded byte for byte.

`fields` evaluates the seven fields UNFOLDED - the entity encoders first (`model.py:26-46`), the layer-1 operands from their
outputs (`model.py:128,146,148-153`) - so that it shares no algebra with `drin_prepare`, which folds W_h1 W_e / W_v1 W_e once per
weight version.  In fp64 (`fields64`) it is the yardstick; in fp32 it is the reference's own distance from that yardstick, which is
what the GPU tests take for their slack.  `scores_from_fields` pushes the fields through the arithmetic the cached path does, so
that tests/test_cache_rows_host.py can show the restatement is the same model as `oracle.drin_oracle.forward`.

Row layouts (floats; the header of csrc/entity_cache.hip):
  f32        h_t 0 | h_i D | fv_t 2D | fv_i 3D | c^ 4D | o^ 5D | sg 5D+R (+ 3 pad)
  mixed_f16  h_t 0 | h_i D | c^ 2D | fv 3D | o^ 4D | tail 4D + R/2: sg, s_fvt, s_fvi, s_o
             fv: the 16-byte unit of float4 column c4 holds fv_t[4 c4 .. +3] then fv_i[4 c4 .. +3] as fp16; o^: R fp16 in natural order
Field names: h_t, h_i, fv_t, fv_i, chat (c^), ohat (o^), sg - the names of `oracle.precision_emulation.CACHE_FIELDS`."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import drin_oracle as O

F16_FIELDS = ("fv_t", "fv_i", "ohat")                       # scaled fp16 in the mixed rows
TAIL_SLOT = {"sg": 0, "fv_t": 1, "fv_i": 2, "ohat": 3}       # mixed rows: tail = sg, s_fvt, s_fvi, s_o
FORMATS = ("f32", "mixed_f16")


def row_floats(D: int, R: int, fmt: str) -> int:
    return 4 * D + R // 2 + 4 if fmt == "mixed_f16" else 5 * D + R + 4


def _offsets(D: int, R: int, fmt: str) -> Dict[str, Tuple[int, int]]:
    """{name: (first float, floats)} of one row."""
    if fmt == "mixed_f16":
        return {"h_t": (0, D), "h_i": (D, D), "chat": (2 * D, D), "fv": (3 * D, D), "ohat": (4 * D, R // 2), "tail": (4 * D + R // 2, 4)}
    return {"h_t": (0, D), "h_i": (D, D), "fv_t": (2 * D, D), "fv_i": (3 * D, D), "chat": (4 * D, D), "ohat": (5 * D, R), "tail": (5 * D + R, 4)}


def _widths(cfg) -> Tuple[int, int]:
    return cfg.gcn_embed_dim, cfg.resnet_embed_dim


# ---- the fields, from the reference's formulas ---------------------------------------------------------------------------------
def fields(cfg, sd, text, mask, image, obj, score, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The seven fields of every row of a table, evaluated in `dtype`: text [E, T, D] (+ mask [E, T]) or pooled [E, D], image
    [E, (1,) R], obj [E, Ke, (1,) R], score [E, Ke].  Also "x_t", the pooled text (NaN where the reference's slice is empty)."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    text, image, obj, score = text.to(dtype), image.to(dtype), obj.to(dtype), score.to(dtype)
    E = text.shape[0]
    if text.dim() == 3:                                     # ghmfc.py:245-249; model.py:73-75: token 0 feeds the cosine
        x_t, cls = O.entity_token_mean(text[None], mask[None])[0], text[:, 0]
    else:
        x_t = cls = text
    x_i = image.mean(-2) if image.dim() == 3 else image     # model.py:43-45
    if obj.dim() == 4:                                      # model.py:82-83
        obj = obj.mean(-2)
    pre = "vertex_encoder."
    W_et, b_et = p[pre + "entity_text_encoder.final_layer.weight"], p[pre + "entity_text_encoder.final_layer.bias"]
    W_ei, b_ei = p[pre + "entity_image_linear.weight"], p[pre + "entity_image_linear.bias"]
    W_h1 = p["gcn_layers.0.w_h.weight"]
    W_v1, b_v1 = p["gcn_layers.0.w_v.weight"], p["gcn_layers.0.w_v.bias"]
    et0, ei0 = F.linear(x_t, W_et, b_et), F.linear(x_i, W_ei, b_ei)
    eps = cfg.cosine_eps
    unit_obj = obj / torch.linalg.vector_norm(obj, dim=-1, keepdim=True).clamp_min(eps)
    ohat = torch.zeros(E, obj.shape[-1], dtype=dtype)
    sg = torch.zeros(E, dtype=dtype)
    for j in range(obj.shape[1]):                           # model.py:86-91: j in order
        ohat = ohat + score[:, j, None] * unit_obj[:, j]
        sg = sg + score[:, j]
    return {"x_t": x_t,
            "h_t": F.linear(et0 - b_et, W_h1), "h_i": F.linear(ei0 - b_ei, W_h1),
            "fv_t": F.linear(et0, W_v1, b_v1), "fv_i": F.linear(ei0, W_v1, b_v1),
            "chat": cls / torch.linalg.vector_norm(cls, dim=-1, keepdim=True).clamp_min(eps),
            "ohat": ohat, "sg": sg}


def fields64(cfg, sd, text, mask, image, obj, score) -> Dict[str, torch.Tensor]:
    return fields(cfg, sd, text, mask, image, obj, score, torch.float64)


def folded_weights64(sd) -> Dict[str, torch.Tensor]:
    """{field: the [D, K] matrix whose product with x_t / x_i the builder's table-sized GEMM of that field evaluates}, in fp64 -
    the operands `precision_emulation._rounded_product_error` needs to say what a split-bf16 product of that field may miss."""
    p = {k: v.double() for k, v in sd.items()}
    W_et, W_ei = p["vertex_encoder.entity_text_encoder.final_layer.weight"], p["vertex_encoder.entity_image_linear.weight"]
    W_h1, W_v1 = p["gcn_layers.0.w_h.weight"], p["gcn_layers.0.w_v.weight"]
    return {"h_t": W_h1 @ W_et, "h_i": W_h1 @ W_ei, "fv_t": W_v1 @ W_et, "fv_i": W_v1 @ W_ei}


def scores_from_fields(cfg, sd, f: Dict[str, torch.Tensor], mention, candidates, miet, mtei) -> torch.Tensor:
    """Scores [B, N] from the fields of the candidates' rows, by the arithmetic of the cached path (`k_cached_pairs` and what
    follows it), in the fields' dtype: `mention` = the first 7 tensors of the 14-sequence, `candidates` [B, N] rows of the table.
    Two layers, scalar edges, every edge on; activations and the edge type from `cfg`."""
    dt = f["h_t"].dtype
    p = {k: v.to(dt) for k, v in sd.items()}
    mtf, _mask, start, end, mimg, mobj, ms = [t.to(dt) if t.is_floating_point() else t for t in mention]
    act_v, act_e = getattr(F, cfg.gcn_vertex_activation), getattr(F, cfg.gcn_edge_activation)
    g = {k: v[candidates] for k, v in f.items()}                                         # [B, N, .]
    pre = "vertex_encoder."
    span = O.span_mean(mtf, start, end)
    mt0 = F.linear(span, p[pre + "mention_text_encoder.final_layer.linear.weight"], p[pre + "mention_text_encoder.final_layer.linear.bias"])
    mi0 = F.linear(mimg.mean(-2), p[pre + "mention_image_linear.weight"], p[pre + "mention_image_linear.bias"])
    b_et, b_ei = p[pre + "entity_text_encoder.final_layer.bias"], p[pre + "entity_image_linear.bias"]
    L = "gcn_layers.0."
    W_h1, b_h1 = p[L + "w_h.weight"], p[L + "w_h.bias"]
    unit = lambda x: x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(cfg.cosine_eps)   # noqa: E731
    if mobj.dim() == 4:
        mobj = mobj.mean(-2)
    mu = (ms[..., None] * unit(mobj)).sum(-2)
    e_tt = (unit(span)[:, None, :] * g["chat"]).sum(-1)
    e_ti, e_it = mtei.to(dt) / cfg.clip_logit_scale, miet.to(dt) / cfg.clip_logit_scale
    e_ii = (mu[:, None, :] * g["ohat"]).sum(-1) / (ms.sum(-1)[:, None] * g["sg"] + cfg.miei_eps)
    hm_t, hm_i = F.linear(mt0, W_h1), F.linear(mi0, W_h1)
    wb_t, wb_i = W_h1 @ b_et, W_h1 @ b_ei
    D = W_h1.shape[0]
    ln = lambda h: act_v(F.layer_norm(h, (D,), p[L + "layer_norm.weight"], p[L + "layer_norm.bias"], cfg.layer_norm_eps))   # noqa: E731
    ht, hi = g["h_t"], g["h_i"]
    c = lambda e: e[..., None]                                                            # noqa: E731
    et1 = ln(ht + c(e_tt) * hm_t[:, None] + c(e_it) * hm_i[:, None] + wb_t + b_h1)
    ei1 = ln(hi + c(e_ti) * hm_t[:, None] + c(e_ii) * hm_i[:, None] + wb_i + b_h1)
    mt1 = ln((c(e_tt) * (ht + wb_t)).mean(1) + (c(e_ti) * (hi + wb_i)).mean(1) + hm_t + b_h1)
    mi1 = ln((c(e_it) * (ht + wb_t)).mean(1) + (c(e_ii) * (hi + wb_i)).mean(1) + hm_i + b_h1)
    edges = [e_tt, e_ti, e_it, e_ii]
    if cfg.gcn_edge_type == "dynamic":
        fu_t = F.linear(mt0, p[L + "w_u.weight"], p[L + "w_u.bias"])
        fu_i = F.linear(mi0, p[L + "w_u.weight"], p[L + "w_u.bias"])
        edges = [act_e((fu[:, None, :] * g[fv]).mean(-1) + e)
                 for e, fu, fv in ((e_tt, fu_t, "fv_t"), (e_ti, fu_t, "fv_i"), (e_it, fu_i, "fv_t"), (e_ii, fu_i, "fv_i"))]
    v2, _ = O.gcn_layer(p, 1, [mt1, mi1, et1, ei1], edges, (1, 1, 1, 1), cfg.gcn_edge_type == "dynamic",
                        vertex_activation=cfg.gcn_vertex_activation, edge_activation=cfg.gcn_edge_activation)
    return O.cosine(v2[0][:, None, :], v2[2], cfg.cosine_eps)


# ---- the scale rule and the fp16 conversion --------------------------------------------------------------------------------------
def field_scale(max_abs: torch.Tensor) -> torch.Tensor:
    """`cache_field_scale` (csrc/device_utils.h): the smallest power of two >= max_abs; 1 for a zero, NaN or infinite max; never
    below 2^-126 (a denormal max) nor above 2^126 (so that the reciprocal is a normal number too).  fp64 in, fp64 out."""
    m = max_abs.to(torch.float64)
    ok = (m > 0) & torch.isfinite(m)
    safe = torch.where(ok, m, torch.ones_like(m))
    mant, exp = torch.frexp(safe)                           # safe = mant 2^exp, mant in [0.5, 1)
    exp = torch.where(mant == 0.5, exp - 1, exp).clamp(-126, 126)
    return torch.where(ok, torch.ldexp(torch.ones_like(m), exp), torch.ones_like(m))


def scaled_f16_parts(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(units fp16 [..., K], scale fp64 [..., 1]): x / scale rounded to fp16, nearest even, under the row's `field_scale`."""
    x = x.to(torch.float64)
    scale = field_scale(x.abs().amax(-1, keepdim=True))
    return (x / scale).to(torch.float32).to(torch.float16), scale


def scaled_f16(x: torch.Tensor) -> torch.Tensor:
    """What a mixed row holds of x, back in fp64."""
    units, scale = scaled_f16_parts(x)
    return units.to(torch.float64) * scale


# ---- the two row layouts ------------------------------------------------------------------------------------------------------------
def _rows(cache: torch.Tensor, D: int, R: int, fmt: str) -> torch.Tensor:
    """[E, row floats] fp32 VIEW of a cache buffer (uint8 or fp32, any device)."""
    flat = cache.view(torch.float32) if cache.dtype != torch.float32 else cache
    return flat.view(-1, row_floats(D, R, fmt))


def field_view(cache: torch.Tensor, cfg, fmt: str, name: str) -> torch.Tensor:
    """[E, floats] fp32 VIEW (no copy) of one block of every row: a field's name, "fv" (the interleaved fp16 units of the mixed
    rows) or "tail"."""
    D, R = _widths(cfg)
    first, n = _offsets(D, R, fmt)[name]
    return _rows(cache, D, R, fmt)[:, first:first + n]


def decode(cache: torch.Tensor, cfg, fmt: str) -> Dict[str, Optional[torch.Tensor]]:
    """{h_t, h_i, chat, sg: fp32 as stored; fv_t, fv_i, ohat: fp32 as stored (f32 rows) or unit x scale in fp64 (mixed rows);
    "units": {fv_t, fv_i, ohat: the raw fp16 [E, K]} (mixed rows, else None); "tail": [E, 4] fp32 - sg, s_fvt, s_fvi, s_o (mixed)
    or sg and the 3 pad floats (f32)}.  Copies: the buffer is not aliased."""
    D, R = _widths(cfg)
    rows = _rows(cache, D, R, fmt)
    E = rows.shape[0]
    off = _offsets(D, R, fmt)
    take = lambda k: rows[:, off[k][0]:off[k][0] + off[k][1]].clone()   # noqa: E731
    out = {k: take(k) for k in ("h_t", "h_i", "chat", "tail")}
    out["sg"] = out["tail"][:, 0].clone()
    if fmt != "mixed_f16":
        out.update({k: take(k) for k in F16_FIELDS}, units=None)
        return out
    fv = take("fv").view(torch.float16).view(E, D // 4, 2, 4)           # [column c4][fv_t | fv_i][4]
    units = {"fv_t": fv[:, :, 0, :].reshape(E, D), "fv_i": fv[:, :, 1, :].reshape(E, D), "ohat": take("ohat").view(torch.float16).view(E, R)}
    out["units"] = units
    for k in F16_FIELDS:
        out[k] = units[k].to(torch.float64) * out["tail"][:, TAIL_SLOT[k], None].to(torch.float64)
    return out


def encode(f: Dict[str, torch.Tensor], cfg, fmt: str) -> torch.Tensor:
    """The inverse of `decode`: the bytes (uint8) of the rows.  f32 rows are built from h_t, h_i, fv_t, fv_i, chat, ohat and
    "tail"; mixed rows from h_t, h_i, chat, "units" and "tail" (the fp64 products of `decode` are derived, not stored)."""
    D, R = _widths(cfg)
    E = f["h_t"].shape[0]
    off = _offsets(D, R, fmt)
    rows = torch.zeros(E, row_floats(D, R, fmt), dtype=torch.int32, device=f["h_t"].device)   # (integers: bits move as they are)

    def put(k, v):
        rows[:, off[k][0]:off[k][0] + off[k][1]] = v.contiguous().view(torch.int32).view(E, off[k][1])
    for k in ("h_t", "h_i", "chat", "tail"):
        put(k, f[k])
    if fmt != "mixed_f16":
        for k in F16_FIELDS:
            put(k, f[k])
    else:
        u = f["units"]
        put("fv", torch.stack([u["fv_t"].view(E, D // 4, 4), u["fv_i"].view(E, D // 4, 4)], dim=2))
        put("ohat", u["ohat"])
    return rows.view(torch.uint8).view(-1)


def scale_field_in_place(cache: torch.Tensor, cfg, fmt: str, field: str, k: int) -> None:
    """One field of every row of a built cache times exactly 2^k, in place: the field's tail scale (mixed rows' fp16 fields) or
    the field's floats."""
    D, R = _widths(cfg)
    rows = _rows(cache, D, R, fmt)
    off = _offsets(D, R, fmt)
    if fmt == "mixed_f16" and field in F16_FIELDS:
        rows[:, off["tail"][0] + TAIL_SLOT[field]] *= 2.0 ** k
    else:
        rows[:, off[field][0]:off[field][0] + off[field][1]] *= 2.0 ** k
