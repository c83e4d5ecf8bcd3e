"""A plain-torch restatement of the reference's MELHI forward (baselines/melhi.py), written from its semantics
(DESIGN.md section 14), for the tests: any dtype (fp64 on the GPU as the yardstick), any device, differentiable in the
parameters.  It computes what the reference's lstm_extract_last returns without packing anything: the time-0 output of
every context sequence and one full recurrence per side, placed by torch's length order.

`sd` is a state dict with the reference's 10 keys; `batch` the 8-item WikiDiverse batch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def torch_order(lengths) -> torch.Tensor:
    return torch.sort(torch.as_tensor(lengths, dtype=torch.int64, device="cpu"), descending=True)[1]


def _cell(gates: torch.Tensor, c_prev):
    i, f, g, o = gates.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = i * g if c_prev is None else f * c_prev + i * g
    return o * torch.tanh(c), c


def melhi_scores(batch, sd, thres_tmim: float = 0.3, thres_imie: float = 0.3, eps: float = 1e-8, return_mask: bool = False):
    mf, mmask, start, end, mimage, ef, _, eimage = batch[:8]
    B, L, D = mf.shape
    dev = mf.device
    w_img, b_img = sd["image_map_text.weight"], sd["image_map_text.bias"]
    w_ih, w_hh = sd["mention_encoder.mention_lstm.weight_ih_l0"], sd["mention_encoder.mention_lstm.weight_hh_l0"]
    b_ih, b_hh = sd["mention_encoder.mention_lstm.bias_ih_l0"], sd["mention_encoder.mention_lstm.bias_hh_l0"]

    # image side and the mask (no gradient through the comparisons)
    mimg = mimage.mean(-2)
    mim = mimg @ w_img.T + b_img
    eim = eimage @ w_img.T + b_img
    c1 = F.cosine_similarity(mf[:, 0], mim, dim=-1, eps=eps)
    c2 = F.cosine_similarity(mimg.unsqueeze(1).expand_as(eimage), eimage, dim=-1, eps=eps)
    mask = ((c1 > thres_tmim) & (c2 > thres_imie).any(-1)).to(mf.dtype)
    mim = mim * mask[:, None]
    eim = eim * mask[:, None, None]

    # span mean, Python slice rules (an empty span is NaN)
    st, en = start.detach().cpu().long().tolist(), end.detach().cpu().long().tolist()
    word = torch.stack([mf[b, st[b]:en[b]].mean(0) for b in range(B)])

    # X = [token | word | mim]: the last two blocks are one constant per mention
    w_tok = w_ih[:, :D]
    const = word @ w_ih[:, D:2 * D].T + mim @ w_ih[:, 2 * D:].T + b_ih + b_hh
    mlen = mmask.detach().cpu().long().sum(-1).tolist()
    sides = []
    for side in range(2):
        toks = []
        for b in range(B):
            if side == 0:
                toks.append(list(range(1, min(st[b], L))) if st[b] > 1 else None)
            else:
                toks.append(list(range(en[b], mlen[b])) if mlen[b] > en[b] else None)
        lengths = [len(t) if t is not None else 1 for t in toks]
        order = torch_order(lengths).tolist()
        real = torch.tensor([t is not None for t in toks], device=dev)
        tok0 = torch.tensor([t[0] if t is not None else 0 for t in toks], device=dev)
        x0 = mf[torch.arange(B, device=dev), tok0]
        g0 = torch.where(real[:, None], x0 @ w_tok.T + const, (b_ih + b_hh).expand(B, -1))
        h0, _ = _cell(g0, None)
        tmax = lengths[order[0]]
        c = sum(1 for j in order if lengths[j] == tmax)
        jstar = order[c - 1]
        if tmax >= 2:
            h, cs = None, None
            for t in toks[jstar]:
                gates = mf[jstar, t] @ w_tok.T + const[jstar]
                if h is not None:
                    gates = gates + h @ w_hh.T
                h, cs = _cell(gates, cs)
            last = h
        else:
            last = h0[jstar]
        pos = [0] * B
        for p, j in enumerate(order):
            pos[j] = p
        sides.append(torch.stack([h0[order[pos[b] - 1]] if pos[b] > 0 else last for b in range(B)]))
    men = torch.cat(sides, -1) @ sd["mention_encoder.mention_final_map.weight"].T + sd["mention_encoder.mention_final_map.bias"]
    ent = torch.cat([ef, eim], -1) @ sd["entity_final_map.weight"].T + sd["entity_final_map.bias"]
    scores = F.cosine_similarity(men.unsqueeze(1).expand_as(ent), ent, dim=-1, eps=eps)
    return (scores, mask) if return_mask else scores
