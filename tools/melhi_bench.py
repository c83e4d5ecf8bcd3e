"""Time the MELHI baseline on one GPU: the forward, and the forward + backward + Adam step, at B = 64 and 4096 (N = 11, the
reference widths), with the library's per-kernel-class split, against a plain-torch form of the same model on the same GPU
(nn.LSTM over packed sequences, as the reference builds them).  Prints one JSON line per configuration.

usage:  python tools/melhi_bench.py [--batches 64,4096] [--steps 10] [--warmup 3] [--torch-steps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from drin_amd import _lib  # noqa: E402
from drin_amd.melhi import MelhiConfig, Model  # noqa: E402


def make_batch(B: int, cfg: MelhiConfig, seed: int = 0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D, R, L, P, N = cfg.embed_dim, cfg.image_dim, cfg.mention_tokens, cfg.image_regions, cfg.num_candidates
    mf = torch.randn(B, L, D, device="cuda", generator=g)
    mimage = torch.randn(B, P, R, device="cuda", generator=g).abs()
    ef = torch.randn(B, N, D, device="cuda", generator=g)
    eimage = torch.randn(B, N, R, device="cuda", generator=g)
    s = torch.randint(0, 20, (B,), device="cuda", generator=g)
    e = s + torch.randint(1, 4, (B,), device="cuda", generator=g)
    mlen = torch.clamp(e + torch.randint(1, 40, (B,), device="cuda", generator=g), max=L)
    mmask = (torch.arange(L, device="cuda")[None] < mlen[:, None]).long()
    return [mf, mmask, s + 1, e + 1, mimage, ef, 0, eimage]


def torch_form(model: Model, batch):
    """The plain-torch form: the reference's algorithm on the GPU (packed sequences through nn.LSTM, the same extraction)."""
    mf, mmask, start, end, mimage, ef, _, eimage = batch
    B, L, D = mf.shape
    H = 3 * D
    sim = nn.CosineSimilarity(-1)
    mimg = mimage.mean(-2)
    mim, eim = model.image_map_text(mimg), model.image_map_text(eimage)
    mask = (sim(mf[:, 0], mim) > model.cfg.thres_tmim) & ((sim(mimg.unsqueeze(1).expand_as(eimage), eimage) > model.cfg.thres_imie).sum(-1) > 0)
    mim, eim = mim * mask[:, None], eim * mask[:, None, None]
    st, en, ml = start.tolist(), end.tolist(), mmask.sum(-1).tolist()
    word = torch.stack([mf[b, st[b]:en[b]].mean(0) for b in range(B)])
    x = torch.cat([mf, word[:, None].expand(-1, L, -1), mim[:, None].expand(-1, L, -1)], -1)
    zero = torch.zeros(1, H, device=mf.device)
    lstm = model.mention_encoder.mention_lstm
    outs = []
    for seqs in ([x[b, 1:st[b]] if st[b] > 1 else zero for b in range(B)], [x[b, en[b]:ml[b]] if ml[b] > en[b] else zero for b in range(B)]):
        packed = lstm(nn.utils.rnn.pack_sequence(seqs, enforce_sorted=False))[0]
        outs.append(packed.data[packed.unsorted_indices - 1])
    men = model.mention_encoder.mention_final_map(torch.cat(outs, -1))
    ent = model.entity_final_map(torch.cat([ef, eim], -1))
    return F.cosine_similarity(men.unsqueeze(1).expand_as(ent), ent, dim=-1)


def timeit(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,4096")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    cfg = MelhiConfig()
    for B in [int(x) for x in a.batches.split(",")]:
        torch.manual_seed(0)
        model = Model(cfg, precision=a.precision).cuda()
        opt = torch.optim.Adam(model.parameters(), lr=1e-5)
        batch = make_batch(B, cfg)
        G = torch.randn(B, cfg.num_candidates, device="cuda")

        def fwd():
            with torch.no_grad():
                model(batch)

        def step():
            opt.zero_grad(set_to_none=True)
            (model(batch) * G).sum().backward()
            opt.step()

        fwd_ms = timeit(fwd, a.steps, a.warmup)
        step_ms = timeit(step, a.steps, a.warmup)
        _lib.profile_begin()
        step()
        torch.cuda.synchronize()
        prof = _lib.profile_end()
        with torch.no_grad():
            t_fwd_ms = timeit(lambda: torch_form(model, batch), a.torch_steps, 1)

        def t_step():
            opt.zero_grad(set_to_none=True)
            (torch_form(model, batch) * G).sum().backward()
            opt.step()

        t_step_ms = timeit(t_step, a.torch_steps, 1)
        print(json.dumps({
            "workload": "melhi", "batch": B, "num_candidates": cfg.num_candidates, "precision": a.precision,
            "forward_ms": round(fwd_ms, 3), "train_step_ms": round(step_ms, 3),
            "forward_pairs_per_s": round(B * cfg.num_candidates / fwd_ms * 1e3, 1),
            "train_pairs_per_s": round(B * cfg.num_candidates / step_ms * 1e3, 1),
            "kernel_ms_per_train_step": {k: round(v[0], 3) for k, v in prof.items() if v[1]},
            "launches_per_train_step": {k: v[1] for k, v in prof.items() if v[1]},
            "torch_forward_ms": round(t_fwd_ms, 3), "torch_train_step_ms": round(t_step_ms, 3),
            "speedup_forward": round(t_fwd_ms / fwd_ms, 2), "speedup_train_step": round(t_step_ms / step_ms, 2),
        }), flush=True)


if __name__ == "__main__":
    main()
