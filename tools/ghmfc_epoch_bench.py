"""End-to-end epoch throughput of GHMFC's three batch forms on one GPU, after tools/epoch_bench.py: a
synthetic WikiMEL-layout dataset at the reference widths is written into a temporary directory in the files `GhmfcData` reads,
then one training epoch of `TrainableModel` at the reference's batch of 64 runs through
  gathered  - the reference's loader contract: the host gathers `entity_feature[rows]`, 19.9 MB per mention, and copies it over
  indexed   - `IndexedGhmfcData` through the host loader, the entity table on the device
  device    - the whole split on the device (`GhmfcDeviceSplit`): no host work in the step
and scoring (`eval()`) runs over the device split with and without the per-entity cache.  The loss is a stand-in (softmax
cross-entropy of the scores against the answer) under `torch.optim.Adam`: the step's library work is what is timed.
Reports ms/step with the library's per-kernel-class split of one step and writes a summary line followed by one JSON line
per form to `--out` (profiles/ghmfc_table_bench.jsonl).  A record, not a gate.

usage:  python tools/ghmfc_epoch_bench.py [--mentions 512] [--entities 2048] [--batch 64] [--workers 8] [--out PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from drin_amd import _lib  # noqa: E402
from drin_amd.ghmfc import GhmfcConfig  # noqa: E402
from drin_amd.ghmfc_data import GhmfcDeviceSplit, IndexedGhmfcData, load_entity_table  # noqa: E402
from drin_amd.ghmfc_shim import GhmfcData  # noqa: E402
from drin_amd.ghmfc_train import TrainableModel  # noqa: E402

D, R, L, P, N, T = 768, 2048, 128, 49, 101, 64


def write_dataset(root: str, mentions: int, entities: int, valid: int) -> None:
    g = np.random.Generator(np.random.Philox(key=[7, 1]))
    save = lambda name, a: np.save(os.path.join(root, name), a)   # noqa: E731
    save("entity-attr-feature.npy", g.standard_normal((entities, T, D), dtype=np.float32))
    ntok = g.integers(3, T + 1, size=entities)
    save("entity-attr-mask.npy", (np.arange(T)[None, :] < ntok[:, None]).astype(np.int64))
    qids = np.array([f"Q{100000 + 7 * i}" for i in range(entities)])
    with open(os.path.join(root, "qid2idx.json"), "w") as f:
        json.dump({q: i for i, q in enumerate(qids.tolist())}, f)
    for split, m in (("train", mentions), ("valid", valid), ("test", valid)):
        save(f"mention-text-feature_{split}.npy", g.standard_normal((m, L, D), dtype=np.float32))
        mlen = g.integers(8, L + 1, size=m)
        save(f"mention-text-mask_{split}.npy", (np.arange(L)[None, :] < mlen[:, None]).astype(np.int64))
        save(f"start-pos_{split}.npy", np.zeros(m, dtype=np.int64))
        save(f"end-pos_{split}.npy", np.full(m, 3, dtype=np.int64))
        save(f"mention-image-feature_{split}.npy", np.abs(g.standard_normal((m, P, R), dtype=np.float32)))
        save(f"answer_{split}.npy", g.integers(0, N, size=m).astype(np.int64))
        save(f"entity-name-raw_{split}.npy", qids[g.integers(0, entities, size=(m, N))].reshape(-1))


def to_device(batch, dev):
    return [t.to(dev, non_blocking=True) if isinstance(t, torch.Tensor) else t for t in batch]


def loss_of(scores, onehot):
    onehot = onehot.to(scores.device)
    target = torch.where(onehot.any(1), onehot.argmax(1), torch.full_like(onehot.argmax(1), N - 1))
    return torch.nn.functional.cross_entropy(scores * 20.0, target)


def kernel_split(fn) -> dict:
    _lib.profile_begin()
    fn()
    torch.cuda.synchronize()
    return {k: {"ms": round(ms, 4), "launches": n} for k, (ms, n) in _lib.profile_end().items() if n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mentions", type=int, default=512)
    ap.add_argument("--entities", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ghmfc_table_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="ghmfc_epoch_")
    records = []
    try:
        t0 = time.perf_counter()
        write_dataset(root, a.mentions, a.entities, 2 * a.batch)
        print(f"wrote {a.mentions} mentions / {a.entities} entities to a temporary directory in {time.perf_counter() - t0:.1f} s", flush=True)
        cfg = GhmfcConfig(dataset_name="wikimel", num_candidates=N, embed_dim=D, image_dim=R, mention_tokens=L, image_regions=P,
                          num_heads=8, entity_tokens=T)
        table = load_entity_table(root, dev)
        common = dict(workload="ghmfc_train_epoch", batch=a.batch, mentions=a.mentions, entities=a.entities, precision=a.precision,
                      widths=dict(D=D, R=R, L=L, P=P, N=N, T=T))
        for form in ("device", "indexed", "gathered"):
            torch.manual_seed(0)
            model = TrainableModel(cfg, precision=a.precision, dropout=0.1, seed=0).to(dev).train()
            opt = torch.optim.Adam(model.parameters(), lr=1e-5)
            if form == "gathered":
                make = lambda split: DataLoader(GhmfcData(root, split, "wikimel", N, D, mention_mmap="r"), a.batch,   # noqa: E731
                                                num_workers=a.workers)
            elif form == "indexed":
                make = lambda split: DataLoader(IndexedGhmfcData(root, split, N, mention_mmap="r"), a.batch, num_workers=a.workers)   # noqa: E731
            else:
                make = lambda split: GhmfcDeviceSplit(IndexedGhmfcData(root, split, N), dev, a.batch)   # noqa: E731
            if form != "gathered":
                model.attach_entity_table(table)

            def step(batch):
                batch = to_device(batch, dev)
                loss = loss_of(model(batch[:-1]), batch[-1])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                return batch

            for batch in make("valid"):                    # warm-up: a training pass over the valid split
                last = step(batch)
            torch.cuda.synchronize()
            train = make("train")
            t0 = time.perf_counter()
            for batch in train:
                step(batch)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            steps = len(train)
            model.check_indices()
            rec = dict(common, form=form, steps=steps, ms_per_step=round(dt / steps * 1e3, 3), mentions_per_s=round(a.mentions / dt, 1),
                       kernel_classes_one_step=kernel_split(lambda: step(last)))
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del model, opt, train
            torch.cuda.empty_cache()
        # scoring over the device split, with and without the per-entity rows
        torch.manual_seed(0)
        model = TrainableModel(cfg, precision=a.precision).to(dev).eval()
        model.attach_entity_table(table)
        split = GhmfcDeviceSplit(IndexedGhmfcData(root, "train", N), dev, a.batch)
        for cached in (False, True):
            model.enable_entity_cache(cached)
            with torch.no_grad():
                for batch in split:                        # warm-up: one pass over the split; builds the rows when cached
                    last = batch
                    model(batch[:-1])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for batch in split:
                    model(batch[:-1])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = dict(common, workload="ghmfc_score_epoch", form="device", entity_cache=cached, steps=len(split),
                           ms_per_step=round(dt / len(split) * 1e3, 3), mentions_per_s=round(a.mentions / dt, 1),
                           kernel_classes_one_step=kernel_split(lambda: model(last[:-1])))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    train = {r["form"]: r["ms_per_step"] for r in records if r["workload"] == "ghmfc_train_epoch"}
    score = {"cached" if r["entity_cache"] else "uncached": r["ms_per_step"] for r in records if r["workload"] == "ghmfc_score_epoch"}
    summary = dict(common, workload="summary", train_ms_per_step=train, score_ms_per_step=score)
    with open(a.out, "w") as f:                          # the summary first: what a `track json` tag of a document reads
        for rec in [summary] + records:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
