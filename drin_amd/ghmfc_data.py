"""GHMFC's WikiMEL data in table form: what `ghmfc_shim.GhmfcData` gathers per mention on the host
(`baselines/data.py`: `rows = [self.qid2idx[q] ...]`, `entity_feature[rows]` - `[N, T, D]`, 19.9 MB at the reference widths) stays
an `[N]` int64 row list, and the entity table goes to the device once.

* `IndexedGhmfcData`: the same 9-item samples with item 5 = the candidate rows and item 6 = 0; the entity feature file is never
  opened.
* `load_entity_table`: the table as a `drin_amd.model.EntityTable(text, mask, None, None, None)`.
* `create_indexed_datasets`: the three loaders; `GhmfcDeviceSplit` / `create_device_splits`: whole splits on the device,
  iterated as slices / index-selects of device tensors like `drin_amd.data.DeviceSplit`.

The WikiDiverse layout stores per-mention candidate features and has no shared table: refused.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional

import numpy as np
import torch
from torch.utils.data import DataLoader

from .data import ShardSampler
from .ghmfc_shim import GhmfcData, _args
from .ghmfc_variants import variant_config_from_reference_args
from .melhi_shim import SPLITS
from .model import EntityTable


class IndexedGhmfcData(GhmfcData):
    """One WikiMEL split in table form: (mention_feature, mention_mask, start + 1, end + 1, mention_image, rows [N] int64, 0, 0,
    answer one-hot) per mention, `rows` being what `qid2idx` maps the stored QIDs to (`baselines/data.py`'s gather index)."""

    def __init__(self, root: str, split: str, num_candidates: int, mention_mmap=None, mention_image: bool = True):
        p = lambda name: os.path.join(root, name)   # noqa: E731
        self.wikimel = True
        self.mention_feature = np.load(p(f"mention-text-feature_{split}.npy"), mmap_mode=mention_mmap)
        self.mention_mask = np.load(p(f"mention-text-mask_{split}.npy"))
        self.entity_qid = np.load(p(f"entity-name-raw_{split}.npy")).reshape((-1, num_candidates))
        with open(p("qid2idx.json")) as f:
            self.qid2idx = json.load(f)
        self.start = np.load(p(f"start-pos_{split}.npy"))
        self.end = np.load(p(f"end-pos_{split}.npy"))
        self.answer = np.load(p(f"answer_{split}.npy"))
        self.mention_image = np.load(p(f"mention-image-feature_{split}.npy"), mmap_mode=mention_mmap) if mention_image else None
        n = num_candidates - 1
        self.lookup = torch.cat([torch.eye(n, dtype=torch.int8), torch.zeros(1, n, dtype=torch.int8)])

    def rows(self, i) -> np.ndarray:
        return np.asarray([self.qid2idx[q] for q in self.entity_qid[i]], dtype=np.int64)

    def __getitem__(self, i):
        return (torch.from_numpy(self.mention_feature[i].copy()), torch.from_numpy(np.asarray(self.mention_mask[i])),
                int(self.start[i]) + 1, int(self.end[i]) + 1,
                0 if self.mention_image is None else torch.from_numpy(np.asarray(self.mention_image[i]).copy()),
                torch.from_numpy(self.rows(i)), 0, 0, self.lookup[int(self.answer[i])])


def load_entity_table(root: str, device="cpu", entity_text_type: str = "attr") -> EntityTable:
    """The shared WikiMEL entity table (`entity-<type>-feature.npy` `[E, T, D]`, `entity-<type>-mask.npy` `[E, T]`) on `device`."""
    up = lambda name: torch.as_tensor(np.ascontiguousarray(np.load(os.path.join(root, name)))).to(device)   # noqa: E731
    return EntityTable(up(f"entity-{entity_text_type}-feature.npy").to(torch.float32), up(f"entity-{entity_text_type}-mask.npy").to(torch.int64),
                       None, None, None)


def _setup(args):
    a = args if args is not None else _args()
    cfg = variant_config_from_reference_args(a)
    if cfg.dataset_name != "wikimel":
        raise ValueError("the table form exists for the wikimel layout only (baselines/data.py: the qid2idx gather)")
    return a, cfg


def create_indexed_datasets(args=None) -> List[DataLoader]:
    """[train, valid, test] loaders of `IndexedGhmfcData` over `args.preprocess_dir` (`args`: `common.args` by default), as
    `ghmfc_shim.create_datasets()` builds them (WikiMEL only)."""
    a, cfg = _setup(args)
    loaders = []
    for split in SPLITS:
        ds = IndexedGhmfcData(a.preprocess_dir, split, cfg.num_candidates, getattr(a, "mention_mmap", None), cfg.reads_mention_image)
        loaders.append(DataLoader(ds, a.batch_size, shuffle=(split == "train" and getattr(a, "shuffle_train_data", True)),
                                  num_workers=getattr(a, "dataloader_workers", 0)))
    return loaders


class GhmfcDeviceSplit:
    """One split of `IndexedGhmfcData` resident on `device`: mention tensors, candidate rows and answers are uploaded once;
    iterating yields the 9-item batches of a `DataLoader(ds, batch_size, sampler=sampler)` - same order, same shapes and dtypes
    (the loader's collated 0s are int64 zeros `[B]`) - as slices (no sampler) or as views of one index-select per epoch."""

    def __init__(self, ds: IndexedGhmfcData, device, batch_size: int, sampler=None):
        dev = torch.device(device)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        n = len(ds)
        zeros = torch.zeros(n, dtype=torch.int64, device=dev)
        rows = np.stack([ds.rows(i) for i in range(n)]) if n else np.zeros((0, ds.entity_qid.shape[1]), dtype=np.int64)
        self.tensors = [up(ds.mention_feature), up(ds.mention_mask), up(np.asarray(ds.start).astype(np.int64)) + 1,
                        up(np.asarray(ds.end).astype(np.int64)) + 1, zeros if ds.mention_image is None else up(ds.mention_image),
                        up(rows), zeros, zeros]
        self.lookup = ds.lookup.to(dev)
        self.answer = up(np.asarray(ds.answer).astype(np.int64))
        self.n, self.batch_size, self.sampler, self.device, self.dataset = n, batch_size, sampler, dev, ds

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None else self.n
        return (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        if self.sampler is None:
            for b0 in range(0, self.n, self.batch_size):                  # contiguous: views, nothing is copied
                sl = slice(b0, min(self.n, b0 + self.batch_size))
                yield [t[sl] for t in self.tensors] + [self.lookup[self.answer[sl]]]
        else:
            order = torch.as_tensor(list(self.sampler), dtype=torch.int64).to(self.device)
            shard = [t.index_select(0, order) for t in self.tensors] + [self.lookup[self.answer.index_select(0, order)]]
            for b0 in range(0, order.numel(), self.batch_size):
                yield [t[b0:b0 + self.batch_size] for t in shard]


def create_device_splits(device, args=None) -> List[GhmfcDeviceSplit]:
    """[train, valid, test] `GhmfcDeviceSplit`s: a drop-in for `create_indexed_datasets()`.  The train split is shuffled by a
    `drin_amd.data.ShardSampler` seeded with `args.seed` (call `split.sampler.set_epoch(e)` per epoch)."""
    a, cfg = _setup(args)
    splits = []
    for split in SPLITS:
        ds = IndexedGhmfcData(a.preprocess_dir, split, cfg.num_candidates, getattr(a, "mention_mmap", None), cfg.reads_mention_image)
        shuffle = split == "train" and getattr(a, "shuffle_train_data", True)
        sampler: Optional[ShardSampler] = ShardSampler(len(ds), 0, 1, True, getattr(a, "seed", 0)) if shuffle else None
        splits.append(GhmfcDeviceSplit(ds, device, a.batch_size, sampler))
    return splits
