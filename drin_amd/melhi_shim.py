"""The two modules the reference's driver binds for `model_type = "melhi"` (`train.py:9-14`), backed by this library.

In a checkout of the reference the binding is one changed line of `train.py`:

    from drin_amd import melhi_shim as data_module, melhi_shim as model_module      # was: from baselines import ...

`Model()` takes no argument and reads `common.args` (imported at call time); `create_datasets()` gives the [train, valid,
test] loaders of the WikiDiverse offline path of `baselines/data.py` (the same `.npy` files, the same 9-item batches).
"""
from __future__ import annotations

import importlib
import os
from typing import List

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .melhi import Model as _Model
from .melhi import config_from_reference_args

SPLITS = ("train", "valid", "test")


def _args():
    return importlib.import_module("common.args")


class Model(_Model):
    """`model_module.Model()`: geometry from `common.args`; split-bf16 contractions unless DRIN_PRECISION=f32."""

    def __init__(self):
        super().__init__(config_from_reference_args(_args()), precision=os.environ.get("DRIN_PRECISION", "bf16x3"))


class MelhiData(Dataset):
    """One split of the WikiDiverse offline features: (mention_feature, mention_mask, start + 1, end + 1, mention_image,
    entity_feature, 0, entity_image, answer one-hot) per mention."""

    def __init__(self, root: str, split: str, num_candidates: int, embed_dim: int, image_dim: int, mention_mmap=None,
                 entity_mmap=None):
        p = lambda name: os.path.join(root, f"{name}_{split}.npy")   # noqa: E731
        self.mention_feature = np.load(p("mention-text-feature"), mmap_mode=mention_mmap)
        self.mention_mask = np.load(p("mention-text-mask"))
        self.entity_feature = np.load(p("entity-attr-feature")).reshape((-1, num_candidates, embed_dim))
        self.start = np.load(p("start-pos"))
        self.end = np.load(p("end-pos"))
        self.answer = np.load(p("answer"))
        self.mention_image = np.load(p("mention-image-feature"), mmap_mode=mention_mmap)
        self.entity_image = np.load(p("entity-image-feature"), mmap_mode=entity_mmap).reshape((-1, num_candidates, image_dim))
        n = num_candidates - 1
        self.lookup = torch.cat([torch.eye(n, dtype=torch.int8), torch.zeros(1, n, dtype=torch.int8)])

    def __len__(self):
        return len(self.answer)

    def __getitem__(self, i):
        return (torch.from_numpy(self.mention_feature[i].copy()), torch.from_numpy(np.asarray(self.mention_mask[i])),
                int(self.start[i]) + 1, int(self.end[i]) + 1, torch.from_numpy(np.asarray(self.mention_image[i]).copy()),
                torch.from_numpy(self.entity_feature[i].copy()), 0, torch.from_numpy(np.asarray(self.entity_image[i]).copy()),
                self.lookup[int(self.answer[i])])


def create_datasets() -> List[DataLoader]:
    """`data_module.create_datasets()` for MELHI: loaders over `args.preprocess_dir` with `args.batch_size`."""
    a = _args()
    cfg = config_from_reference_args(a)
    loaders = []
    for split in SPLITS:
        ds = MelhiData(a.preprocess_dir, split, cfg.num_candidates, cfg.embed_dim, cfg.image_dim,
                       getattr(a, "mention_mmap", None), getattr(a, "entity_mmap", None))
        loaders.append(DataLoader(ds, a.batch_size, shuffle=(split == "train" and getattr(a, "shuffle_train_data", True)),
                                  num_workers=getattr(a, "dataloader_workers", 0)))
    return loaders
