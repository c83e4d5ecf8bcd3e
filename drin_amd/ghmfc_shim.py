"""The two modules the reference's driver binds for `model_type = "ghmfc"` (`train.py:9-14`), backed by this library, for
training (`trainer.fit`) and for scoring a trained checkpoint (`trainer.test`); DESIGN.md sections 15 and 18.

In a checkout of the reference the binding is one changed line of `train.py`:

    from drin_amd import ghmfc_shim as data_module, ghmfc_shim as model_module      # was: from baselines import ...

`Model()` takes no argument and reads `common.args` (imported at call time); `create_datasets()` gives the [train, valid,
test] loaders of the offline path of `baselines/data.py` (the same `.npy` files, the same 9-item batches) on either dataset.
DRIN_GHMFC_TABLE=1 (WikiMEL) selects the table form of both (`drin_amd.ghmfc_table`, `drin_amd.ghmfc_data`).
"""
from __future__ import annotations

import importlib
import json
import os
from typing import List

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .ghmfc import config_from_reference_args, entity_settings_from_reference_args
from .ghmfc_train import TrainableModel as _Model
from .ghmfc_variants import VariantModel, variant_config_from_reference_args
from .melhi_shim import SPLITS


def _args():
    return importlib.import_module("common.args")


class _DefaultEntityArgs:
    """`common.args` as the two legacy config functions accept it: the default entity names in front of everything else."""
    entity_final_layer_name, entity_final_pooling = "linear", "avg"

    def __init__(self, args):
        self._args = args

    def __getattr__(self, name):
        return getattr(self._args, name)


def _configs(a):
    """(VariantConfig, GhmfcConfig or None for a non-default mention encoder) of `common.args`, the entity settings
    (`entity_final_layer_name`, `entity_final_pooling`: `ghmfc.entity_settings_from_reference_args`) set on both."""
    entity = entity_settings_from_reference_args(a)
    view = _DefaultEntityArgs(a)
    cfg = variant_config_from_reference_args(view)
    base = config_from_reference_args(view) if cfg.is_default else None       # the default's own refusals
    for c in (cfg, base):
        for name, value in entity.items():
            if c is not None:
                setattr(c, name, value)
    return cfg, base


def _table_form() -> bool:
    """DRIN_GHMFC_TABLE=1: the table form - `create_datasets()` gives the indexed loaders and `Model()`
    loads the WikiMEL entity table and attaches it (it follows the model to its device)."""
    return os.environ.get("DRIN_GHMFC_TABLE", "") not in ("", "0")


def _attach_table(model, a):
    from .ghmfc_data import _setup, load_entity_table
    _setup(_DefaultEntityArgs(a))                                              # WikiDiverse has no shared table: refused
    return model.attach_entity_table(load_entity_table(a.preprocess_dir, "cpu", getattr(a, "entity_text_type", "attr")))


class Model(_Model):
    """`model_module.Model()`: geometry and `transformer_dropout` from `common.args`; split-bf16 products unless
    DRIN_PRECISION=f32; the softmax-attention core of DRIN_ATTENTION_CORE ("fma", the default, or "mfma").  The attention dropout of train() mode is the library's own mask, seeded by `args.seed`.  With another
    mention encoder selected in `common.args` (`mention_final_layer_name`, `mention_multimodal_attention`: "transformer",
    "multimodal" + "text", "linear", "none") `Model()` is a `drin_amd.ghmfc_variants.VariantModel` built the same way.
    `entity_final_layer_name` ("linear" | "none") and `entity_final_pooling` ("avg" | "max") are honoured by either."""

    def __new__(cls):
        a = _args()
        cfg, _base = _configs(a)
        if cfg.is_default:
            return super().__new__(cls)
        model = VariantModel(cfg, precision=os.environ.get("DRIN_PRECISION", "bf16x3"), dropout=getattr(a, "transformer_dropout", 0.1),
                             seed=getattr(a, "seed", 0), core=os.environ.get("DRIN_ATTENTION_CORE", "fma"))
        return _attach_table(model, a) if _table_form() else model

    def __init__(self):
        a = _args()
        super().__init__(_configs(a)[1], precision=os.environ.get("DRIN_PRECISION", "bf16x3"),
                         dropout=getattr(a, "transformer_dropout", 0.1), seed=getattr(a, "seed", 0),
                         core=os.environ.get("DRIN_ATTENTION_CORE", "fma"))
        if _table_form():
            _attach_table(self, a)


class GhmfcData(Dataset):
    """One split of the offline features (`baselines/data.py:85-122,169-192`): (mention_feature, mention_mask, start + 1,
    end + 1, mention_image, entity_feature, entity_mask, 0, answer one-hot) per mention.  WikiDiverse: entity_feature [N, D]
    and entity_mask 0; WikiMEL: entity rows gathered from the shared table through `qid2idx.json`, [N, T, D] and [N, T].
    `mention_image=False` (a mention encoder other than "multimodal", `baselines/data.py:113,130`): the image file is not
    opened and the item is 0."""

    def __init__(self, root: str, split: str, dataset_name: str, num_candidates: int, embed_dim: int, entity_text_type: str = "attr",
                 mention_mmap=None, mention_image: bool = True):
        p = lambda name: os.path.join(root, name)   # noqa: E731
        self.wikimel = dataset_name == "wikimel"
        self.mention_feature = np.load(p(f"mention-text-feature_{split}.npy"), mmap_mode=mention_mmap)
        self.mention_mask = np.load(p(f"mention-text-mask_{split}.npy"))
        if self.wikimel:
            self.entity_qid = np.load(p(f"entity-name-raw_{split}.npy")).reshape((-1, num_candidates))
            self.entity_feature = np.load(p(f"entity-{entity_text_type}-feature.npy"))
            self.entity_mask = np.load(p(f"entity-{entity_text_type}-mask.npy"))
            with open(p("qid2idx.json")) as f:
                self.qid2idx = json.load(f)
        else:
            self.entity_feature = np.load(p(f"entity-{entity_text_type}-feature_{split}.npy")).reshape((-1, num_candidates, embed_dim))
        self.start = np.load(p(f"start-pos_{split}.npy"))
        self.end = np.load(p(f"end-pos_{split}.npy"))
        self.answer = np.load(p(f"answer_{split}.npy"))
        self.mention_image = np.load(p(f"mention-image-feature_{split}.npy"), mmap_mode=mention_mmap) if mention_image else None
        n = num_candidates - 1
        self.lookup = torch.cat([torch.eye(n, dtype=torch.int8), torch.zeros(1, n, dtype=torch.int8)])

    def __len__(self):
        return len(self.answer)

    def __getitem__(self, i):
        if self.wikimel:
            rows = [self.qid2idx[q] for q in self.entity_qid[i]]
            entity_feature = torch.from_numpy(np.asarray(self.entity_feature[rows], dtype=np.float32))
            entity_mask = torch.from_numpy(np.asarray(self.entity_mask[rows], dtype=np.int64))
        else:
            entity_feature, entity_mask = torch.from_numpy(self.entity_feature[i].copy()), 0
        return (torch.from_numpy(self.mention_feature[i].copy()), torch.from_numpy(np.asarray(self.mention_mask[i])),
                int(self.start[i]) + 1, int(self.end[i]) + 1,
                0 if self.mention_image is None else torch.from_numpy(np.asarray(self.mention_image[i]).copy()),
                entity_feature, entity_mask, 0, self.lookup[int(self.answer[i])])


def create_datasets() -> List[DataLoader]:
    """`data_module.create_datasets()` for GHMFC: loaders over `args.preprocess_dir` with `args.batch_size`."""
    a = _args()
    cfg, _base = _configs(a)
    if _table_form():
        from .ghmfc_data import create_indexed_datasets
        return create_indexed_datasets(_DefaultEntityArgs(a))                  # the loaders read no entity setting
    loaders = []
    for split in SPLITS:
        ds = GhmfcData(a.preprocess_dir, split, cfg.dataset_name, cfg.num_candidates, cfg.embed_dim,
                       getattr(a, "entity_text_type", "attr"), getattr(a, "mention_mmap", None), cfg.reads_mention_image)
        loaders.append(DataLoader(ds, a.batch_size, shuffle=(split == "train" and getattr(a, "shuffle_train_data", True)),
                                  num_workers=getattr(a, "dataloader_workers", 0)))
    return loaders
