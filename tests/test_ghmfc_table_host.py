"""CPU-side checks of GHMFC's table form: the new entry points are exported, bound and declared with the
ABI still 12, `drin_ghmfc_table` is laid out as the header says, every entry point refuses bad arguments with the right status
before any launch, the workspace layouts hold, and the data helpers (`drin_amd.ghmfc_data`) deliver what the loader's qid2idx
gather indexes - without opening the entity feature file."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from drin_amd import _lib
from drin_amd.data import ShardSampler
from drin_amd.ghmfc_data import GhmfcDeviceSplit, IndexedGhmfcData, create_device_splits, create_indexed_datasets, load_entity_table
from drin_amd.ghmfc_shim import GhmfcData
from drin_amd.ghmfc_table import GhmfcIndexedBatch, TableForm, raise_bad_index
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantModel
from drin_amd.model import EntityTable
from tests.ghmfc_table_inputs import write_wikimel_dataset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
NEW_INT = ("drin_gather_rows", "drin_entity_token_mean_indexed", "drin_cosine_rows_indexed_fwd", "drin_ghmfc_forward_table",
           "drin_ghmfc_entity_rows")
NEW_SIZE = ("drin_ghmfc_table_workspace_bytes", "drin_ghmfc_entity_rows_workspace_bytes")
ONE = C.c_void_p(16)      # aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)      # 4-byte aligned only
BIG = 1 << 40


def last():
    return _lib.load().drin_last_error().decode()


def test_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in NEW_INT:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    for name in NEW_SIZE:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API size_t {name}(" in header, name
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12
    assert "ghmfc_table.hip" in __import__("drin_amd.build", fromlist=["SOURCES"]).SOURCES


def test_table_mirror_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.DrinGhmfcTableC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(drin_ghmfc_table));']
    lines += [f'  printf("{f} %zu\\n", offsetof(drin_ghmfc_table, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "table.c", tmp_path / "table"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)     # the header is plain C
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.DrinGhmfcTableC)
    for f in fields:
        assert int(got[f]) == getattr(_lib.DrinGhmfcTableC, f).offset, f


def test_indexed_row_entry_points_validate_on_host():
    lib = _lib.load()

    def gather(table=ONE, index=ONE, E=9, out=ONE, count=5, width=16, status=ONE):
        return lib.drin_gather_rows(table, index, E, out, count, width, status, None)

    def mean(text=ONE, mask=ONE, index=ONE, E=9, out=ONE, pairs=5, tokens=6, width=16, status=ONE):
        return lib.drin_entity_token_mean_indexed(text, mask, index, E, out, pairs, tokens, width, status, None)

    def cosine(x=ONE, rows=ONE, index=ONE, E=9, out=ONE, batch=2, n=4, width=16, status=ONE):
        return lib.drin_cosine_rows_indexed_fwd(x, rows, index, E, out, batch, n, width, 1e-8, status, None)

    for f, who, first in ((gather, "drin_gather_rows", "table"), (mean, "drin_entity_token_mean_indexed", "text"),
                          (cosine, "drin_cosine_rows_indexed_fwd", "x")):
        assert f(None) == _lib.E_NULL and last() == f"{who}: {first} is NULL"
        assert f(ODD) == _lib.E_ALIGN and last() == f"{who}: {first} is not 16-byte aligned"
        assert f(out=None) == _lib.E_NULL and "out is NULL" in last()
        assert f(index=None) == _lib.E_NULL and last() == f"{who}: index is NULL"
        assert f(index=ODD) == _lib.E_ALIGN and "index must be 8-byte" in last()
        assert f(status=C.c_void_p(18)) == _lib.E_ALIGN and "index_status 4-byte" in last()
        for E in (0, -3):
            assert f(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()
        for width in (0, 6, -4):
            assert f(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
    assert gather(out=ODD) == _lib.E_ALIGN and "out is not 16-byte aligned" in last()
    assert gather(count=0) == _lib.E_SHAPE and "count = 0" in last()
    assert mean(mask=None) == _lib.E_NULL and "mask is NULL" in last()
    assert mean(pairs=0) == _lib.E_SHAPE and "pairs = 0" in last()
    assert mean(tokens=0) == _lib.E_SHAPE and "tokens = 0" in last()
    assert cosine(rows=None) == _lib.E_NULL and "rows is NULL" in last()
    assert cosine(rows=ODD) == _lib.E_ALIGN and "rows is not 16-byte aligned" in last()
    assert cosine(batch=0) == _lib.E_SHAPE and "batch = 0" in last()
    assert cosine(n=65536) == _lib.E_SHAPE and "num_candidates = 65536" in last()


def ghmfc_config(B=3, N=4, D=16, R=32, L=12, P=3, H=2, precision=_lib.PREC_BF16X3):
    return _lib.DrinGhmfcConfigC(batch=B, num_candidates=N, embed_dim=D, image_dim=R, mention_tokens=L, image_regions=P, num_heads=H,
                                 entity_tokens=0, precision=precision, layer_norm_eps=1e-5, cosine_eps=1e-8)


def table_struct(**over):
    f = dict(size=C.sizeof(_lib.DrinGhmfcTableC), text=ONE, mask=ONE, num_entities=9, entity_tokens=6, candidates=ONE, index_status=ONE,
             rows=None)
    f.update(over)
    return _lib.DrinGhmfcTableC(**f)


def test_forward_table_validates_on_host():
    lib = _lib.load()
    who = "drin_ghmfc_forward_table"
    params = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[16] * 52))
    batch = _lib.DrinGhmfcBatchC(ONE, ONE, ONE, None, None)            # entity_feature / entity_mask are not read

    def run(cfg=None, bt=batch, pc=params, table=None, ws=ONE, nbytes=BIG, scores=ONE, men=ONE, **over):
        cfg = cfg or ghmfc_config()
        t = table if table is not None else table_struct(**over)
        return lib.drin_ghmfc_forward_table(C.byref(cfg), C.byref(bt), C.byref(pc), C.byref(t), ws, nbytes, scores, men, None)

    assert run(scores=None) == _lib.E_NULL and last().startswith(who)
    assert run(ws=None) == _lib.E_NULL
    assert lib.drin_ghmfc_forward_table(C.byref(ghmfc_config()), C.byref(batch), C.byref(params), None, ONE, BIG, ONE, ONE, None) == _lib.E_NULL
    assert "table is NULL" in last()
    assert run(size=C.sizeof(_lib.DrinGhmfcTableC) - 8) == _lib.E_SHAPE and "table.size" in last()
    assert run(size=0) == _lib.E_SHAPE
    for E in (0, -1):
        assert run(num_entities=E) == _lib.E_SHAPE and f"table.num_entities = {E}" in last()
    assert run(entity_tokens=-1) == _lib.E_SHAPE and run(entity_tokens=513) == _lib.E_SHAPE and "entity_tokens = 513" in last()
    assert run(cfg=ghmfc_config(D=18)) == _lib.E_SHAPE and "multiples of 4" in last()
    assert run(candidates=None) == _lib.E_NULL and "table.candidates" in last()
    assert run(text=None) == _lib.E_NULL
    assert run(mask=None) == _lib.E_NULL
    assert run(mask=None, entity_tokens=0, nbytes=0) == _lib.E_WORKSPACE      # a pooled table reads no mask: the next check
    assert run(text=None, mask=None, rows=ONE, nbytes=0) == _lib.E_WORKSPACE  # with rows neither text nor mask is read
    assert run(bt=_lib.DrinGhmfcBatchC(None, ONE, ONE, None, None)) == _lib.E_NULL
    broken = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*([16] * 51 + [0])))
    assert run(pc=broken) == _lib.E_NULL and f"{who}: parameter 51" in last()
    assert run(nbytes=1024) == _lib.E_WORKSPACE and "workspace 1024 bytes <" in last()
    assert run(text=ODD) == _lib.E_ALIGN and run(ws=ODD) == _lib.E_ALIGN and run(men=ODD) == _lib.E_ALIGN
    assert run(rows=ODD) == _lib.E_ALIGN and run(candidates=ODD) == _lib.E_ALIGN and run(index_status=C.c_void_p(18)) == _lib.E_ALIGN
    assert who in last()
    # the workspace: less without the entity regions, 0 on a bad table
    c = ghmfc_config(B=300)
    full = lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(table_struct()))
    pooled = lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(table_struct(entity_tokens=0)))
    lean = lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(table_struct(rows=ONE)))
    plain = lib.drin_ghmfc_workspace_bytes(C.byref(c))
    assert full == pooled > lean > 0 and full - lean >= 2 * 256 * 4 * 16 * 4 and full >= plain
    assert lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(table_struct(size=3))) == 0 and "table.size" in last()
    assert lib.drin_ghmfc_table_workspace_bytes(C.byref(c), None) == 0


def test_entity_rows_validates_on_host():
    lib = _lib.load()
    who = "drin_ghmfc_entity_rows"

    def run(text=ONE, mask=ONE, E=9, T=6, D=16, w=ONE, b=ONE, precision=_lib.PREC_BF16X3, rows=ONE, ws=ONE, nbytes=BIG):
        return lib.drin_ghmfc_entity_rows(text, mask, E, T, D, w, b, precision, rows, ws, nbytes, None)

    for name in ("text", "w", "b", "rows", "mask", "ws"):
        assert run(**{name: None}) == _lib.E_NULL and last().startswith(who), name
    for name in ("text", "w", "b", "rows", "ws"):
        assert run(**{name: ODD}) == _lib.E_ALIGN and last().startswith(who), name
    for D in (0, 6, -4):
        assert run(D=D) == _lib.E_SHAPE and "multiple of 4" in last()
    for E in (0, -1):
        assert run(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()
    assert run(T=-1) == _lib.E_SHAPE and run(T=513) == _lib.E_SHAPE
    assert run(precision=7) == _lib.E_UNSUPPORTED
    assert run(nbytes=16) == _lib.E_WORKSPACE and "workspace 16 bytes <" in last()
    need = lib.drin_ghmfc_entity_rows_workspace_bytes
    assert need(9, 6, 16) == 9 * 16 * 4 + (-(9 * 16 * 4) % 256) and need(9, 0, 16) == 0       # a pooled table needs none
    assert need(1 << 20, 64, 768) == 65536 * 768 * 4                                       # one chunk of entities
    assert need(0, 6, 16) == 0 and need(9, 6, 6) == 0


def test_layout_selfcheck_passes():
    """drin_host_selftest walks the table-form layouts at the tiny widths, the reference widths and N = 1001 (api.hip)."""
    lib = _lib.load()
    assert lib.drin_host_selftest() == _lib.OK, last()
    src = open(os.path.join(REPO, "drin_amd", "csrc", "api.hip")).read()
    assert "ghmfc_table_layout_selfcheck(b, 4, 16, 32, 12, 3, 6" in src and "ghmfc_table_layout_selfcheck(b, 1001, 768, 2048, 128, 49, 64" in src


# ---- the models, as far as they go without a GPU -----------------------------------------------------------------------------
def test_models_refuse_on_the_host():
    from tests.test_ghmfc_host import cfg_for
    model = TrainableModel(cfg_for("wm_b3")).eval()
    assert isinstance(model, TableForm) and issubclass(VariantModel, TableForm)
    D, N = model.cfg.embed_dim, model.cfg.num_candidates
    text, mask = torch.zeros(5, 6, D), torch.ones(5, 6, dtype=torch.int64)
    cand = torch.zeros(3, N, dtype=torch.int64)
    mention = [torch.zeros(3, 12, D), torch.ones(3, 12, dtype=torch.int64), torch.ones(3), torch.ones(3), torch.zeros(3, 3, 32)]
    with pytest.raises(ValueError, match="5 items"):
        GhmfcIndexedBatch(mention[:4], EntityTable(text, mask, None, None, None), cand)
    with pytest.raises(RuntimeError, match="GPU only"):
        model(GhmfcIndexedBatch(mention, EntityTable(text, mask, None, None, None), cand))
    with pytest.raises(ValueError, match="no entity table is attached"):
        model(mention + [cand, 0, 0])
    with pytest.raises(NotImplementedError, match="bfloat16"):
        model.attach_entity_table(EntityTable(text.bfloat16(), mask, None, None, None))
    with pytest.raises(ValueError, match="neither"):
        model.attach_entity_table(EntityTable(torch.zeros(5, 6, D + 4), mask, None, None, None))
    with pytest.raises(ValueError, match="does not match"):
        model.attach_entity_table(EntityTable(text, mask[:, :5], None, None, None))
    with pytest.raises(TypeError):
        model.attach_entity_table((text, mask))
    model.attach_entity_table(EntityTable(text, mask, None, None, None))
    with pytest.raises(RuntimeError, match="GPU only"):                # attached on the host, the model still there
        model(mention + [cand, 0, 0])
    assert model.entity_table is not None and model.attach_entity_table(None).entity_table is None
    assert model.enable_entity_cache().entity_cache_builds == 0
    assert "_table_state" not in model.__getstate__()                   # per-process bookkeeping is not copied
    with pytest.raises(IndexError, match=r"row -4 at pair 205"):
        raise_bad_index([1, 205, -4, -1])
    with pytest.raises(IndexError, match=r"row 4294967297 at pair 3"):
        raise_bad_index([1, 3, 1, 1])


# ---- the data helpers --------------------------------------------------------------------------------------------------------
def fake_args(root, **over):
    a = types.ModuleType("common.args")
    for k, v in dict(dataset_name="wikimel", num_candidates_model=4, bert_embed_dim=16, resnet_embed_dim=32, max_mention_sentence_len=12,
                     resnet_num_region=3, transformer_num_heads=2, transformer_dropout=0.1, seed=5, preprocess_dir=str(root),
                     batch_size=3, shuffle_train_data=False, max_entity_attr_token_len=6).items():
        setattr(a, k, v)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def same_batches(a, b):
    a, b = list(a), list(b)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert len(x) == len(y) == 9
        for i, (s, t) in enumerate(zip(x, y)):
            assert s.dtype == t.dtype and torch.equal(s, t), i


def test_indexed_data_gives_the_rows_of_qid2idx(tmp_path, monkeypatch):
    info = write_wikimel_dataset(str(tmp_path), entity_features=False)  # the feature file does not exist: opening it fails
    opened = []
    real_load = np.load
    monkeypatch.setattr(np, "load", lambda path, *a, **k: (opened.append(os.path.basename(str(path))), real_load(path, *a, **k))[1])
    with pytest.raises(FileNotFoundError):
        GhmfcData(str(tmp_path), "train", "wikimel", 4, 16)              # the gathered form needs it
    opened.clear()
    ds = IndexedGhmfcData(str(tmp_path), "train", 4)
    assert len(ds) == 7
    for i in range(len(ds)):
        item = ds[i]
        assert len(item) == 9
        mf, mmask, start, end, image, rows, emask, eimage, answer = item
        assert mf.shape == (12, 16) and mf.dtype == torch.float32 and mmask.shape == (12,) and mmask.dtype == torch.int64
        assert isinstance(start, int) and isinstance(end, int) and start == 1 and image.shape == (3, 32)
        assert rows.shape == (4,) and rows.dtype == torch.int64 and np.array_equal(rows.numpy(), info["pick"]["train"][i])
        assert emask == 0 and eimage == 0 and answer.shape == (3,) and answer.dtype == torch.int8
    assert "entity-attr-feature.npy" not in opened and "entity-attr-mask.npy" not in opened
    assert IndexedGhmfcData(str(tmp_path), "valid", 4, mention_image=False)[0][4] == 0
    loaders = create_indexed_datasets(fake_args(tmp_path))
    assert [len(ld.dataset) for ld in loaders] == [7, 3, 2]
    batch = next(iter(loaders[0]))
    assert batch[5].shape == (3, 4) and batch[5].dtype == torch.int64 and np.array_equal(batch[5].numpy(), info["pick"]["train"][:3])
    assert batch[6].tolist() == [0, 0, 0] and "entity-attr-feature.npy" not in opened
    with pytest.raises(ValueError, match="wikimel layout only"):
        create_indexed_datasets(fake_args(tmp_path, dataset_name="wikidiverse"))
    with pytest.raises(ValueError, match="wikimel layout only"):
        create_device_splits("cpu", fake_args(tmp_path, dataset_name="wikidiverse"))


def test_indexed_items_are_the_gathered_items(tmp_path):
    write_wikimel_dataset(str(tmp_path))
    table = load_entity_table(str(tmp_path))
    assert table.text.shape == (9, 6, 16) and table.text.dtype == torch.float32 and table.mask.dtype == torch.int64
    assert table.image is None and table.object is None and table.object_score is None and table.num_entities == 9
    full, indexed = GhmfcData(str(tmp_path), "test", "wikimel", 4, 16), IndexedGhmfcData(str(tmp_path), "test", 4)
    for i in range(len(full)):
        a, b = full[i], indexed[i]
        assert torch.equal(a[5], table.text[b[5]]) and torch.equal(a[6], table.mask[b[5]])
        assert all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(a[:5] + a[7:], b[:5] + b[7:]))


@pytest.mark.parametrize("image", [True, False])
def test_device_split_yields_the_loaders_batches(tmp_path, image):
    write_wikimel_dataset(str(tmp_path))
    ds = IndexedGhmfcData(str(tmp_path), "train", 4, mention_image=image)
    same_batches(GhmfcDeviceSplit(ds, "cpu", 3), DataLoader(ds, 3))
    same_batches(GhmfcDeviceSplit(ds, "cpu", 7), DataLoader(ds, 7))
    sampler = ShardSampler(len(ds), 0, 1, True, seed=11)
    split = GhmfcDeviceSplit(ds, "cpu", 2, sampler)
    assert len(split) == len(DataLoader(ds, 2, sampler=sampler)) == 4
    for epoch in (0, 1):
        sampler.set_epoch(epoch)
        same_batches(split, DataLoader(ds, 2, sampler=sampler))
    splits = create_device_splits("cpu", fake_args(tmp_path, shuffle_train_data=True))
    assert [s.n for s in splits] == [7, 3, 2] and splits[0].sampler is not None and splits[1].sampler is None
    same_batches(splits[0], DataLoader(splits[0].dataset, 3, sampler=splits[0].sampler))


def test_shim_is_unchanged_without_the_switch(tmp_path, monkeypatch):
    write_wikimel_dataset(str(tmp_path))
    args = fake_args(tmp_path)
    common = types.ModuleType("common")
    common.args = args
    monkeypatch.setitem(sys.modules, "common", common)
    monkeypatch.setitem(sys.modules, "common.args", args)
    from drin_amd import ghmfc_shim
    monkeypatch.delenv("DRIN_GHMFC_TABLE", raising=False)
    model = ghmfc_shim.Model()
    assert isinstance(model, TrainableModel) and model.entity_table is None
    loaders = ghmfc_shim.create_datasets()
    assert all(type(ld.dataset) is GhmfcData for ld in loaders)
    batch = next(iter(loaders[0]))
    assert batch[5].shape == (3, 4, 6, 16) and batch[5].dtype == torch.float32 and batch[6].shape == (3, 4, 6)
    monkeypatch.setenv("DRIN_GHMFC_TABLE", "0")
    assert type(ghmfc_shim.create_datasets()[0].dataset) is GhmfcData
    monkeypatch.setenv("DRIN_GHMFC_TABLE", "1")
    loaders = ghmfc_shim.create_datasets()
    assert all(type(ld.dataset) is IndexedGhmfcData for ld in loaders)
    model = ghmfc_shim.Model()
    assert model.entity_table is not None and model.entity_table.text.shape == (9, 6, 16)
    setattr(args, "mention_final_layer_name", "none")
    variant = ghmfc_shim.Model()
    assert isinstance(variant, VariantModel) and variant.entity_table is not None
    setattr(args, "dataset_name", "wikidiverse")
    with pytest.raises(ValueError, match="wikimel layout only"):
        ghmfc_shim.Model()
