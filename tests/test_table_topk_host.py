"""CPU-side checks of the cosine top-k against the whole table: the six entry points are exported, bound
and declared with the ABI still 12, every argument check fires before a launch with the right status and message, the workspace
query is aligned, monotone and refuses what would overflow, the layout self-check passes, `link_recall` counts what it says and
`link` refuses a model on the host."""
import ctypes as C
import os

import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc_table import LinkResult, TableForm
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantModel
from drin_amd.metrics import link_recall
from drin_amd.model import EntityTable

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
NEW_INT = ("drin_row_inv_norms", "drin_topk_update", "drin_table_topk", "drin_ghmfc_mention_forward")
NEW_SIZE = ("drin_table_topk_workspace_bytes", "drin_ghmfc_mention_forward_workspace_bytes")
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
    assert "table_topk.hip" in __import__("drin_amd.build", fromlist=["SOURCES"]).SOURCES
    assert f"#define DRIN_TOPK_SLICE {_lib.TOPK_SLICE}" in header and "THE ORDERING CONTRACT" in header
    for name in ("link",):
        assert hasattr(TableForm, name) and hasattr(TrainableModel, name) and hasattr(VariantModel, name)


def test_row_inv_norms_validates_on_host():
    lib, who = _lib.load(), "drin_row_inv_norms"

    def run(rows=ONE, E=9, width=16, eps=1e-8, out=ONE):
        return lib.drin_row_inv_norms(rows, E, width, eps, out, None)

    assert run(rows=None) == _lib.E_NULL and last() == f"{who}: rows is NULL"
    assert run(rows=ODD) == _lib.E_ALIGN and last() == f"{who}: rows is not 16-byte aligned"
    assert run(out=None) == _lib.E_NULL and last() == f"{who}: out is NULL"
    assert run(out=C.c_void_p(18)) == _lib.E_ALIGN and "out is not 4-byte aligned" in last()
    for E in (0, -3):
        assert run(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()
    for width in (0, 6, -4):
        assert run(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
    for eps in (0.0, -1.0, float("nan")):
        assert run(eps=eps) == _lib.E_SHAPE and "eps must be positive" in last()


def test_topk_update_validates_on_host():
    lib, who = _lib.load(), "drin_topk_update"

    def run(block=ONE, ld=4, batch=3, cols=10, base=0, inv=ONE, k=5, keys=ONE, rows=ONE, scratch=ONE, nbytes=BIG, first=1, ok=ONE,
            orows=ONE):
        return lib.drin_topk_update(block, ld, batch, cols, base, inv, k, keys, rows, scratch, nbytes, first, ok, orows, None)

    for name, arg in (("block", "block"), ("state_keys", "keys"), ("state_rows", "rows"), ("scratch", "scratch")):
        assert run(**{arg: None}) == _lib.E_NULL and last() == f"{who}: {name} is NULL"
        assert run(**{arg: ODD}) == _lib.E_ALIGN and last() == f"{who}: {name} is not 16-byte aligned"
    assert run(inv=C.c_void_p(18)) == _lib.E_ALIGN and "col_inv_norms" in last()
    assert run(orows=ODD) == _lib.E_ALIGN and "out_rows 8-byte" in last()
    assert run(ok=None) == _lib.E_NULL and run(orows=None) == _lib.E_NULL and "go together" in last()
    for batch in (0, 65536):
        assert run(batch=batch, ld=65536) == _lib.E_SHAPE and f"batch = {batch}" in last()
    for k in (0, 257, -1):
        assert run(k=k) == _lib.E_SHAPE and f"k = {k}" in last()
    assert run(cols=-1) == _lib.E_SHAPE and "cols = -1" in last()
    assert run(cols=1 << 31) == _lib.E_SHAPE and "cols" in last()
    assert run(base=-1) == _lib.E_SHAPE and "col_base = -1" in last()
    for ld in (3, 6, 0, -4):                                            # batch 3: a multiple of 4 from 4 up
        assert run(ld=ld) == _lib.E_SHAPE and f"ld = {ld}" in last()
    assert run(batch=5, ld=4) == _lib.E_SHAPE and "ld = 4" in last()
    # the finishing call: cols = 0 reads neither block nor scratch, needs the outputs and a state
    assert run(cols=0, first=1, block=None, scratch=None) == _lib.E_SHAPE and "finishing call" in last()
    assert run(cols=0, first=0, ok=None, orows=None, block=None, scratch=None) == _lib.E_SHAPE and "finishing call" in last()
    # scratch: ceil(cols / slice) * batch * kp * 8 bytes, kp = 64 / 128 / 256
    S = _lib.TOPK_SLICE
    for cols, k, need in ((10, 5, 3 * 64 * 8), (S, 64, 3 * 64 * 8), (S + 1, 65, 2 * 3 * 128 * 8), (2 * S + 5, 256, 3 * 3 * 256 * 8)):
        assert run(cols=cols, k=k, nbytes=need - 1) == _lib.E_WORKSPACE and f"scratch {need - 1} bytes < {need}" in last()


def test_table_topk_validates_on_host():
    lib, who = _lib.load(), "drin_table_topk"

    def run(x=ONE, rows=ONE, inv=ONE, E=300, batch=3, width=16, k=20, eps=1e-8, precision=_lib.PREC_BF16X3, chunk=64, ws=ONE,
            nbytes=BIG, scores=ONE, orows=ONE):
        return lib.drin_table_topk(x, rows, inv, E, batch, width, k, eps, precision, chunk, ws, nbytes, scores, orows, None)

    for name, arg in (("x", "x"), ("rows", "rows"), ("row_inv_norms", "inv"), ("workspace", "ws")):
        assert run(**{arg: None}) == _lib.E_NULL and last() == f"{who}: {name} is NULL"
        assert run(**{arg: ODD}) == _lib.E_ALIGN and last() == f"{who}: {name} is not 16-byte aligned"
    assert run(scores=None) == _lib.E_NULL and run(orows=None) == _lib.E_NULL and "out_scores / out_rows is NULL" in last()
    assert run(scores=C.c_void_p(18)) == _lib.E_ALIGN and run(orows=ODD) == _lib.E_ALIGN and "out_rows 8-byte" in last()
    for E in (0, -1):
        assert run(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()
    for batch in (0, 65536, -2):
        assert run(batch=batch) == _lib.E_SHAPE and f"batch = {batch}" in last()
    for width in (0, 6, -4):
        assert run(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
    for k in (0, 257):
        assert run(k=k) == _lib.E_SHAPE and f"k = {k}" in last()
    assert run(E=19, k=20) == _lib.E_SHAPE and last() == f"{who}: k = 20 exceeds num_entities = 19"
    assert run(precision=_lib.PREC_BF16X3_ALL) == _lib.E_UNSUPPORTED and "precision 3" in last()
    assert run(chunk=-1) == _lib.E_SHAPE and "chunk_entities = -1" in last()
    assert run(E=1 << 40, chunk=1 << 31) == _lib.E_SHAPE and "chunk_entities" in last()
    need = lib.drin_table_topk_workspace_bytes(3, 300, 16, 20, 64)
    assert need > 0 and run(nbytes=need - 1) == _lib.E_WORKSPACE and f"workspace {need - 1} bytes < {need}" in last()


def test_workspace_bytes_are_aligned_monotone_and_refuse_overflow():
    need = _lib.load().drin_table_topk_workspace_bytes
    base = need(3, 300, 16, 20, 64)
    # xpad 4 x 16, block 64 x 4, keys 3 x 64, rows and one slice's lists 3 x 64 x 2 each, scores 3 x 64: floats, each region
    # rounded up to 256 bytes
    r256 = lambda floats: -(-floats * 4 // 256) * 256   # noqa: E731
    assert base == r256(64) + r256(256) + r256(192) + 2 * r256(384) + r256(192)
    for args in ((3, 300, 16, 20, 64), (64, 65536, 768, 100, 0), (4096, 1000000, 768, 100, 0), (65535, 1000000, 768, 256, 0), (1, 1, 4, 1, 0)):
        assert need(*args) > 0 and need(*args) % 256 == 0, args
    assert need(3, 300, 16, 20, 64) < need(4, 300, 16, 20, 64) < need(5, 300, 16, 20, 64) <= need(8, 300, 16, 20, 64) < need(300, 300, 16, 20, 64)
    assert need(3, 300, 16, 20, 64) == need(3, 300, 16, 64, 64) < need(3, 300, 16, 65, 64) == need(3, 300, 16, 128, 64) < need(3, 300, 16, 129, 64)
    assert need(3, 300, 16, 20, 1) < need(3, 300, 16, 20, 64) < need(3, 300, 16, 20, 256) < need(3, 300, 16, 20, 300) == need(3, 300, 16, 20, 4000)
    assert need(3, 300, 16, 20, 0) == need(3, 300, 16, 20, 300)          # the default chunk covers a small table whole
    # the default chunk bounds the block of dot products to 256 MiB: the rest of the workspace at B = 4096, E = 1 M, k = 100
    assert (256 << 20) - 256 * 4096 * 4 < need(4096, 1000000, 768, 100, 0) - need(4096, 1000000, 768, 100, 1) <= (256 << 20) + (64 << 20)
    for bad, text in (((0, 300, 16, 20, 0), "batch = 0"), ((3, 0, 16, 20, 0), "num_entities = 0"), ((3, 300, 18, 20, 0), "multiple of 4"),
                      ((3, 300, 16, 301, 0), "k = 301"), ((3, 19, 16, 20, 0), "exceeds num_entities"), ((3, 300, 16, 20, -5), "negative"),
                      ((65535, 1 << 50, 16, 256, 1 << 40), "out of range"), ((3, 1 << 52, 16, 20, 0), "num_entities")):
        assert need(*bad) == 0 and text in last(), bad


def test_mention_forward_validates_on_host():
    lib, who = _lib.load(), "drin_ghmfc_mention_forward"
    params = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[16] * 52))
    batch = _lib.DrinGhmfcBatchC(ONE, ONE, ONE, None, None)            # entity_feature / entity_mask are not read

    def config(B=3, N=4, D=16, R=32, L=12, P=3, H=2, T=0, precision=_lib.PREC_BF16X3):
        return _lib.DrinGhmfcConfigC(batch=B, num_candidates=N, embed_dim=D, image_dim=R, mention_tokens=L, image_regions=P, num_heads=H,
                                     entity_tokens=T, precision=precision, layer_norm_eps=1e-5, cosine_eps=1e-8)

    def run(cfg=None, bt=batch, pc=params, ws=ONE, nbytes=BIG, men=ONE):
        cfg = cfg or config()
        return lib.drin_ghmfc_mention_forward(C.byref(cfg), C.byref(bt), C.byref(pc), ws, nbytes, men, None)

    assert lib.drin_ghmfc_mention_forward(None, C.byref(batch), C.byref(params), ONE, BIG, ONE, None) == _lib.E_NULL
    assert run(men=None) == _lib.E_NULL and last().startswith(who) and run(ws=None) == _lib.E_NULL
    assert run(bt=_lib.DrinGhmfcBatchC(None, ONE, ONE, None, None)) == _lib.E_NULL and "mention tensor" in last()
    broken = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*([16] * 51 + [0])))
    assert run(pc=broken) == _lib.E_NULL and f"{who}: parameter 51" in last()
    assert run(cfg=config(D=18)) == _lib.E_SHAPE and "multiples of 4" in last()
    assert run(cfg=config(B=0)) == _lib.E_SHAPE and run(cfg=config(L=513)) == _lib.E_UNSUPPORTED
    assert run(cfg=config(precision=7)) == _lib.E_UNSUPPORTED
    assert run(nbytes=1024) == _lib.E_WORKSPACE and f"{who}: workspace 1024 bytes <" in last()
    assert run(ws=ODD) == _lib.E_ALIGN and run(men=ODD) == _lib.E_ALIGN and who in last()
    # the candidate side is not read: any num_candidates / entity_tokens, the same bytes, and no entity regions
    need = lib.drin_ghmfc_mention_forward_workspace_bytes
    size = need(C.byref(config()))
    assert size > 0 and size % 256 == 0
    assert size == need(C.byref(config(N=0))) == need(C.byref(config(N=70000, T=9999)))
    assert run(cfg=config(N=0), nbytes=size - 1) == _lib.E_WORKSPACE
    c300 = config(B=300)
    assert need(C.byref(c300)) < lib.drin_ghmfc_workspace_bytes(C.byref(c300)) and need(C.byref(c300)) > size
    assert need(None) == 0 and need(C.byref(config(D=18))) == 0


def test_layout_selfcheck_passes():
    """drin_host_selftest walks the top-k workspace at the tiny shape, the reference width and E = 1 M at B = 4096 (api.hip)."""
    lib = _lib.load()
    assert lib.drin_host_selftest() == _lib.OK, last()
    src = open(os.path.join(REPO, "drin_amd", "csrc", "api.hip")).read()
    assert "table_topk_layout_selfcheck(3, 300, 16, k, 64)" in src and "table_topk_layout_selfcheck(4096, 1000000, 768, k, 0)" in src


def test_link_recall_on_hand_made_rows():
    rows = torch.tensor([[4, 2, 9], [7, 7, 1], [0, 5, 3], [8, 6, 2]])
    answers = torch.tensor([4, 1, 6, 2])                                # rank 1, rank 3, absent, rank 3
    assert link_recall(rows, answers, [1, 2, 3]) == [0.25, 0.25, 0.75]
    assert link_recall(rows, rows[:, 0], [1]) == [1.0] and link_recall(rows, torch.full((4,), -1), [3]) == [0.0]
    assert link_recall(rows.numpy(), answers.tolist(), (3,)) == [0.75]
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        link_recall(rows, answers, [4])
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        link_recall(rows, answers, [0])
    with pytest.raises(ValueError, match="answer_rows"):
        link_recall(rows, answers[:3], [1])
    assert LinkResult._fields == ("scores", "rows")


def test_link_refuses_on_the_host():
    from tests.test_ghmfc_host import cfg_for
    model = TrainableModel(cfg_for("wm_b3"))
    D = model.cfg.embed_dim
    table = EntityTable(torch.zeros(5, 6, D), torch.ones(5, 6, dtype=torch.int64), None, None, None)
    mention = [torch.zeros(3, 12, D), torch.ones(3, 12, dtype=torch.int64), torch.ones(3), torch.ones(3), torch.zeros(3, 3, 32)]
    with pytest.raises(RuntimeError, match="eval\\(\\) only"):
        model.link(mention, 2, table)
    model.eval()
    with pytest.raises(ValueError, match="none attached"):
        model.link(mention, 2)
    with pytest.raises(ValueError, match="five mention-side items"):
        model.link(mention[:4], 2, table)
    for k in (0, 257):
        with pytest.raises(ValueError, match=f"k = {k} is not in"):
            model.link(mention, k, table)
    with pytest.raises(ValueError, match="k = 6 exceeds the table's 5 entities"):
        model.link(mention, 6, table)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        model.link(mention, 2, EntityTable(table.text.bfloat16(), table.mask, None, None, None))
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(mention, 2, table)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.attach_entity_table(table).link(mention + [0, 0, 0], 2)
    assert model.entity_cache_builds == 0
