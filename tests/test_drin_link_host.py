"""CPU-side checks of DRIN behind a first stage: `drin_cross_modal_edges` and `drin_rank_rows` are exported,
bound and declared with the ABI still 12, refuse every bad argument on the host with an error naming the entry point, their
kernels use no scratch; `EntityTable.set_clip`, `Model.link` and `EncoderModel.link` raise as documented; the restated order
agrees with the contract of tests/test_gpu_table_topk.py; and the oracle margins the GPU link test relies on hold."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig
from drin_amd.model import EntityTable, IndexedBatch, Model
from oracle.cases import TINY
from tests.drin_link_restatement import CASES, K_LINK, TOL, canonical, expected_rank, link_case, near_threshold, rank_order
from tests.test_gpu_table_topk import contract_order

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
ONE = C.c_void_p(16)      # aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)      # 4-byte aligned only
EDGES, RANK = "drin_cross_modal_edges", "drin_rank_rows"


def last():
    return _lib.load().drin_last_error().decode()


def test_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in (EDGES, RANK):
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    assert "preprocess/clip.py:158-172" in header and "model.py:203" in header
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12
    assert "cross_edges.hip" in __import__("drin_amd.build", fromlist=["SOURCES"]).SOURCES


def test_cross_modal_edges_validates_on_host():
    lib = _lib.load()

    def edges(m_image=ONE, m_text=ONE, t_text=ONE, t_image=ONE, index=ONE, E=9, batch=2, n=4, width=16, miet=ONE, mtei=ONE, status=ONE):
        return lib.drin_cross_modal_edges(m_image, m_text, t_text, t_image, index, E, batch, n, width, 100.0, 1e-8, miet, mtei, status, None)

    for arg in ("m_image", "m_text", "t_text", "t_image", "miet", "mtei"):                   # a half-given edge
        assert edges(**{arg: None}) == _lib.E_NULL and last().startswith(EDGES + ": ") and "NULL" in last(), arg
    assert edges(m_image=None, t_text=None, miet=None, m_text=None, t_image=None, mtei=None) == _lib.E_NULL and "both edges" in last()
    assert edges(index=None) == _lib.E_NULL and last() == f"{EDGES}: index is NULL"
    for arg in ("m_image", "m_text", "t_text", "t_image"):
        assert edges(**{arg: ODD}) == _lib.E_ALIGN and last().startswith(EDGES + ": ") and "not 16-byte aligned" in last(), arg
    for arg in ("miet", "mtei", "status"):
        assert edges(**{arg: C.c_void_p(18)}) == _lib.E_ALIGN and last().startswith(EDGES + ": ") and "4-byte aligned" in last(), arg
    assert edges(index=ODD) == _lib.E_ALIGN and "index must be 8-byte" in last()
    for width in (0, 6, -4, 514):
        assert edges(width=width) == _lib.E_SHAPE and last().startswith(EDGES + ": ") and "multiple of 4" in last()
    for batch in (0, 65536):
        assert edges(batch=batch) == _lib.E_SHAPE and last().startswith(EDGES + ": ") and f"batch = {batch}" in last()
    for n in (0, 65536):
        assert edges(n=n) == _lib.E_SHAPE and f"num_candidates = {n}" in last()
    for E in (0, -3):
        assert edges(E=E) == _lib.E_SHAPE and f"num_entities = {E}" in last()
    # one edge alone passes the pointer checks: the next refusal is the shape's
    assert edges(m_text=None, t_image=None, mtei=None, batch=0) == _lib.E_SHAPE and "batch = 0" in last()
    assert edges(m_image=None, t_text=None, miet=None, batch=0) == _lib.E_SHAPE and "batch = 0" in last()


def test_rank_rows_validates_on_host():
    lib = _lib.load()

    def rank(scores=ONE, rows=ONE, batch=2, n=8, k=3, out_scores=ONE, out_rows=ONE, out_slots=ONE):
        return lib.drin_rank_rows(scores, rows, batch, n, k, out_scores, out_rows, out_slots, None)

    for arg in ("scores", "rows", "out_scores", "out_rows"):
        assert rank(**{arg: None}) == _lib.E_NULL and last() == f"{RANK}: {arg} is NULL"
    for arg in ("scores", "out_scores", "out_slots"):
        assert rank(**{arg: C.c_void_p(18)}) == _lib.E_ALIGN and last().startswith(RANK + ": ") and "aligned" in last(), arg
    for arg in ("rows", "out_rows"):
        assert rank(**{arg: ODD}) == _lib.E_ALIGN and last().startswith(RANK + ": ") and "8-byte aligned" in last(), arg
    for batch in (0, 65536):
        assert rank(batch=batch) == _lib.E_SHAPE and last().startswith(RANK + ": ") and f"batch = {batch}" in last()
    assert rank(n=4097, k=1) == _lib.E_SHAPE and last().startswith(RANK + ": ") and "n = 4097" in last()
    assert rank(n=0) == _lib.E_SHAPE and "n = 0" in last()
    assert rank(k=0) == _lib.E_SHAPE and "k = 0" in last()
    assert rank(n=8, k=9) == _lib.E_SHAPE and last() == f"{RANK}: k = 9 exceeds n = 8"


def test_new_kernels_use_no_scratch():
    from drin_amd import build, resources
    build.build(verbose=False)
    rows = [k for k in resources.kernel_resources() if "k_cross_modal_edges" in k["name"] or "k_rank_rows" in k["name"]]
    names = " ".join(k["name"] for k in rows)
    assert "k_rank_rows" in names and sum("k_cross_modal_edges" in k["name"] for k in rows) >= 2
    for k in rows:
        print(k["name"], k.get("vgpr_count"), k.get("sgpr_count"), k.get("group_segment_fixed_size"))
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
    assert all(k.get("group_segment_fixed_size", 0) == 0 for k in rows if "cross_modal" in k["name"])      # no LDS either


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def _cpu_case(name="wm"):
    c = link_case(name)
    model = Model(c["cfg"]).eval()
    return c, model


def test_set_clip_refuses_and_follows_the_table():
    c = link_case("wm")
    t = c["table"]
    table = EntityTable(t.text, t.mask, t.image, t.object, t.object_score)
    E = table.num_entities
    assert table.clip_text is None and table.clip_image is None
    key = table._table_key()
    good = torch.randn(E, 8)
    with pytest.raises(ValueError, match="float32"):
        table.set_clip(good.double(), good)
    with pytest.raises(ValueError, match="float32"):
        table.set_clip(good, good.half())
    with pytest.raises(ValueError, match="expected"):
        table.set_clip(good[:-1], good)
    with pytest.raises(ValueError, match="expected"):
        table.set_clip(good, torch.randn(E + 1, 8))
    with pytest.raises(ValueError, match="multiple of 4"):
        table.set_clip(torch.randn(E, 6), torch.randn(E, 6))
    assert table.clip_text is None
    assert table.set_clip(good, good + 1) is table and torch.equal(table.clip_text, good) and torch.equal(table.clip_image, good + 1)
    assert table._table_key() == key                                   # the per-entity cache does not depend on them
    moved = table.to("cpu")
    assert torch.equal(moved.clip_text, good) and torch.equal(moved.clip_image, good + 1)
    table.invalidate()
    table.enable_cache(False)
    assert table.clip_text is not None                                  # dropped by nothing else


def test_model_link_raises_as_documented():
    c, model = _cpu_case()
    N = c["cfg"].num_candidates_model
    args = (c["mention"], c["table"], K_LINK, c["clip_image"], c["clip_text"])
    q, r = torch.randn(3, 8), torch.randn(c["table"].num_entities, 8)
    with pytest.raises(ValueError, match="exactly one"):
        model.link(*args)
    with pytest.raises(ValueError, match="exactly one"):
        model.link(*args, candidates=c["candidates"], queries=q, rows=r)
    with pytest.raises(ValueError, match="go together"):
        model.link(*args, queries=q)
    with pytest.raises(ValueError, match=f"expected \\[B, {N}\\]"):
        model.link(*args, candidates=c["candidates"][:, :-1])
    with pytest.raises(ValueError, match="k = "):
        model.link(c["mention"], c["table"], N + 1, c["clip_image"], c["clip_text"], candidates=c["candidates"])
    with pytest.raises(ValueError, match="k = "):
        model.link(c["mention"], c["table"], 0, c["clip_image"], c["clip_text"], candidates=c["candidates"])
    t = c["table"]
    bare = EntityTable(t.text, t.mask, t.image, t.object, t.object_score)
    with pytest.raises(ValueError, match="no CLIP rows"):
        model.link(c["mention"], bare, K_LINK, c["clip_image"], c["clip_text"], candidates=c["candidates"])
    with pytest.raises(ValueError, match="no CLIP rows"):
        IndexedBatch.from_clip(c["mention"], bare, c["candidates"], c["clip_image"], c["clip_text"])
    with pytest.raises(RuntimeError, match="GPU only"):                 # everything else is in order: no CPU fallback
        model.link(*args, candidates=c["candidates"])
    with pytest.raises(RuntimeError, match="eval"):
        model.train().link(*args, candidates=c["candidates"])
    wide = Model(DrinConfig(num_candidates_data=300, **TINY)).eval()    # N = 301: no cosine first stage lists that many
    with pytest.raises(ValueError, match="at most 256"):
        wide.link(*args, queries=q, rows=r)


def test_encoder_model_refuses_link():
    from drin_amd.drin_encoders import EncoderModel
    model = Model(DrinConfig(mention_final_layer_name="none", **TINY))
    assert isinstance(model, EncoderModel)
    with pytest.raises(NotImplementedError, match="section 22"):
        model.link(None, None, 1, None, None)


def test_synth_clip_rows_are_seeded_and_leave_the_other_draws_alone():
    cfg = DrinConfig(**TINY)
    before = synth.make_batch(cfg, 2, 3)
    a, b = synth.make_clip_rows(7, 2, 8, seed=3), synth.make_clip_rows(7, 2, 8, seed=3)
    assert [tuple(t.shape) for t in a] == [(7, 8), (7, 8), (2, 8), (2, 8)] and all(t.dtype == torch.float32 for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], synth.make_clip_rows(7, 2, 8, seed=4)[0])
    assert not torch.equal(a[0], a[1]) and 0.5 < float(torch.cat(a).std()) < 1.5
    assert all(torch.equal(x, y) for x, y in zip(before, synth.make_batch(cfg, 2, 3)))


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restated_order_agrees_with_the_contract_without_duplicate_rows():
    """The order `drin_rank_rows` is held to on the GPU (tests/test_gpu_drin_link.py): the header states the slot rule beside the
    entry point, and the restatement of it is the contract of section 24 wherever that one speaks."""
    header = open(HEADER).read()
    decl = header[header.index("the first k of n (score, row) pairs"):header.index("DRIN_API int drin_rank_rows(")]
    assert "lower slot" in decl and "canonical" in decl and RANK in _lib.EXPORTS and hasattr(_lib.load(), RANK)
    r = np.random.default_rng(11)
    for n in (1, 2, 17, 101):
        scores = np.round(r.standard_normal(n), 1).astype(np.float32)           # many ties
        for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan)[:n]):
            scores[(3 * i) % n] = v
        rows = r.permutation(10 * n)[:n].astype(np.int64)
        assert np.array_equal(rank_order(scores, rows), contract_order(scores, rows)), n
    # and the slot rule, where the contract is silent: equal scores on equal rows keep the input order
    scores = np.array([1.0, 2.0, 1.0, -0.0, 0.0, np.nan, 1.0], dtype=np.float32)
    rows = np.array([5, 9, 5, 3, 3, 1, 4], dtype=np.int64)
    assert rank_order(scores, rows).tolist() == [1, 6, 0, 2, 3, 4, 5]
    bits, out_rows, slots = expected_rank(scores[None], rows[None], 7)
    assert out_rows.tolist() == [[9, 4, 5, 5, 3, 3, 1]] and slots.tolist() == [[1, 6, 0, 2, 3, 4, 5]]
    assert bits[0, 4] == 0 and bits[0, 5] == 0 and bits[0, 6] == 0x7FC00000
    assert canonical(np.array([-0.0, -np.nan], dtype=np.float32)).tolist() == [0, 0x7FC00000]


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_margins_of_the_link_cases(name):
    """What `test_gpu_drin_link.py` relies on, from the fp64 oracle alone: at the k-th score of every mention at most 2 other
    candidates lie within the WIDER bar, no candidate row repeats inside a mention, and the scores are finite."""
    c = link_case(name)
    ref, cand = c["ref"], c["candidates"]
    assert ref.dtype == torch.float64 and tuple(ref.shape) == tuple(cand.shape) and torch.isfinite(ref).all()
    assert all(len(set(row.tolist())) == cand.shape[1] for row in cand)
    worst = near_threshold(ref, K_LINK, max(TOL.values()))
    print(f"{name}: at most {worst} other candidates within {max(TOL.values()):g} of the k-th oracle score")
    assert worst <= 2
