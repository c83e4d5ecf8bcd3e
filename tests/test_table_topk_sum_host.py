"""CPU-side checks of the summed-cosine first stage: `drin_table_topk_sum`, its size query and
`drin_topk_combine` are exported, bound and declared with the ABI still 12; every bad argument is refused on the host, before a
launch, with an error naming the entry point; the workspace size follows its rules; the selftest walks the layouts; the new
kernels use no scratch; `Model.link(first_stage="edges")` raises as documented and the earlier calls raise what they raised;
and the margins the GPU selection test relies on hold on the fp64 restatement."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

from drin_amd import _lib
from drin_amd.drin_encoders import EncoderModel
from drin_amd.config import DrinConfig
from drin_amd.model import Model
from oracle.cases import TINY
from tests.drin_link_restatement import K_LINK, link_case
from tests.table_topk_sum_restatement import CASES, near_threshold, sum_case, tol_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
ONE = 16                  # aligned, never dereferenced: every check below fails before a launch
ODD = 20                  # 4-byte aligned only
SUM, SIZE, COMBINE = "drin_table_topk_sum", "drin_table_topk_sum_workspace_bytes", "drin_topk_combine"


def last():
    return _lib.load().drin_last_error().decode()


def terms_of(*specs):
    """a drin_topk_term array of (width, weight) or (width, weight, x, rows, inv) specs; pointers default to ONE"""
    arr = (_lib.DrinTopkTermC * max(len(specs), 1))()
    for s, spec in enumerate(specs):
        width, weight, x, rows, inv = (tuple(spec) + (ONE, ONE, ONE))[:5] if len(spec) == 2 else spec
        arr[s].x, arr[s].rows, arr[s].row_inv_norms, arr[s].width, arr[s].weight = x, rows, inv, width, weight
    return arr


def test_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in (SUM, COMBINE):
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    assert hasattr(lib, SIZE) and SIZE in _lib.EXPORTS and f"DRIN_API size_t {SIZE}(" in header
    assert "typedef struct drin_topk_term" in header and "#define DRIN_TOPK_MAX_TERMS 4" in header and _lib.TOPK_MAX_TERMS == 4
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12
    assert "DESIGN.md section 33" in header


def test_term_mirror_matches_the_header_layout(tmp_path):
    fields = [f for f, _ in _lib.DrinTopkTermC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(drin_topk_term));']
    lines += [f'  printf("{f} %zu\\n", offsetof(drin_topk_term, {f}));' for f in fields] + ['  return 0;', '}']
    src, exe = tmp_path / "term.c", tmp_path / "term"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.DrinTopkTermC) == 32
    for f in fields:
        assert int(got[f]) == getattr(_lib.DrinTopkTermC, f).offset, f


def test_table_topk_sum_validates_on_host():
    lib = _lib.load()

    def call(terms=None, n=None, E=300, batch=3, k=20, precision=_lib.PREC_BF16X3, chunk=0, ws=ONE, ws_bytes=1 << 40, scores=ONE, rows=ONE):
        terms = terms_of((16, 1.0), (8, 1.0), (8, 1.0)) if terms is None else terms
        n = len(terms) if n is None else n
        return lib.drin_table_topk_sum(terms, n, E, batch, k, 1e-8, precision, chunk, ws, ws_bytes, scores, rows, None)

    assert lib.drin_table_topk_sum(None, 1, 300, 3, 20, 1e-8, 1, 0, ONE, 1 << 40, ONE, ONE, None) == _lib.E_NULL
    assert last() == f"{SUM}: terms is NULL"
    for n in (0, 5, -1):
        assert call(n=n) == _lib.E_SHAPE and last().startswith(SUM + ": ") and f"num_terms = {n}" in last()
    for bad in (math.inf, -math.inf, math.nan):
        assert call(terms_of((16, 1.0), (8, bad))) == _lib.E_SHAPE and last() == f"{SUM}: term 1: weight is not finite"
    assert call(terms_of((16, 0.0), (8, 0.0))) == _lib.E_SHAPE and last().startswith(SUM + ": ") and "no live term" in last()
    for width in (0, 6, -4, 514):
        assert call(terms_of((16, 1.0), (width, 2.0))) == _lib.E_SHAPE and last().startswith(f"{SUM}: term 1: ") and "multiple of 4" in last()
    for i, name in enumerate(("x", "rows", "row_inv_norms")):
        ptrs = [ONE, ONE, ONE]
        ptrs[i] = 0
        assert call(terms_of((16, 1.0), (8, 1.0, *ptrs))) == _lib.E_NULL and last() == f"{SUM}: term 1: {name} is NULL"
        ptrs[i] = ODD
        assert call(terms_of((8, 1.0, *ptrs))) == _lib.E_ALIGN and last() == f"{SUM}: term 0: {name} is not 16-byte aligned"
    # a dropped term's pointers and width are not looked at
    assert call(terms_of((16, 1.0), (6, 0.0, 0, 0, 0)), batch=0) == _lib.E_SHAPE and "batch = 0" in last()
    assert call(ws=None) == _lib.E_NULL and "workspace is NULL" in last()
    assert call(ws=ODD) == _lib.E_ALIGN and last().startswith(SUM + ": ")
    assert call(scores=None) == _lib.E_NULL and call(rows=None) == _lib.E_NULL and "out_scores / out_rows" in last()
    assert call(scores=18) == _lib.E_ALIGN and call(rows=ODD) == _lib.E_ALIGN and "8-byte aligned" in last()
    for batch in (0, 65536):
        assert call(batch=batch) == _lib.E_SHAPE and last().startswith(SUM + ": ") and f"batch = {batch}" in last()
    for k in (0, 257):
        assert call(k=k) == _lib.E_SHAPE and last().startswith(SUM + ": ") and f"k = {k}" in last()
    assert call(E=10, k=11) == _lib.E_SHAPE and last() == f"{SUM}: k = 11 exceeds num_entities = 10"
    assert call(E=0) == _lib.E_SHAPE and "num_entities = 0" in last()
    for precision in (2, 3, 5, 7):
        assert call(precision=precision) == _lib.E_UNSUPPORTED and last().startswith(SUM + ": ")
    assert call(chunk=-1) == _lib.E_SHAPE and "chunk_entities = -1 is negative" in last()
    assert call(E=1 << 40, chunk=(1 << 30) + 1) == _lib.E_SHAPE and "out of range" in last()
    assert call(ws_bytes=64) == _lib.E_WORKSPACE and last().startswith(SUM + ": workspace 64 bytes < ")


def test_topk_combine_validates_on_host():
    lib = _lib.load()

    def call(n=2, blocks=(ONE, ONE), invs=(ONE, ONE), scales=(ONE, ONE), weights=(1.0, 1.0), ld=4, batch=3, cols=5, out=ONE, null=None):
        arrays = [(C.c_void_p * 4)(*p) for p in (blocks, invs, scales)]
        w = (C.c_float * 4)(*weights)
        args = [None if null == i else a for i, a in enumerate(arrays)] + [None if null == 3 else w]
        return lib.drin_topk_combine(*args, n, ld, batch, cols, out, None)

    for i, name in enumerate(("blocks", "col_inv_norms", "row_scales", "weights")):
        assert call(null=i) == _lib.E_NULL and last() == f"{COMBINE}: {name} is NULL"
    assert call(out=None) == _lib.E_NULL and last() == f"{COMBINE}: out is NULL"
    for n in (0, 5):
        assert call(n=n) == _lib.E_SHAPE and f"num_terms = {n}" in last()
    assert call(blocks=(ONE, None)) == _lib.E_NULL and last() == f"{COMBINE}: term 1: blocks is NULL"
    assert call(invs=(None, ONE)) == _lib.E_NULL and last() == f"{COMBINE}: term 0: col_inv_norms is NULL"
    assert call(scales=(ONE, None)) == _lib.E_NULL and "term 1: row_scales is NULL" in last()
    assert call(blocks=(ODD, ONE)) == _lib.E_ALIGN and call(scales=(ONE, ODD)) == _lib.E_ALIGN and call(invs=(ONE, 18)) == _lib.E_ALIGN
    assert call(invs=(ODD, ONE), batch=0) == _lib.E_SHAPE                 # a column factor is read 4 bytes at a time
    assert call(out=ODD) == _lib.E_ALIGN and last() == f"{COMBINE}: out is not 16-byte aligned"
    assert call(weights=(1.0, math.nan)) == _lib.E_SHAPE and "term 1: weight is not finite" in last()
    for batch in (0, 65536):
        assert call(batch=batch, ld=65536) == _lib.E_SHAPE and f"batch = {batch}" in last()
    assert call(cols=0) == _lib.E_SHAPE and "cols = 0" in last()
    for ld in (0, 2, 6, -4, 1 << 31):
        assert call(ld=ld) == _lib.E_SHAPE and last().startswith(f"{COMBINE}: ld = {ld} ")
    assert call(batch=5, ld=4) == _lib.E_SHAPE


def test_workspace_size_follows_its_rules():
    lib = _lib.load()

    def size(specs, batch=64, E=65536, k=100, chunk=0):
        t = terms_of(*specs)
        return lib.drin_table_topk_sum_workspace_bytes(t, len(specs), batch, E, k, chunk)

    edges = [(768, 1.0), (512, 1.0), (512, 1.0)]
    base = size(edges)
    assert base > 0 and base % 256 == 0
    # monotone in S (explicit chunk: the default one shrinks with S), B and k
    assert 0 < size(edges[:1], chunk=512) < size(edges[:2], chunk=512) < size(edges, chunk=512) < size(edges + [(768, 2.0)], chunk=512)
    assert size(edges, batch=64, chunk=512) < size(edges, batch=65, chunk=512) < size(edges, batch=128, chunk=512)
    assert size(edges, k=1) == size(edges, k=64) < size(edges, k=65) == size(edges, k=128) < size(edges, k=129)
    # a dropped term takes no room and its width and pointers are not looked at
    assert size(edges + [(6, 0.0, 0, 0, 0)]) == base and size([(4, 0.0)] + edges) == base
    # the default chunk: a multiple of 256 rows whose live blocks together stay within 256 MiB - at B = 4096 and E = 1 M the three
    # blocks take 5 376 rows each, and the whole workspace stays under 256 MiB + the selection's lists
    big = size(edges, batch=4096, E=1000000, k=100)
    blocks = 3 * 5376 * 4096 * 4
    assert blocks <= 256 << 20 < 3 * (5376 + 256) * 4096 * 4 and blocks < big < blocks + (64 << 20)
    assert lib.drin_table_topk_sum_workspace_bytes(None, 1, 64, 65536, 100, 0) == 0 and last() == f"{SIZE}: terms is NULL"
    for bad, what in ((dict(batch=0), "batch = 0"), (dict(batch=65536), "batch = 65536"), (dict(k=0), "k = 0"), (dict(k=257), "k = 257"),
                      (dict(E=50), "exceeds num_entities"), (dict(chunk=-2), "negative"), (dict(E=1 << 40, chunk=(1 << 30) + 1), "out of range")):
        assert size(edges, **bad) == 0 and last().startswith(SIZE + ": ") and what in last(), bad
    assert size([(768, 1.0), (510, 1.0)]) == 0 and "term 1: width 510" in last()
    assert size([(768, 0.0)]) == 0 and "no live term" in last()
    assert size([(768, math.inf)]) == 0 and "not finite" in last()
    t = terms_of(*edges)
    for n in (0, 5):
        assert lib.drin_table_topk_sum_workspace_bytes(t, n, 64, 65536, 100, 0) == 0 and f"num_terms = {n}" in last()


def test_selftest_walks_the_sum_layouts():
    lib = _lib.load()
    assert lib.drin_host_selftest() == _lib.OK, lib.drin_last_error()
    # and the sizes those layouts give through the public query are the sums of their regions (each rounded up to 256 bytes)
    rounded = lambda floats: -(-floats // 64) * 64 * 4   # noqa: E731

    def expected(widths, B, E, k, chunk):
        Bp, kp, S = -(-B // 4) * 4, 64 if k <= 64 else (128 if k <= 128 else 256), len(widths)
        chunk = min(E, chunk or max(256, (256 << 20) // (S * Bp * 4) // 256 * 256))
        slices = -(-chunk // _lib.TOPK_SLICE)
        per_term = sum(rounded(Bp * d) + rounded(Bp) + rounded(chunk * Bp) for d in widths)
        return per_term + rounded(S * B * kp) + rounded(B * kp) + rounded(B * kp * 2) + rounded(slices * B * kp * 2) + rounded(B * kp)

    for widths, B, E, k, chunk in (((16, 8, 8), 3, 300, 20, 64), ((16, 8, 8), 3, 300, 20, 0), ((768, 512, 512), 4096, 1000000, 100, 0),
                                   ((16, 260, 4, 768), 9, 70000, 256, 0)):
        t = terms_of(*[(d, 1.0) for d in widths])
        assert lib.drin_table_topk_sum_workspace_bytes(t, len(widths), B, E, k, chunk) == expected(widths, B, E, k, chunk), (widths, B, E, k, chunk)


def test_new_kernels_use_no_scratch_and_no_lds():
    from drin_amd import build, resources
    build.build(verbose=False)
    rows = [k for k in resources.kernel_resources() if "k_topk_combine" in k["name"] or "k_weighted_cosine_sum" in k["name"]]
    names = " ".join(k["name"] for k in rows)
    assert sum("k_topk_combine" in k["name"] for k in rows) == 4 and "k_weighted_cosine_sum" in names
    for k in rows:
        print(k["name"], k.get("vgpr_count"), k.get("sgpr_count"))
        assert k["object"] == "table_topk.o"
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k.get("group_segment_fixed_size", 0) == 0, k
    isa = resources.kernel_isa("table_topk.o", "k_topk_combineILi3E")
    text = [t for _a, t, _b in isa]
    assert sum(t.startswith("global_load_dwordx4") for t in text) >= 3 and any(t.startswith("global_store_dwordx4") for t in text)
    assert not any("atomic" in t for t in text)
    for kernel in ("k_topk_combineILi3E", "k_topk_combineILi4E", "k_weighted_cosine_sum"):   # no contraction: the sums can be restated
        text = [t for _a, t, _b in resources.kernel_isa("table_topk.o", kernel)]
        assert any(t.startswith("v_pk_add_f32") or t.startswith("v_add_f32") for t in text), kernel
        assert not any(t.split()[0] in ("v_fma_f32", "v_pk_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32") for t in text), kernel


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def _cpu_case(name="wm"):
    c = link_case(name)
    return c, Model(c["cfg"]).eval()


def test_model_link_edges_raises_as_documented():
    c, model = _cpu_case()
    args = (c["mention"], c["table"], K_LINK, c["clip_image"], c["clip_text"])
    q, r = torch.randn(3, 8), torch.randn(c["table"].num_entities, 8)
    with pytest.raises(ValueError, match="conflicts with"):
        model.link(*args, first_stage="edges", candidates=c["candidates"])
    with pytest.raises(ValueError, match="conflicts with"):
        model.link(*args, first_stage="edges", queries=q, rows=r)
    with pytest.raises(ValueError, match="conflicts with"):
        model.link(*args, first_stage="edges", rows=r)
    with pytest.raises(ValueError, match="not None or 'edges'"):
        model.link(*args, first_stage="clip")
    with pytest.raises(ValueError, match="all three edge weights zero"):
        model.link(*args, first_stage="edges", edge_weights=(0, 0.0, 0))
    with pytest.raises(ValueError, match="expected 3"):
        model.link(*args, first_stage="edges", edge_weights=(1, 1))
    with pytest.raises(ValueError, match="goes with first_stage"):
        model.link(*args, candidates=c["candidates"], edge_weights=(1, 1, 1))
    off = Model(c["cfg"].with_(gcn_edge_enabled=(0, 0, 0, 1))).eval()   # the default weights are the configuration's
    with pytest.raises(ValueError, match="all three edge weights zero"):
        off.link(*args, first_stage="edges")
    with pytest.raises(ValueError, match="k = "):
        model.link(c["mention"], c["table"], 0, c["clip_image"], c["clip_text"], first_stage="edges")
    with pytest.raises(ValueError, match="float32 \\[3, 64\\]"):
        model.link(c["mention"], c["table"], K_LINK, c["clip_image"][:, :32], c["clip_text"], first_stage="edges")
    t = c["table"]
    from drin_amd.model import EntityTable
    bare = EntityTable(t.text, t.mask, t.image, t.object, t.object_score)
    with pytest.raises(ValueError, match="no CLIP rows"):
        model.link(c["mention"], bare, K_LINK, c["clip_image"], c["clip_text"], first_stage="edges")
    with pytest.raises(RuntimeError, match="GPU only"):                 # everything else is in order: no CPU fallback
        model.link(*args, first_stage="edges")
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(*args, first_stage="edges", edge_weights=(0, 1, 0.5))
    stored = EntityTable(t.text.bfloat16(), t.mask, t.image, t.object, t.object_score).set_clip(t.clip_text, t.clip_image)
    with pytest.raises(NotImplementedError, match="bf16-stored rows"):  # tt reads the text rows ...
        model.link(c["mention"], stored, K_LINK, c["clip_image"], c["clip_text"], first_stage="edges")
    with pytest.raises(RuntimeError, match="GPU only"):                 # ... and a dropped tt does not look at them
        model.link(c["mention"], stored, K_LINK, c["clip_image"], c["clip_text"], first_stage="edges", edge_weights=(0, 1, 1))
    with pytest.raises(RuntimeError, match="eval"):
        model.train().link(*args, first_stage="edges")
    wide = Model(DrinConfig(num_candidates_data=300, **TINY)).eval()    # N = 301: no cosine first stage lists that many
    with pytest.raises(ValueError, match="at most 256"):
        wide.link(*args, first_stage="edges")
    small = Model(c["cfg"].with_(num_candidates_data=40)).eval()        # N = 41 > the table's 30 rows
    with pytest.raises(ValueError, match="exceed the table's 30"):
        small.link(*args, first_stage="edges")
    enc = Model(DrinConfig(mention_final_layer_name="none", **TINY))
    assert isinstance(enc, EncoderModel)
    with pytest.raises(NotImplementedError, match="section 22"):
        enc.link(None, None, 1, None, None, first_stage="edges")


def test_earlier_link_calls_raise_what_they_raised():
    """the calls tests/test_drin_link_host.py::test_model_link_raises_as_documented pins, with the new keywords left out"""
    c, model = _cpu_case()
    N = c["cfg"].num_candidates_model
    args = (c["mention"], c["table"], K_LINK, c["clip_image"], c["clip_text"])
    q, r = torch.randn(3, 8), torch.randn(c["table"].num_entities, 8)
    with pytest.raises(ValueError, match="exactly one"):
        model.link(*args)
    with pytest.raises(ValueError, match="exactly one"):
        model.link(*args, first_stage=None, edge_weights=None)
    with pytest.raises(ValueError, match="exactly one"):
        model.link(*args, candidates=c["candidates"], queries=q, rows=r)
    with pytest.raises(ValueError, match="go together"):
        model.link(*args, queries=q)
    with pytest.raises(ValueError, match=f"expected \\[B, {N}\\]"):
        model.link(*args, candidates=c["candidates"][:, :-1])
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(*args, candidates=c["candidates"])
    with pytest.raises(RuntimeError, match="GPU only"):
        model.link(*args, queries=q, rows=r)


def test_invalidate_drops_the_edge_norms():
    c, model = _cpu_case()
    model.__dict__["_link_edges_inv"] = {0: "stale"}
    model.__dict__["_link_inv"] = "stale"
    assert model.invalidate() is model and "_link_edges_inv" not in model.__dict__ and "_link_inv" not in model.__dict__
    model.__dict__["_link_edges_inv"] = {0: "held"}
    assert "_link_edges_inv" not in model.__getstate__()


# ---- the margins the GPU selection test relies on ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_few_rows_lie_within_the_tolerance_of_the_kth(name):
    c = sum_case(name)
    assert c["ref"].shape == (c["B"], c["E"]) and c["ref"].dtype.name == "float64"
    counts = {p: near_threshold(c["ref"], c["k"], tol_of(c["weights"], p)) for p in ("bf16x3", "f32")}
    print(f"{name}: rows within tol of the k-th fp64 score: {counts} (cap {c['cap']})")
    assert max(counts.values()) <= c["cap"]
