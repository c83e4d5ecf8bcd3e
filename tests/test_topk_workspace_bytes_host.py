"""The bytes that the four top-k workspace queries return, as literal values recorded from the library BEFORE the two workspace
layouts became one: `drin_table_topk_workspace_bytes`, its `_ex`, `drin_table_topk_sum_workspace_bytes`, its
`_ex`.  The cases are those of `drin_host_selftest` and the host tests, and around them fp32 and bf16-stored rows, both precisions,
chunk 0 / 1 / 64 / 512, widths 16 / 32 / 768 / 776 (776: the widen route), 1 to 4 terms of mixed storage, 1 .. 65 535 mentions.  Every
offset of the old layouts is a partial sum of the same rounded regions, so equal totals over these cases pin the layout; the numbers
are not computed by the code under test.

Each row: the arguments, then the bytes of (the plain query, `_ex` with fp32 rows in f32 / bf16x3, `_ex` with the stored dtypes in
f32 / bf16x3); 0 = refused (width 4 as bf16)."""
import ctypes as C

import pytest

from drin_amd import _lib

# (batch, num_entities, width, k, chunk_entities)
SINGLE = [
    ((3, 300, 16, 20, 64), (5888, 5888, 5888, 9984, 9984)),
    ((3, 300, 16, 20, 0), (9728, 9728, 9728, 28928, 28928)),
    ((3, 300, 16, 1, 1), (5120, 5120, 5120, 5376, 5376)),
    ((3, 300, 16, 256, 512), (23552, 23552, 23552, 42752, 42752)),
    ((1, 1, 4, 1, 0), (2048, 2048, 2048, 0, 0)),
    ((4, 300, 16, 20, 1), (6656, 6656, 6656, 6912, 6912)),
    ((5, 1500, 32, 64, 0), (56832, 56832, 56832, 248832, 57856)),
    ((5, 1500, 32, 64, 64), (10752, 10752, 10752, 18944, 11776)),
    ((5, 2000, 768, 100, 512), (56320, 56320, 56320, 1629184, 80896)),
    ((5, 2000, 776, 100, 512), (56576, 56576, 56576, 1645824, 1645824)),
    ((64, 5000, 768, 100, 1024), (655360, 655360, 655360, 3801088, 851968)),
    ((64, 65536, 768, 100, 0), (18153472, 18153472, 18153472, 219480064, 18350080)),
    ((4096, 1000000, 768, 100, 0), (306184192, 306184192, 306184192, 356515840, 318767104)),
    ((4096, 1000000, 776, 100, 0), (306315264, 306315264, 306315264, 357171200, 357171200)),
    ((4096, 1000000, 768, 100, 1), (25182208, 25182208, 25182208, 25185280, 37765120)),
    ((65535, 1000000, 768, 256, 512), (738191360, 738191360, 738191360, 739764224, 939517952)),
    ((65535, 1000000, 768, 256, 0), (872409088, 872409088, 872409088, 875554816, 1073735680)),
]

# ((widths), (how each term's rows are stored), batch, num_entities, k, chunk_entities)
SUMMED = [
    (((16, 8, 8), ('f32', 'f32', 'f32'), 3, 300, 20, 0), (23040, 23040, 23040, 23040, 23040)),
    (((16, 8, 8), ('f32', 'f32', 'f32'), 3, 300, 20, 64), (11520, 11520, 11520, 11520, 11520)),
    (((16, 8, 8), ('bf16', 'bf16', 'bf16'), 3, 300, 20, 1), (9216, 9216, 9216, 9472, 9472)),
    (((16,), ('f32',), 1, 7, 7, 0), (2560, 2560, 2560, 2560, 2560)),
    (((16,), ('bf16',), 1, 7, 7, 64), (2560, 2560, 2560, 3072, 3072)),
    (((32,), ('bf16',), 4, 300, 20, 64), (8960, 8960, 8960, 17152, 9472)),
    (((768,), ('bf16',), 5, 2000, 100, 512), (59136, 59136, 59136, 1632000, 83712)),
    (((776,), ('bf16',), 5, 2000, 100, 512), (59392, 59392, 59392, 1648640, 1648640)),
    (((32, 16), ('bf16', 'f32'), 3, 300, 20, 512), (17152, 17152, 17152, 55552, 17664)),
    (((32, 16, 16), ('bf16', 'f32', 'bf16'), 3, 300, 20, 0), (23296, 23296, 23296, 61696, 43008)),
    (((32, 16, 16), ('bf16', 'f32', 'bf16'), 3, 300, 20, 64), (11776, 11776, 11776, 19968, 16384)),
    (((32, 16, 24), ('bf16', 'bf16', 'bf16'), 5, 1500, 64, 256), (39168, 39168, 39168, 71936, 64768)),
    (((768, 512, 512), ('bf16', 'bf16', 'bf16'), 4096, 1000000, 100, 0), (316719104, 316719104, 316719104, 333234176, 346079232)),
    (((768, 512, 512), ('bf16', 'f32', 'bf16'), 4096, 1000000, 100, 512), (73449472, 73449472, 73449472, 75022336, 94420992)),
    (((768, 512, 776), ('bf16', 'f32', 'bf16'), 4096, 1000000, 100, 0), (321044480, 321044480, 321044480, 337731584, 350314496)),
    (((768, 512, 512), ('f32', 'f32', 'f32'), 64, 65536, 100, 0), (52069120, 52069120, 52069120, 52069120, 52069120)),
    (((16, 260, 4, 768), ('bf16', 'f32', 'f32', 'bf16'), 9, 70000, 1, 0), (13592832, 13592832, 13592832, 228632832, 18109696)),
    (((16, 260, 4, 768), ('f32', 'f32', 'f32', 'f32'), 9, 70000, 100, 0), (13694208, 13694208, 13694208, 13694208, 13694208)),
    (((16, 264, 8, 768), ('bf16', 'bf16', 'bf16', 'bf16'), 9, 70000, 256, 0), (13897472, 13897472, 13897472, 228937472, 87854336)),
    (((16, 260, 4, 768), ('f32', 'f32', 'f32', 'f32'), 65535, 1000000, 256, 0), (1215289344, 1215289344, 1215289344, 1215289344, 1215289344)),
    (((768, 776), ('bf16', 'bf16'), 65535, 1000000, 256, 512), (1210572800, 1210572800, 1210572800, 1212162048, 1413488640)),
]


DTYPE = {"f32": _lib.FEAT_F32, "bf16": _lib.FEAT_BF16}
PRECS = (_lib.PREC_F32, _lib.PREC_BF16X3)


@pytest.mark.parametrize("args,want", SINGLE, ids=[f"one{i}" for i in range(len(SINGLE))])
def test_single_table_queries_return_the_recorded_bytes(args, want):
    lib = _lib.load()
    got = [lib.drin_table_topk_workspace_bytes(*args)]
    for dtype in (_lib.FEAT_F32, _lib.FEAT_BF16):
        got += [lib.drin_table_topk_workspace_bytes_ex(*args, dtype, prec) for prec in PRECS]
    assert tuple(got) == want


@pytest.mark.parametrize("case,want", SUMMED, ids=[f"sum{i}" for i in range(len(SUMMED))])
def test_summed_queries_return_the_recorded_bytes(case, want):
    lib = _lib.load()
    widths, stored, B, E, k, chunk = case
    S = len(widths)
    terms = (_lib.DrinTopkTermC * S)()
    for t, w in zip(terms, widths):
        t.width, t.weight = w, 1.0
    got = [lib.drin_table_topk_sum_workspace_bytes(terms, S, B, E, k, chunk)]
    for dtypes in (["f32"] * S, stored):
        arr = (C.c_int32 * S)(*[DTYPE[d] for d in dtypes])
        got += [lib.drin_table_topk_sum_workspace_bytes_ex(terms, arr, S, B, E, k, chunk, prec) for prec in PRECS]
    assert tuple(got) == want
