"""`drin_width_class` (include/drin_hip.h): the one host function per kernel family that names the width form - tiny, guarded,
exact - its launcher takes.  Host-only, no device: the bands over a grid of (D, R, cache row format, vertex activation) against a
restatement of the instantiations the sources build, one step either side of every boundary, agreement with
`drin_fused_supported` on what is built at all, NULL and invalid configurations.  tests/test_gpu_width_bands.py asks this
function which form each of its cases runs; this file pins what it answers."""
import ctypes as C

import pytest

from drin_amd import _lib
from tests.helpers import config_c, width_class

STREAM, PAIR, ROWS, PACK, CACHED, LNB = "entity_stream", "pair_rows", "cache_rows", "cache_pack", "cached_pairs", "ln_backward"
NB, TINY, GUARDED, EXACT = "not-built", "tiny", "guarded", "exact"


def _restated(D, R, family, mixed, generic):
    """The instantiations as the kernels' template lists state them (csrc/fused_kernels.hip, csrc/entity_cache.hip): <1,1> holds
    256 columns per slot, <3,8> 768 / 2048, mixed cached pairs <1,2> 256 / 512; EXACT is compiled for gelu at (768, 2048) - 768
    alone where the family reads text rows only."""
    if D > 768 or R > 2048:
        return NB
    if mixed and family in (ROWS, PACK, CACHED) and (D % 8 or R % 8):
        return NB
    if family == PACK and not mixed:
        return NB
    text_only = family in (PAIR, PACK)
    tiny_r = 512 if (family == CACHED and mixed) else 256
    if D <= 256 and (text_only or R <= tiny_r):
        return TINY
    if D == 768 and (text_only or R == 2048) and not (generic and family in (PAIR, CACHED)):
        return EXACT
    return GUARDED


WIDTHS_D = (4, 64, 252, 256, 260, 264, 512, 736, 760, 764, 768, 772, 1024)
WIDTHS_R = (4, 64, 256, 260, 264, 508, 512, 516, 520, 1024, 2016, 2040, 2044, 2048, 2052, 2056)


@pytest.mark.parametrize("fmt", ["f32", "mixed_f16"])
@pytest.mark.parametrize("act", ["gelu", "relu", "silu"])
def test_bands_over_a_grid_of_widths(fmt, act):
    seen = set()
    for D in WIDTHS_D:
        for R in WIDTHS_R:
            for family in (STREAM, PAIR, ROWS, PACK, CACHED):
                got = width_class(D, R, family, fmt, act)
                assert got == _restated(D, R, family, fmt == "mixed_f16", act != "gelu"), (D, R, family, fmt, act)
                seen.add((family, got))
            assert width_class(D, R, LNB, fmt, act) == -(-D // 256), (D, R)
    # the grid reaches every form of every family (a generic activation has no exact pair / cached-pairs form)
    for family in (STREAM, PAIR, ROWS, CACHED) + ((PACK,) if fmt == "mixed_f16" else ()):
        want = {NB, TINY, GUARDED} | ({EXACT} if act == "gelu" or family in (STREAM, ROWS, PACK) else set())
        assert {b for f, b in seen if f == family} == want, (family, fmt, act)


@pytest.mark.parametrize("D,R,family,fmt,act,want", [
    # 256 / 260: the top of tiny and the first width past it, in D and in R
    (256, 256, STREAM, "f32", "gelu", TINY), (260, 256, STREAM, "f32", "gelu", GUARDED), (256, 260, STREAM, "f32", "gelu", GUARDED),
    (256, 2048, PAIR, "f32", "gelu", TINY), (260, 64, PAIR, "f32", "gelu", GUARDED), (260, 64, PAIR, "f32", "relu", GUARDED),
    (256, 256, ROWS, "f32", "gelu", TINY), (64, 260, ROWS, "f32", "gelu", GUARDED),
    (256, 64, PACK, "mixed_f16", "gelu", TINY), (264, 64, PACK, "mixed_f16", "gelu", GUARDED),
    (256, 256, CACHED, "f32", "gelu", TINY), (64, 260, CACHED, "f32", "gelu", GUARDED), (260, 64, CACHED, "f32", "silu", GUARDED),
    (256, 2048, LNB, "f32", "gelu", 1), (260, 64, LNB, "f32", "gelu", 2), (512, 64, LNB, "f32", "gelu", 2), (516, 64, LNB, "f32", "gelu", 3),
    # 512 / 516 (520: the next multiple of 8): mixed rows keep the tiny form one image slot longer than fp32 rows
    (64, 264, CACHED, "mixed_f16", "gelu", TINY), (64, 512, CACHED, "mixed_f16", "gelu", TINY), (64, 512, CACHED, "mixed_f16", "relu", TINY),
    (64, 520, CACHED, "mixed_f16", "gelu", GUARDED), (64, 516, CACHED, "mixed_f16", "gelu", NB), (64, 516, CACHED, "f32", "gelu", GUARDED),
    (64, 512, CACHED, "f32", "gelu", GUARDED), (264, 512, CACHED, "mixed_f16", "gelu", GUARDED),
    (64, 512, ROWS, "mixed_f16", "gelu", GUARDED), (64, 512, STREAM, "mixed_f16", "gelu", GUARDED),
    # 764 / 768 and 2044 / 2048: exact needs both widths where image rows are read, D alone where they are not
    (768, 2048, STREAM, "f32", "gelu", EXACT), (764, 2048, STREAM, "f32", "gelu", GUARDED), (768, 2044, STREAM, "f32", "gelu", GUARDED),
    (768, 2048, STREAM, "f32", "relu", EXACT),
    (768, 2016, PAIR, "f32", "gelu", EXACT), (764, 2048, PAIR, "f32", "gelu", GUARDED), (768, 2048, PAIR, "f32", "silu", GUARDED),
    (768, 2048, ROWS, "f32", "gelu", EXACT), (736, 2048, ROWS, "f32", "gelu", GUARDED), (768, 2016, ROWS, "f32", "gelu", GUARDED),
    (768, 2016, PACK, "mixed_f16", "gelu", EXACT), (760, 2040, PACK, "mixed_f16", "gelu", GUARDED), (768, 2048, PACK, "f32", "gelu", NB),
    (768, 2048, CACHED, "f32", "gelu", EXACT), (768, 2048, CACHED, "mixed_f16", "gelu", EXACT), (768, 2048, CACHED, "f32", "relu", GUARDED),
    (768, 2048, CACHED, "mixed_f16", "tanh", GUARDED), (768, 2040, CACHED, "mixed_f16", "gelu", GUARDED), (764, 2044, CACHED, "mixed_f16", "gelu", NB),
    (764, 2044, CACHED, "f32", "gelu", GUARDED), (768, 2048, LNB, "f32", "gelu", 3),
    # 768 / 772 and 2048 / 2052: past the folded path; the LayerNorm backward goes on to V = 4
    (772, 128, STREAM, "f32", "gelu", NB), (772, 128, PAIR, "f32", "gelu", NB), (772, 128, ROWS, "f32", "gelu", NB),
    (772, 128, CACHED, "f32", "gelu", NB), (768, 2052, STREAM, "f32", "gelu", NB), (64, 2052, PAIR, "f32", "gelu", NB),
    (772, 128, LNB, "f32", "gelu", 4), (1024, 2056, LNB, "f32", "gelu", 4), (1024, 2056, CACHED, "f32", "gelu", NB),
])
def test_one_step_either_side_of_every_boundary(D, R, family, fmt, act, want):
    assert width_class(D, R, family, fmt, act) == want


def _config(D, R, **fields):
    c = config_c(D, R)
    for k, v in fields.items():   # raw values of the C fields: invalid ones too
        setattr(c, k, v)
    return c


def test_agrees_with_drin_fused_supported_on_what_is_built():
    """A family of the folded / cached paths has a form exactly where `drin_fused_supported` accepts the geometry - widths, layer
    count, edge feature, inner dims - and the LayerNorm backward, a kernel of the layer-by-layer path, wherever the config is valid."""
    lib = _lib.load()
    variants = [dict(), dict(num_layers=1), dict(num_layers=3), dict(vector_edges=1), dict(entity_image_inner=2),
                dict(mention_object_inner=3), dict(entity_object_inner=2)]
    n_yes = n_no = 0
    for D in WIDTHS_D:
        for R in WIDTHS_R:
            for fields in variants:
                if fields.get("vector_edges") and D % 8:
                    continue
                c = _config(D, R, **fields)
                fused = lib.drin_fused_supported(C.byref(c)) == _lib.OK
                n_yes, n_no = n_yes + fused, n_no + (not fused)
                for family in (STREAM, PAIR, ROWS, CACHED):
                    built = lib.drin_width_class(C.byref(c), _lib.WIDTH_FAMILIES[family]) != _lib.WIDTH_NOT_BUILT
                    assert built == fused, (D, R, fields, family)
                assert lib.drin_width_class(C.byref(c), _lib.WIDTH_FAMILIES[LNB]) == -(-D // 256)
    assert n_yes > 100 and n_no > 100


def test_null_and_invalid_configurations():
    lib = _lib.load()
    for family in _lib.WIDTH_FAMILIES.values():
        assert lib.drin_width_class(None, family) == _lib.E_NULL
        assert b"config is NULL" in lib.drin_last_error()
        assert lib.drin_width_class(C.byref(_config(66, 128)), family) == _lib.E_SHAPE          # not a multiple of 4
        assert lib.drin_width_class(C.byref(_config(128, 130)), family) == _lib.E_SHAPE
        assert lib.drin_width_class(C.byref(_config(1028, 128)), family) == _lib.E_UNSUPPORTED  # past validate_config's D
        assert lib.drin_width_class(C.byref(_config(0, 128)), family) == _lib.E_SHAPE
        assert lib.drin_width_class(C.byref(_config(128, 128, cache_format=2)), family) == _lib.E_UNSUPPORTED
        assert lib.drin_width_class(C.byref(_config(128, 128, vertex_activation=9)), family) == _lib.E_UNSUPPORTED
    for family in (-1, len(_lib.WIDTH_FAMILIES)):
        assert lib.drin_width_class(C.byref(_config(128, 128)), family) == _lib.E_SHAPE
        assert b"not a drin_width_family" in lib.drin_last_error()
    # a status is negative, a band is not: the two never collide
    assert all(v >= 0 for v in _lib.WIDTH_BANDS) and _lib.E_SHAPE < 0 and _lib.E_NULL < 0 and _lib.E_UNSUPPORTED < 0
