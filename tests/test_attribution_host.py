"""CPU-side checks of gradient x input attribution: the two entry points are exported, bound and declared
with the ABI and the profiler classes unchanged, they refuse bad arguments with the right status before any launch, the fp64
restatement (tests/attribution_restatement.py) equals `sum x g` on the reference-generated gradients of
tests/golden/input_grads.npz, and the two identities `Model.attribute` relies on - token 0 and the object feature rows contract
to 0 - hold on those gradients."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from oracle.cases import build_case
from tests import attribution_restatement as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
FULL = ["tiny_wd", "tiny_wm", "tiny_wd_edges_1010", "tiny_wd_static", "tiny_wd_layers3", "tiny_wd_vector", "tiny_wm_silu_relu"]
ONE = C.c_void_p(16)      # aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)      # 4-byte aligned only
F32, BF16 = _lib.FEAT_F32, _lib.FEAT_BF16


def last():
    return _lib.load().drin_last_error().decode()


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in ("drin_token_attribution", "drin_rows_dot"):
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12
    assert "attribution_kernels.hip" in __import__("drin_amd.build", fromlist=["SOURCES"]).SOURCES
    from drin_amd.model import Attribution, Model
    assert callable(Model.attribute) and Attribution._fields[:2] == ("scores", "candidate")


def test_token_attribution_validates_on_host():
    lib, who = _lib.load(), "drin_token_attribution"

    def run(tokens=ONE, dtype=F32, mask=ONE, index=None, E=0, status=None, g=ONE, out=ONE, pairs=5, T=6, width=16):
        return lib.drin_token_attribution(tokens, dtype, mask, index, E, status, g, out, pairs, T, width, None)

    for name, text in (("tokens", "tokens"), ("g", "grad_pooled"), ("out", "out")):
        assert run(**{name: None}) == _lib.E_NULL and last() == f"{who}: {text} is NULL"
        assert run(**{name: ODD}) == _lib.E_ALIGN and last() == f"{who}: {text} is not 16-byte aligned"
    assert run(mask=None) == _lib.E_NULL and last() == f"{who}: mask is NULL"
    assert run(mask=ODD) == _lib.E_ALIGN and run(index=ODD, E=4) == _lib.E_ALIGN and "8-byte" in last()
    assert run(index=ONE, E=4, status=C.c_void_p(18)) == _lib.E_ALIGN and "index_status 4-byte" in last()
    for dtype in (-1, 2, 7):
        assert run(dtype=dtype) == _lib.E_SHAPE and f"token_dtype = {dtype}" in last()
    for width in (0, -4, 6, 770):
        assert run(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
    for width in (0, 4, 12, 772):
        assert run(dtype=BF16, width=width) == _lib.E_SHAPE and "multiple of 8" in last()
    for T in (0, -1):
        assert run(T=T) == _lib.E_SHAPE and f"T = {T}" in last()
    assert run(pairs=-1) == _lib.E_SHAPE and "pairs = -1" in last()
    for E in (0, -2):
        assert run(index=ONE, E=E) == _lib.E_SHAPE and f"num_entities (with entity_index) = {E}" in last()
    # nothing to do is not an error, and is decided after every check (no device is touched: there is none here)
    assert run(pairs=0) == _lib.OK and run(pairs=0, index=ONE, E=3, status=ONE, dtype=BF16, width=776) == _lib.OK
    assert run(pairs=0, width=6) == _lib.E_SHAPE


def test_rows_dot_validates_on_host():
    lib, who = _lib.load(), "drin_rows_dot"

    def run(x=ONE, dtype=F32, g=ONE, out=ONE, rows=5, width=16):
        return lib.drin_rows_dot(x, dtype, g, out, rows, width, None)

    for name in ("x", "g"):
        assert run(**{name: None}) == _lib.E_NULL and last() == f"{who}: {name} is NULL"
        assert run(**{name: ODD}) == _lib.E_ALIGN and last() == f"{who}: {name} is not 16-byte aligned"
    assert run(out=None) == _lib.E_NULL and "out is NULL" in last()
    assert run(out=C.c_void_p(18)) == _lib.E_ALIGN and "out must be 4-byte" in last()
    assert run(dtype=3) == _lib.E_SHAPE and "x_dtype = 3" in last()
    for width in (0, 6, -8):
        assert run(width=width) == _lib.E_SHAPE and "multiple of 4" in last()
    assert run(dtype=BF16, width=2052) == _lib.E_SHAPE and "multiple of 8" in last()
    assert run(rows=-1) == _lib.E_SHAPE and run(rows=(1 << 31) + 1) == _lib.E_SHAPE and "rows = 2147483649" in last()
    assert run(rows=0) == _lib.OK and run(rows=0, out=ODD) == _lib.OK


# ---- the restatement on the reference's own gradients ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "input_grads.npz"))


def case(golden, name):
    _cfg, _sd, batch = build_case(name)
    inputs = [t.detach().cpu() if torch.is_tensor(t) else t for t in batch[:14]]
    grads = {field: torch.from_numpy(golden[f"{name}/{field}"]) for field in R.FLOAT_INPUTS.values()}
    return inputs, grads


@pytest.mark.parametrize("name", FULL)
def test_restatement_equals_x_times_gradient_of_the_reference(golden, name):
    """What is pinned: for a token block, `token_attribution` from the POOLED rows' gradient alone (recovered from the block's: a
    kept token's row x cnt) equals `(x * x.grad).sum(-1)` of the reference's gradients on every token but token 0, to 1e-12 of the
    cancellation-free scale, and the reference passes nothing outside the kept slice.  For the other fields the restatement IS
    `(x * g).sum` over the flattened row, so the comparison there checks shapes and the flattening, nothing more."""
    inputs, grads = case(golden, name)
    want = R.gradient_x_input(inputs, grads)
    for field, (i, lead) in R.ATTRIBUTED.items():
        x, g = inputs[i].double(), grads[field].double()
        A, S = want[field]
        assert tuple(A.shape) == tuple(x.shape[:A.dim()])
        # (for the row fields this only holds `gradient_x_input`'s shapes and flattening to the plain expression: the two are the
        #  same sum; the independent check is the token branch below)
        direct = (x * g).reshape(*A.shape, -1).sum(-1)
        assert (direct - A).norm() <= 1e-12 * S.norm(), field
        if field == "entity_text" and x.dim() == 4:
            kept, cnt = R.kept_tokens(inputs[8])
            # the pooled rows' gradient: any kept token's row x cnt (every kept token carries g_pool / cnt; none kept: no share at all)
            first = kept.double().argmax(-1)
            g_pool = torch.gather(g, 2, first[..., None, None].expand(-1, -1, 1, g.shape[-1])).squeeze(2) * cnt.unsqueeze(-1)
            g_pool = torch.where(kept.any(-1, keepdim=True), g_pool, torch.zeros_like(g_pool))
            P, T, D = x.shape[0] * x.shape[1], x.shape[2], x.shape[3]
            At, St = R.token_attribution(x.reshape(P, T, D), inputs[8].reshape(P, T), g_pool.reshape(P, D))
            At, St = At.view(A.shape), St.view(A.shape)
            assert (At[..., 1:] - A[..., 1:]).norm() <= 1e-12 * S.norm(), "token rows"
            assert (At[..., 0] == 0).all() and (At[~kept] == 0).all()
            # outside the kept slice and token 0 the reference passes no pooled share either
            outside = ~kept
            outside[..., 0] = False
            assert g[outside].abs().max() == 0 if outside.any() else True


@pytest.mark.parametrize("name", FULL)
def test_token_zero_and_object_rows_contract_to_zero(golden, name):
    """The two identities of the API: token 0 of a token block feeds only the text-text cosine and the object feature rows only
    the object cosines; a cosine is homogeneous of degree 0 in each row, so <x, d cos / dx> = 0 - here within 1e-5 S on the
    reference's fp32 gradients."""
    inputs, grads = case(golden, name)
    for field, i, lead in (("mention_object", 5, 2), ("entity_object", 10, 3)):
        A, S = R.rows_dot(inputs[i], grads[field], lead)          # per object: its inner rows are averaged ahead of the cosine
        # (with the image-image edge switched off the object rows receive no gradient at all: S = 0 there, and A with it)
        assert S.norm() > 0 or name == "tiny_wd_edges_1010", field
        assert (A.abs() <= 1e-5 * S).all(), (field, float((A.abs() / (S + 1e-30)).max()))
    if inputs[7].dim() == 4:
        A, S = R.rows_dot(inputs[7][:, :, 0, :], grads["entity_text"][:, :, 0, :], 2)
        assert S.norm() > 0 and (A.abs() <= 1e-5 * S + 1e-30).all(), ("token 0", float((A.abs() / (S + 1e-30)).max()))


def test_attribute_refuses_a_token_table_it_cannot_read_in_place():
    """The token kernel walks the table with fp32 or bf16 row strides: a table of another dtype, or a non-contiguous one, is
    refused before anything is pooled, gathered or launched (no device is needed to see it)."""
    from drin_amd.config import DrinConfig
    from drin_amd.model import EntityTable, IndexedBatch, Model
    from oracle.cases import TINY
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=6, max_entity_attr_token_len=6, **TINY)
    m, E, B, N = Model(cfg), 9, 2, cfg.num_candidates_model
    text = torch.randn(E, 6, 64)
    rest = (torch.ones(E, 6, dtype=torch.int64), torch.randn(E, 1, 128), torch.randn(E, 1, 1, 128), torch.rand(E, 1))
    mention = [torch.zeros(1)] * 7
    cand, sim = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N)
    for bad, word in ((text.half(), "float16"), (text.double(), "float64"), (text.transpose(1, 2).contiguous().transpose(1, 2), "not contiguous")):
        with pytest.raises(ValueError, match="contiguous float32 or bfloat16") as e:
            m.attribute(IndexedBatch(mention, EntityTable(bad, *rest), cand, sim, sim))
        assert word in str(e.value)
    for p in m.parameters():
        assert p.grad is None
