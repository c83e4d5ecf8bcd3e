"""GHMFC's table form on the MI355X: the indexed row kernels through the C ABI against numpy / torch
indexing, `drin_ghmfc_forward_table` against `drin_ghmfc_forward` on the gathered batch bit for bit, the per-entity rows against
the fp64 restatement, and the three models - scoring, a training step, the cache and its invalidation, bad indices.

Bit equality is asserted wherever the table form runs the gathered form's operands through the gathered form's kernels; the
per-entity rows evaluate the entity Linear once per entity instead of once per pair (another product shape, possibly another
GEMM kernel), so they are held to the project's bars for GHMFC scores against fp64: 1e-4 absolute (bf16x3), 1e-5 (f32).
Set GHMFC_TABLE_PARITY_OUT to a path to have the measured maxima written there as JSON (profiles/ghmfc_table_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib
from drin_amd.ghmfc import GhmfcConfig, Model
from drin_amd.ghmfc_table import GhmfcIndexedBatch
from drin_amd.ghmfc_train import TrainableModel
from drin_amd.ghmfc_variants import VariantConfig, VariantModel
from drin_amd.model import EntityTable
from tests.ghmfc_inputs import KEYS
from tests.ghmfc_restatement import ghmfc_scores
from tests.ghmfc_table_inputs import TABLE_CASES, candidate_rows, entity_table, gathered, rng, table_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
PRECISION = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
dev = lambda a, dtype=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)   # noqa: E731


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal bit for bit, NaN compared as NaN"""
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.nan_to_num(nan=0.0).view(torch.int32), b.nan_to_num(nan=0.0).view(torch.int32))


def status_words():
    return torch.zeros(4, dtype=torch.int32, device=DEV)


# ---- kernels, through the C ABI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 9])
@pytest.mark.parametrize("count", [1, 1000])
@pytest.mark.parametrize("width", [4, 16, 772])
def test_gather_rows_is_exact(width, count, E):
    lib = _lib.load()
    r = rng(f"gather_{width}_{count}_{E}", 1)
    table = r.standard_normal((E, width), dtype=np.float32)
    index = r.integers(0, E, size=count).astype(np.int64)              # unsorted, with repeats (count > E, or E = 1)
    index[-1] = index[0]
    t, i = dev(table), dev(index)
    out = torch.full((count, width), float("nan"), device=DEV)
    words = status_words()
    _lib.check(lib.drin_gather_rows(ptr(t), ptr(i), E, ptr(out), count, width, ptr(words), stream()))
    assert np.array_equal(out.cpu().numpy(), table[index])
    assert words.tolist() == [0, 0, 0, 0]


def token_mean_table(name, E, T, D):
    """text, mask with token counts cycling through 0, 1, 2, 3, 10, 11 and T (those that fit T): the slice 1 : -1 of an empty
    mask, the empty slices, one row, the unroll of 8 with tails of 0 and 1, the whole block"""
    r = rng(name, 1)
    text = r.standard_normal((E, T, D), dtype=np.float32)
    counts = [c for c in (0, 1, 2, 3, 10, 11, T) if c <= T]
    ntok = np.array([counts[e % len(counts)] for e in range(E)])
    return text, (np.arange(T)[None, :] < ntok[:, None]).astype(np.int64)


@pytest.mark.parametrize("D", [16, 768, 1028])
@pytest.mark.parametrize("T", [1, 2, 9, 17])
def test_indexed_token_mean_has_the_bits_of_the_gathered_block(T, D):
    lib = _lib.load()
    E, pairs = 9, 23
    text, mask = token_mean_table(f"mean_{T}_{D}", E, T, D)
    index = rng(f"mean_{T}_{D}", 2).integers(0, E, size=pairs).astype(np.int64)
    index[:E] = np.arange(E)[::-1]                                      # every token count is met
    t, m, i = dev(text), dev(mask), dev(index)
    got = torch.full((pairs, D), 7.0, device=DEV)
    words = status_words()
    _lib.check(lib.drin_entity_token_mean_indexed(ptr(t), ptr(m), ptr(i), E, ptr(got), pairs, T, D, ptr(words), stream()))
    block, bmask = t[i].contiguous(), m[i].contiguous()
    want = torch.full((pairs, D), 7.0, device=DEV)
    _lib.check(lib.drin_entity_token_mean(ptr(block), ptr(bmask), ptr(want), pairs, T, D, stream()))
    assert same_bits(got, want)
    kept = np.maximum(np.where(mask.sum(1) == 0, T - 1, mask.sum(1) - 1) - 1, 0)[index]
    assert np.array_equal(np.isnan(got.cpu().numpy()).all(1), kept == 0)   # an empty slice: a NaN row, nothing else is
    assert words.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("N", [1, 4, 101])
@pytest.mark.parametrize("D", [4, 16, 768])
def test_indexed_cosine_has_the_bits_of_the_gathered_rows(D, N):
    lib = _lib.load()
    B, E = 3, 9
    r = rng(f"cos_{D}_{N}", 1)
    x = r.standard_normal((B, D), dtype=np.float32)
    rows = r.standard_normal((E, D), dtype=np.float32)
    rows[2] = 0.0                                                       # an all-zero row: the eps clamp
    index = candidate_rows(f"cos_{D}_{N}", B, N, E)
    index[B - 1, N - 1] = 2
    xt, rt, it = dev(x), dev(rows), dev(index)
    got, want = (torch.full((B, N), 7.0, device=DEV) for _ in range(2))
    words = status_words()
    _lib.check(lib.drin_cosine_rows_indexed_fwd(ptr(xt), ptr(rt), ptr(it), E, ptr(got), B, N, D, 1e-8, ptr(words), stream()))
    y = rt[it].contiguous()
    _lib.check(lib.drin_cosine_rows_fwd(ptr(xt), ptr(y), ptr(want), B, N, D, 1e-8, stream()))
    assert same_bits(got, want)
    assert got[B - 1, N - 1].item() == 0.0 and words.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("op", ["gather", "mean", "cosine"])
def test_bad_indices_are_clamped_and_reported(op):
    """-1 and E in one call: the results are those of rows 0 and E - 1, the status words name one of the two (the first
    reporter), drin_index_status turns them into DRIN_E_INDEX and zeroes them; a NULL status pointer clamps silently."""
    lib = _lib.load()
    E, T, D, B, N = 9, 6, 16, 2, 4
    text, mask = entity_table("bad_index", E, T, D)
    rows = rng("bad_index", 3).standard_normal((E, D), dtype=np.float32)
    x = rng("bad_index", 4).standard_normal((B, D), dtype=np.float32)
    index = candidate_rows("bad_index", B, N, E)
    index[0, 2], index[1, 1] = -1, E                                    # pairs 2 and 5
    clamped = np.clip(index, 0, E - 1)
    t, m, rt, xt = dev(text), dev(mask), dev(rows), dev(x)

    def run(idx, words):
        i = dev(idx)
        if op == "gather":
            out = torch.full((B * N, D), 7.0, device=DEV)
            _lib.check(lib.drin_gather_rows(ptr(rt), ptr(i), E, ptr(out), B * N, D, ptr(words), stream()))
        elif op == "mean":
            out = torch.full((B * N, D), 7.0, device=DEV)
            _lib.check(lib.drin_entity_token_mean_indexed(ptr(t), ptr(m), ptr(i), E, ptr(out), B * N, T, D, ptr(words), stream()))
        else:
            out = torch.full((B, N), 7.0, device=DEV)
            _lib.check(lib.drin_cosine_rows_indexed_fwd(ptr(xt), ptr(rt), ptr(i), E, ptr(out), B, N, D, 1e-8, ptr(words), stream()))
        return out

    want = run(clamped, None)
    words = status_words()
    assert same_bits(run(index, words), want)
    assert words.tolist() in ([1, 2, -1, -1], [1, 5, E, 0])
    st = lib.drin_index_status(words.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert st == _lib.E_INDEX and words.tolist() == [0, 0, 0, 0]
    message = lib.drin_last_error().decode()
    assert "row -1 at pair 2" in message or f"row {E} at pair 5" in message, message
    assert same_bits(run(index, None), want)                            # NULL: clamped silently
    assert lib.drin_index_status(words.data_ptr(), torch.cuda.current_stream().cuda_stream) == _lib.OK


# ---- the launch sequence -----------------------------------------------------------------------------------------------------
def reference_state_dict(name: str):
    """the weights of `torch.manual_seed(seed); ghmfc.Model(cfg)` as a device state dict, and the configuration"""
    case = TABLE_CASES[name]
    g = case["geom"]
    cfg = GhmfcConfig(dataset_name="wikimel", num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"],
                      image_regions=g["P"], num_heads=g["H"], entity_tokens=case["T"])
    torch.manual_seed(case["seed"])
    model = Model(cfg)
    return cfg, {k: v.detach().to(DEV).contiguous() for k, v in model.state_dict().items()}


def config_c(cfg: GhmfcConfig, B: int, tokens: int, precision: str):
    return _lib.DrinGhmfcConfigC(batch=B, num_candidates=cfg.num_candidates, embed_dim=cfg.embed_dim, image_dim=cfg.image_dim,
                                 mention_tokens=cfg.mention_tokens, image_regions=cfg.image_regions, num_heads=cfg.num_heads,
                                 entity_tokens=tokens, precision=PRECISION[precision], layer_norm_eps=cfg.layer_norm_eps,
                                 cosine_eps=cfg.cosine_eps)


def forward_gathered(cfg, sd, mention, ef, emask, precision):
    lib = _lib.load()
    mf, mmask, mimage = mention[0], mention[1], mention[4]
    B, tokens = mf.shape[0], (ef.shape[2] if ef.dim() == 4 else 0)
    c = config_c(cfg, B, tokens, precision)
    bt = _lib.DrinGhmfcBatchC(ptr(mf), ptr(mmask), ptr(mimage), ptr(ef), ptr(emask))
    pc = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[sd[k].data_ptr() for k in KEYS]))
    nbytes = lib.drin_ghmfc_workspace_bytes(C.byref(c))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    scores = torch.full((B, cfg.num_candidates), 7.0, device=DEV)
    men = torch.full((B, cfg.embed_dim), 7.0, device=DEV)
    _lib.check(lib.drin_ghmfc_forward(C.byref(c), C.byref(bt), C.byref(pc), ptr(ws), nbytes, ptr(scores), ptr(men), stream()))
    return scores, men


def forward_table(cfg, sd, mention, text, mask, cand, precision, rows=None, words=None):
    lib = _lib.load()
    mf, mmask, mimage = mention[0], mention[1], mention[4]
    B, tokens = mf.shape[0], (text.shape[1] if text.dim() == 3 else 0)
    c = config_c(cfg, B, 0, precision)                                  # the table's token count is the table's
    bt = _lib.DrinGhmfcBatchC(ptr(mf), ptr(mmask), ptr(mimage), None, None)
    pc = _lib.DrinGhmfcParamsC.from_buffer_copy((C.c_void_p * 52)(*[sd[k].data_ptr() for k in KEYS]))
    tc = _lib.DrinGhmfcTableC(size=C.sizeof(_lib.DrinGhmfcTableC), text=ptr(text), mask=ptr(mask), num_entities=text.shape[0],
                              entity_tokens=tokens, candidates=ptr(cand), index_status=ptr(words), rows=ptr(rows))
    nbytes = lib.drin_ghmfc_table_workspace_bytes(C.byref(c), C.byref(tc))
    assert nbytes > 0, lib.drin_last_error()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    scores = torch.full((B, cfg.num_candidates), 7.0, device=DEV)
    men = torch.full((B, cfg.embed_dim), 7.0, device=DEV)
    _lib.check(lib.drin_ghmfc_forward_table(C.byref(c), C.byref(bt), C.byref(pc), C.byref(tc), ptr(ws), nbytes, ptr(scores), ptr(men),
                                            stream()))
    return scores, men


def entity_rows(sd, text, mask, precision):
    lib = _lib.load()
    E, D = text.shape[0], text.shape[-1]
    tokens = text.shape[1] if text.dim() == 3 else 0
    nbytes = lib.drin_ghmfc_entity_rows_workspace_bytes(E, tokens, D)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
    rows = torch.full((E, D), 7.0, device=DEV)
    _lib.check(lib.drin_ghmfc_entity_rows(ptr(text), ptr(mask), E, tokens, D, ptr(sd["entity_encoder.final_layer.weight"]),
                                          ptr(sd["entity_encoder.final_layer.bias"]), PRECISION[precision], ptr(rows), ptr(ws), nbytes,
                                          stream()))
    return rows


_CASE_CACHE = {}


def device_case(name: str):
    """(cfg, state dict, mention, text, mask, candidates) on the device and the fp64 restatement's scores, computed once"""
    if name not in _CASE_CACHE:
        mention, text, mask, cand = table_case(name)
        cfg, sd = reference_state_dict(name)
        batch64 = [torch.from_numpy(x).double() if isinstance(x, np.ndarray) and x.dtype.kind == "f" else
                   (torch.from_numpy(x) if isinstance(x, np.ndarray) else x) for x in gathered(mention, text, mask, cand)]
        ref = ghmfc_scores(batch64, {k: v.double().cpu() for k, v in sd.items()}, cfg.num_heads, cfg.cosine_eps)
        _CASE_CACHE[name] = (cfg, sd, [dev(x) for x in mention], dev(text), dev(mask), dev(cand), ref)
    return _CASE_CACHE[name]


def worst_error(got: torch.Tensor, ref: torch.Tensor, what: str) -> float:
    got, ref = got.double().cpu(), ref.double()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs from the restatement"
    err = (got[~nan] - ref[~nan]).abs().max().item()
    print(f"{what}: max |got - fp64| = {err:.3e}")
    return err


_PARITY = {}


def record(key: str, value: float) -> None:
    _PARITY[key] = value
    out = os.environ.get("GHMFC_TABLE_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(dict(sorted(_PARITY.items())), f, indent=1)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["tiny_b3", "tiny_b300", "tiny_pooled_b3", "tiny_pooled_b300"])
def test_forward_table_has_the_bits_of_the_gathered_forward(name, precision):
    cfg, sd, mention, text, mask, cand, ref = device_case(name)
    ef = text[cand].contiguous()
    emask = mask[cand].contiguous() if mask is not None else None
    want_scores, want_men = forward_gathered(cfg, sd, mention, ef, emask, precision)
    words = status_words()
    scores, men = forward_table(cfg, sd, mention, text, mask, cand, precision, words=words)
    assert same_bits(scores, want_scores) and same_bits(men, want_men)
    assert words.tolist() == [0, 0, 0, 0]
    assert worst_error(scores, ref, f"{name} {precision} table form") <= TOL[precision]
    again, _ = forward_table(cfg, sd, mention, text, mask, cand, precision)
    assert same_bits(again, scores)                                     # the same bits every run


def test_forward_table_at_the_reference_widths():
    cfg, sd, mention, text, mask, cand, ref = device_case("reference_b2")
    want_scores, want_men = forward_gathered(cfg, sd, mention, text[cand].contiguous(), mask[cand].contiguous(), "bf16x3")
    scores, men = forward_table(cfg, sd, mention, text, mask, cand, "bf16x3")
    assert same_bits(scores, want_scores) and same_bits(men, want_men)
    err = worst_error(scores, ref, "reference widths bf16x3 table form")
    record("reference_b2/bf16x3/table", err)
    assert err <= TOL["bf16x3"]
    err = worst_error(forward_table(cfg, sd, mention, text, mask, cand, "bf16x3", rows=entity_rows(sd, text, mask, "bf16x3"))[0], ref,
                      "reference widths bf16x3 per-entity rows")
    record("reference_b2/bf16x3/rows", err)
    assert err <= TOL["bf16x3"]


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["tiny_b3", "tiny_b300", "tiny_pooled_b3"])
def test_forward_table_from_entity_rows_against_fp64(name, precision):
    cfg, sd, mention, text, mask, cand, ref = device_case(name)
    rows = entity_rows(sd, text, mask, precision)
    scores, men = forward_table(cfg, sd, mention, text, mask, cand, precision, rows=rows)
    _, want_men = forward_table(cfg, sd, mention, text, mask, cand, precision)
    assert same_bits(men, want_men)                                     # the mention half is the same function
    err = worst_error(scores, ref, f"{name} {precision} per-entity rows")
    record(f"{name}/{precision}/rows", err)
    assert err <= TOL[precision]


# ---- the models --------------------------------------------------------------------------------------------------------------
def make_model(kind: str, name: str, precision: str = "bf16x3", **kw):
    case = TABLE_CASES[name]
    g = case["geom"]
    geom = dict(dataset_name="wikimel", num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"],
                image_regions=g["P"], num_heads=g["H"], entity_tokens=case["T"])
    torch.manual_seed(case["seed"])
    if kind == "model":
        return Model(GhmfcConfig(**geom), precision=precision).to(DEV)
    if kind == "trainable":
        return TrainableModel(GhmfcConfig(**geom), precision=precision, **kw).to(DEV)
    return VariantModel(VariantConfig(mention_final_layer_name="none", mention_final_representation="avg extract", **geom),
                        precision=precision, **kw).to(DEV)


@pytest.mark.parametrize("kind", ["model", "trainable", "variant"])
def test_models_score_the_table_form_with_the_bits_of_the_gathered_batch(kind):
    cfg, sd, mention, text, mask, cand, ref = device_case("tiny_b3")
    model = make_model(kind, "tiny_b3").eval()
    table = EntityTable(text, mask, None, None, None)
    with torch.no_grad():
        want = model(gathered(mention, text, mask, cand))
        indexed = model(GhmfcIndexedBatch(mention, table, cand))
        model.attach_entity_table(table)
        zeros = torch.zeros(cand.shape[0], dtype=torch.int64, device=DEV)
        attached = model(mention + [cand, zeros, zeros])               # the loader's collated 0s
        repr_want, repr_got = model.encode_mentions(gathered(mention, text, mask, cand)), model.encode_mentions(mention + [cand, 0, 0])
    assert same_bits(indexed, want) and same_bits(attached, want) and same_bits(repr_got, repr_want)
    model.check_indices()
    if kind != "variant":
        assert worst_error(want, ref, f"{kind} gathered") <= TOL["bf16x3"]


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_a_training_step_has_the_bits_of_the_gathered_step(dropout):
    name = "tiny_clean_b3"
    cfg, sd, mention, text, mask, cand, ref = device_case(name)
    w = dev(rng(name, 30).standard_normal(tuple(cand.shape), dtype=np.float32))

    def step(table_form: bool):
        model = make_model("trainable", name, dropout=dropout, seed=5).train()
        batch = GhmfcIndexedBatch(mention, EntityTable(text, mask, None, None, None), cand) if table_form else gathered(mention, text, mask, cand)
        scores = model(batch)
        (scores * w).sum().backward()
        grads = [p.grad for p in model.param_list()]
        assert len(grads) == 52 and all(g is not None for g in grads)
        return [scores.detach()] + grads

    want, got, again = step(False), step(True), step(True)
    assert all(same_bits(a, b) for a, b in zip(got, want))
    assert all(same_bits(a, b) for a, b in zip(again, got))
    assert not any(torch.isnan(g).any() for g in got)


def test_a_variant_training_step_has_the_bits_of_the_gathered_step():
    name = "tiny_clean_b3"
    cfg, sd, mention, text, mask, cand, ref = device_case(name)

    def step(table_form: bool):
        model = make_model("variant", name, dropout=0.0).train()
        batch = GhmfcIndexedBatch(mention, EntityTable(text, mask, None, None, None), cand) if table_form else gathered(mention, text, mask, cand)
        scores = model(batch)
        scores.sum().backward()
        fl = model.entity_encoder.final_layer
        return scores.detach(), fl.weight.grad, fl.bias.grad

    assert all(same_bits(a, b) for a, b in zip(step(True), step(False)))


@pytest.mark.parametrize("kind", ["trainable", "variant"])
def test_entity_cache_follows_the_weights(kind):
    name = "tiny_clean_b3"
    cfg, sd, mention, text, mask, cand, _ = device_case(name)
    model = make_model(kind, name).eval()
    model.attach_entity_table(EntityTable(text, mask, None, None, None)).enable_entity_cache()
    batch = mention + [cand, 0, 0]
    heads = cfg.num_heads

    def restated():
        sd64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
        b64 = [x.double().cpu() if isinstance(x, torch.Tensor) and x.is_floating_point() else (x.cpu() if isinstance(x, torch.Tensor) else x)
               for x in gathered(mention, text, mask, cand)]
        if kind == "trainable":
            return ghmfc_scores(b64, sd64, heads, cfg.cosine_eps)
        from tests.ghmfc_restatement import entity_repr                  # the variant's mention: the span mean of the raw text
        m = torch.stack([b64[0][b, int(b64[2][b]):int(b64[3][b])].mean(0) for b in range(b64[0].shape[0])])
        e = entity_repr(b64, sd64)
        return (m[:, None, :] * e).sum(-1) / (m.norm(dim=-1).clamp_min(cfg.cosine_eps)[:, None] * e.norm(dim=-1).clamp_min(cfg.cosine_eps))

    def launches():
        _lib.profile_begin()
        with torch.no_grad():
            scores = model(batch)
        torch.cuda.synchronize()
        return scores, sum(n for _ms, n in _lib.profile_end().values())

    with torch.no_grad():
        first = model(batch)
    assert model.entity_cache_builds == 1
    assert worst_error(first, restated(), f"{kind} cached") <= TOL["bf16x3"]
    rows_ptr = model._tf.rows.data_ptr()
    second, n_reuse = launches()
    assert model.entity_cache_builds == 1 and model._tf.rows.data_ptr() == rows_ptr and same_bits(second, first)
    with torch.no_grad():
        model.entity_encoder.final_layer.weight.mul_(-0.5)              # an in-place edit: the version counter moves
    edited, n_build = launches()
    assert model.entity_cache_builds == 2 and n_build > n_reuse          # the build's launches are in the profile
    assert worst_error(edited, restated(), f"{kind} cached, after an in-place edit") <= TOL["bf16x3"]
    assert not same_bits(edited, first)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    state["entity_encoder.final_layer.bias"] += 0.75
    model.load_state_dict(state)
    with torch.no_grad():
        loaded = model(batch)
    assert model.entity_cache_builds == 3
    assert worst_error(loaded, restated(), f"{kind} cached, after load_state_dict") <= TOL["bf16x3"]
    assert not same_bits(loaded, edited)
    with torch.no_grad():
        assert same_bits(model(batch), loaded) and model.entity_cache_builds == 3
    model.enable_entity_cache(False)
    with torch.no_grad():
        uncached = model(batch)
    assert same_bits(uncached, model(gathered(mention, text, mask, cand)).detach()) and model.entity_cache_builds == 3


@pytest.mark.parametrize("kind", ["model", "trainable", "variant"])
def test_models_raise_on_a_bad_row(kind):
    name = "tiny_clean_b3"
    cfg, sd, mention, text, mask, cand, _ = device_case(name)
    E = text.shape[0]
    bad = cand.clone()
    bad[1, 2] = E + 3                                                   # pair 1 * 4 + 2 = 6
    model = make_model(kind, name).eval()
    model.attach_entity_table(EntityTable(text, mask, None, None, None))
    with torch.no_grad():
        model(mention + [bad, 0, 0])
        with pytest.raises(IndexError, match=rf"row {E + 3} at pair 6"):
            model.check_indices()
        model.check_indices()                                           # reported once
        model(mention + [cand, 0, 0])
        model.check_indices()
        model.validate_indices = True
        with pytest.raises(IndexError, match=rf"row {E + 3} at pair 6"):
            model(mention + [bad, 0, 0])
    if kind != "model":
        model.train()
        with pytest.raises(IndexError, match=rf"row {E + 3} at pair 6"):
            model(mention + [bad, 0, 0])


def test_refusals():
    cfg, sd, mention, text, mask, cand, _ = device_case("tiny_clean_b3")
    model = make_model("trainable", "tiny_clean_b3").eval()
    with pytest.raises(ValueError, match="no entity table is attached"):
        model(mention + [cand, 0, 0])
    with pytest.raises(NotImplementedError, match="bfloat16"):
        model.attach_entity_table(EntityTable(text.to(torch.bfloat16), mask, None, None, None))
    with pytest.raises(RuntimeError, match="GPU only"):
        model(GhmfcIndexedBatch(mention, EntityTable(text.cpu(), mask.cpu(), None, None, None), cand))
    with pytest.raises(RuntimeError, match="GPU only"):
        model(GhmfcIndexedBatch(mention, EntityTable(text, mask, None, None, None), cand.cpu()))
    model.attach_entity_table(EntityTable(text.cpu(), mask.cpu(), None, None, None))   # follows the model to its device
    with torch.no_grad():
        assert same_bits(model(mention + [cand, 0, 0]), model(gathered(mention, text, mask, cand)))
    assert model.entity_table.text.device.type == "cuda"
