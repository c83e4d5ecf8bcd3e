"""-m gpu: GHMFC with `entity_final_pooling = "max"` and / or `entity_final_layer_name = "none"` against
the unmodified reference's goldens (tests/golden/ghmfc_entity.npz) in both precisions, the table form of those models (scores,
the per-entity cache, `link`, bad rows), one training step against autograd of the fp64 restatement, and the library's stated
answer where the reference raises: a 2-token entity gives a NaN score for its pair only.  Every test prints its measured maxima."""
import numpy as np
import pytest
import torch

from drin_amd.ghmfc_table import GhmfcIndexedBatch
from drin_amd.ghmfc_variants import VariantModel
from drin_amd.model import EntityTable
from drin_amd.row_ops import entity_token_pool
from tests.ghmfc_entity_inputs import CASES, TINY_CASES, entity_inputs, geometry
from tests.ghmfc_entity_restatement import entity_case_scores
from tests.ghmfc_table_inputs import rng
from tests.test_ghmfc_entity_host import entity_case_model, entity_cfg, golden
from tests.test_ghmfc_host import as_tensors, compare

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}                                      # tests/test_gpu_ghmfc_variants.py:34
GRAD_TOL = 2e-4                                                          # the same file, line 35
WIKIMEL_TINY = [n for n in TINY_CASES if "T" in CASES[n]]


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal bit for bit, NaN compared as NaN"""
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    return torch.equal(a.nan_to_num(nan=0.0).contiguous().view(torch.int32), b.nan_to_num(nan=0.0).contiguous().view(torch.int32))


def model_and_batch(name, precision, dropout=0.0):
    arrays = entity_inputs(name)
    return entity_case_model(name, precision, dropout=dropout).to(DEV), as_tensors(arrays, torch.float32, DEV), arrays


def default_entity_model(name, precision, weights):
    """the case's model with the default entity settings (Linear over the token mean), carrying `weights` where the keys agree"""
    cfg = entity_cfg(name)
    cfg.entity_final_layer_name, cfg.entity_final_pooling = "linear", "avg"
    torch.manual_seed(0)
    model = VariantModel(cfg, precision=precision, dropout=0.0).to(DEV)
    missing = model.load_state_dict(weights, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("entity_encoder") for k in missing.missing_keys)
    return model


# ---- scoring against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_goldens(name, precision):
    case = CASES[name]
    model, batch, _ = model_and_batch(name, precision)
    model.eval()
    scores, mention = model(batch), model.encode_mentions(batch)
    assert not scores.requires_grad and tuple(scores.shape) == (case["B"], geometry(name)["N"])
    want = golden(name, "scores")
    tag = f"{name} {precision}"
    compare(scores, want, TOL[precision] / max(np.nanmax(np.abs(want)), 1e-30), f"{tag} scores vs golden")
    compare(mention, golden(name, "mention_repr"), TOL[precision], f"{tag} mention_repr vs golden")
    # the mention half is the default model's own: the same bits on the same weights
    default = default_entity_model(name, precision, model.state_dict()).eval()
    assert same_bits(mention, default.encode_mentions(batch))
    if name in TINY_CASES and "T" in case and case["pooling"] == "max" and case["layer"] == "none":
        entity = entity_token_pool(batch[5], batch[6], "max")          # Identity: the entity encoder's output is the pooled rows
        assert same_bits(entity.cpu(), torch.from_numpy(golden(name, "entity_repr")))
    if not list(model.parameters()):
        return                                                          # nothing to train
    model.train()
    with torch.no_grad():                                               # train() at dropout 0: within the same bars
        compare(model(batch), want, TOL[precision] / max(np.nanmax(np.abs(want)), 1e-30), f"{tag} train() scores vs golden")


# ---- the table form ----------------------------------------------------------------------------------------------------------
def seeded_table(name, E=64):
    """(text [E, T, D], mask [E, T], candidates [B, N]) on the device: 0, 3 ... T tokens per entity, rows repeated within and
    across mentions"""
    case, g = CASES[name], geometry(name)
    T, D, B, N = case["T"], g["D"], case["B"], g["N"]
    text = rng(name, 21).standard_normal((E, T, D), dtype=np.float32)
    ntok = np.array([(0, 3, 4, 5, 6, 7, 8)[e % 7] for e in range(E)])
    mask = (np.arange(T)[None, :] < ntok[:, None]).astype(np.int64)
    cand = rng(name, 22).integers(0, E, size=(B, N)).astype(np.int64)
    cand[0, N - 1], cand[B - 1, 0], cand[0, 1] = cand[0, 0], cand[0, 0], E - 1
    return tuple(torch.from_numpy(x).to(DEV) for x in (text, mask, cand))


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", WIKIMEL_TINY)
def test_table_form_scores_cache_and_link(name, precision):
    case = CASES[name]
    model, batch, _ = model_and_batch(name, precision)
    model.eval()
    text, mask, cand = seeded_table(name)
    mention, table = batch[:5], EntityTable(text, mask, None, None, None)
    gathered = mention + [text[cand], mask[cand], 0]
    with torch.no_grad():
        want = model(gathered)
        assert same_bits(model(GhmfcIndexedBatch(mention, table, cand)), want)          # uncached: the gathered batch's bits
        model.attach_entity_table(table)
        assert same_bits(model(mention + [cand, 0, 0]), want)
        assert same_bits(model.encode_mentions(mention + [cand, 0, 0]), model.encode_mentions(gathered))
        model.check_indices()
        # the per-entity rows: once per entity instead of once per pair - the cached bar, against fp64
        model.enable_entity_cache()
        cached = model(mention + [cand, 0, 0])
        assert model.entity_cache_builds == 1
        sd64 = {k: v.double() for k, v in model.state_dict().items()}
        b64 = [x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x for x in gathered]
        ref, _m, _e = entity_case_scores(b64, sd64, case["enc"], case["repr"], case["pooling"], geometry(name)["H"])
        err = (cached.double() - ref).abs().max().item()
        print(f"{name} {precision} cached table form: max |got - fp64| = {err:.3e}")
        assert err <= TOL[precision] and not torch.isnan(cached).any()
        if case["layer"] == "none":                                     # no product anywhere: the cache changes no bit
            assert same_bits(cached, want)
        # link: the k best of the whole table, scored with the bits of the cached table form on the returned rows
        best = model.link(mention, k=5)
        assert tuple(best.rows.shape) == (case["B"], 5) and model.entity_cache_builds == 1
        first = model(mention + [best.rows[:, :4].contiguous(), 0, 0])  # N = 4 candidates per call: rows 0-3, then rows 1-4
        last = model(mention + [best.rows[:, 1:5].contiguous(), 0, 0])
        assert same_bits(first, best.scores[:, :4]) and same_bits(last, best.scores[:, 1:5])
        model.check_indices()
        bad = cand.clone()
        bad[1, 2] = text.shape[0] + 3                                   # pair 1 * 4 + 2 = 6
        model(mention + [bad, 0, 0])
        with pytest.raises(IndexError, match=rf"row {text.shape[0] + 3} at pair 6"):
            model.check_indices()


# ---- one training step -------------------------------------------------------------------------------------------------------
def grad_weights(shape, seed=77):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("name", ["wm_max_linear", "wm_max_none"])
def test_a_training_step_against_fp64_and_in_table_form(name, precision):
    case, H = CASES[name], geometry(name)["H"]
    model, batch, arrays = model_and_batch(name, precision)
    model.train()
    scores = model(batch)
    G = grad_weights(tuple(scores.shape))
    (scores * G).sum().backward()
    keys = [k for k, _ in model.named_parameters()]
    assert len(keys) == (52 if case["layer"] == "linear" else 50)
    assert any(k.startswith("entity_encoder") for k in keys) == (case["layer"] == "linear")      # "none" exposes no entity keys
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    idx = model.max_indices
    ref_scores, _m, _e = entity_case_scores(as_tensors(arrays, torch.float64, DEV), sd, case["enc"], case["repr"], case["pooling"], H,
                                            idx_text=idx["text"], idx_image=idx["image"])
    ref_grads = dict(zip(sd, torch.autograd.grad((ref_scores * G.double()).sum(), list(sd.values()), allow_unused=True)))
    err = (scores.detach().double() - ref_scores.detach()).abs().max().item()
    print(f"{name} {precision} train() scores: max |got - fp64| = {err:.3e}")
    assert err <= TOL[precision]
    top = max(g.abs().max().item() for g in ref_grads.values() if g is not None)
    worst = 0.0
    for k, p in model.named_parameters():
        ref = ref_grads[k]
        assert ref is not None and p.grad is not None and torch.isfinite(p.grad).all(), k
        own = ref.abs().max().item()
        ratio = (p.grad.double() - ref).abs().max().item() / (own if own > 0 else top)
        worst = max(worst, ratio)
        assert ratio <= GRAD_TOL, (k, ratio)
    print(f"{name} {precision} gradients: worst tensor {worst:.2e} of its max|ref| (largest max|ref| {top:.3e})")

    # the table-form step: the candidates' rows of the once-pooled table - the gathered step's bits
    text, mask, cand = seeded_table(name)
    w = grad_weights(tuple(cand.shape), seed=78)

    def step(table_form: bool):
        m = entity_case_model(name, precision, dropout=0.0).to(DEV).train()
        mention = batch[:5]
        b = GhmfcIndexedBatch(mention, EntityTable(text, mask, None, None, None), cand) if table_form else mention + [text[cand], mask[cand], 0]
        s = m(b)
        (s * w).sum().backward()
        return [s.detach()] + [p.grad for p in m.parameters()]

    want, got = step(False), step(True)
    assert len(got) == len(keys) + 1 and all(g is not None for g in got)
    assert all(same_bits(a, b) for a, b in zip(got, want)) and not any(torch.isnan(g).any() for g in got)


# ---- where the reference raises ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wm_max_linear", "wm_max_none", "wm_bare_max_none"])
def test_a_two_token_entity_gives_a_nan_score_for_its_pair_only(name):
    """The reference's max over the empty slice 1 : 1 raises IndexError; the library's stated answer is a NaN row."""
    model, batch, _ = model_and_batch(name, "bf16x3")
    model.eval()
    base = model(batch)
    assert not torch.isnan(base).any()
    masked = list(batch)
    masked[6] = batch[6].clone()
    masked[6][1, 2] = 0
    masked[6][1, 2, :2] = 1                                             # pair (1, 2) holds two tokens
    scores = model(masked)
    nan = torch.isnan(scores)
    assert nan[1, 2] and int(nan.sum()) == 1
    keep = ~nan
    assert torch.equal(scores[keep], base[keep])                        # no other pair's bits change
