"""-m gpu: seeded differential sweep.  The hand-picked cases of the other files pin the reference's goldens and the timed
instantiations; this one draws CONFIGURATIONS at random (fixed seeds: the same 48 cases every run) over everything
`common/args.py:24-36,57,72,83-101` lets a caller change - dataset layout, candidate / object / token counts down to 1,
layer count, static / dynamic and scalar / vector edges, the edge switch, activations by name - and batch shapes (B = 1,
spans of one token, token counts at the Python-slice corners of `ghmfc.py:245-249`), and checks every path the product
offers for that configuration against the CPU oracle on the same inputs: inference (the folded path where it applies, else
layer by layer), the training-mode forward, the table form and the per-entity cache in both row formats, and the parameter
gradients of the triplet loss against autograd through the oracle, including WHICH gradients are None.  The check itself is
`tests/helpers.py::every_path_against_the_oracle`, shared with the hand-picked widths of tests/test_gpu_width_bands.py."""
import os

import numpy as np
import pytest
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig
from drin_amd.model import Model
from oracle import drin_oracle as O
from tests.helpers import _relu_spy, every_path_against_the_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = 48
FULL_WIDTH_CASES = 16     # the same draw at D = 768 / R = 2048: the exact-width instantiations of every row / stream / GEMM kernel
EXTRA_CASES = int(os.environ.get("DRIN_FUZZ_EXTRA", "0"))   # one-off deeper sweeps: further seeds at the small widths (every 8th at full width)


def _draw(i: int):
    g = np.random.Generator(np.random.Philox(key=[2026, i]))
    pick = lambda xs: xs[int(g.integers(0, len(xs)))]   # noqa: E731
    wikimel = bool(g.integers(0, 2))
    D = pick([64, 64, 96, 128])
    vector = g.random() < 0.2
    if vector and D % 8:
        D = 64
    R = pick([64, 128, 192])
    if CASES <= i < CASES + FULL_WIDTH_CASES or (i >= CASES + FULL_WIDTH_CASES and i % 8 == 0):
        D, R = 768, 2048
    kw = dict(
        dataset_name="wikimel" if wikimel else "wikidiverse",
        num_candidates_data=int(pick([0, 1, 2, 5, 10, 15, 16, 17, 33, 47])),
        bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
        resnet_num_region=int(pick([1, 3, 7])), max_mention_sentence_len=int(pick([6, 9, 24])),
        max_entity_attr_token_len=int(pick([1, 2, 3, 5, 9])),
        object_topk_mention=int(pick([1, 2, 3, 4])), object_topk_entity=int(pick([1, 1, 2, 3])),
        num_gcn_layers=int(pick([1, 2, 2, 2, 3])),
        gcn_edge_type=pick(["dynamic", "dynamic", "static"]),
        gcn_edge_feature="vector" if vector else "scaler",
        gcn_edge_enabled=tuple(float(x) for x in (g.random(4) < 0.8)),
        gcn_vertex_activation=pick(["gelu", "gelu", "gelu", "relu", "tanh", "silu", "sigmoid"]),
        gcn_edge_activation=pick(["sigmoid", "sigmoid", "sigmoid", "tanh", "relu", "gelu", "silu"]),
    )
    if wikimel and kw["max_entity_attr_token_len"] < 3:
        # the token mean of ghmfc.py:245-249 runs over tokens 1..ntok-2: with T <= 2 EVERY entity's slice is empty and every
        # score NaN - such a draw compares nothing (11 of 64 cases did).  The all-NaN geometry has its own test below
        kw["max_entity_attr_token_len"] += 3
    cfg = DrinConfig(**kw)
    cfg.validate()
    B = int(pick([1, 2, 3, 5, 8]))
    precision = pick(["f32", "bf16x3_all"])
    return cfg, B, precision, int(g.integers(0, 1 << 30))


def _oracle_kwargs(cfg):
    return O.config_kwargs(cfg)


@pytest.mark.parametrize("i", range(CASES + FULL_WIDTH_CASES + EXTRA_CASES))
def test_random_configuration_every_path_against_the_oracle(i):
    cfg, B, precision, seed = _draw(i)
    every_path_against_the_oracle(cfg, B, precision, seed, i, weights_seed=3 + i, index_seed=i)


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("precision", ["f32", "bf16x3_all"])
def test_token_blocks_too_short_for_a_kept_token_give_nan_everywhere_like_the_reference(T, precision):
    """WikiMEL layout with T <= 2: tokens 1..ntok-2 is an empty slice for every entity, `mean` of it is NaN (ghmfc.py:245-249)
    and the NaN reaches every score through the mention aggregates.  The one geometry the sweep above must not draw (it would
    compare nothing), checked here for what it does promise: the same all-NaN pattern on every path, nothing raised."""
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=5, bert_embed_dim=64, gcn_embed_dim=64, resnet_embed_dim=128,
                     resnet_num_region=3, max_mention_sentence_len=9, max_entity_attr_token_len=T)
    cfg.validate()
    sd = synth.make_state_dict(cfg, 5)
    batch = synth.make_batch(cfg, 3, 11, min_span=1, max_span=3, min_tokens=T)
    ref = O.forward(sd, batch[:14], **_oracle_kwargs(cfg))
    assert torch.isnan(ref).all()
    model = Model(cfg, precision=precision).to(DEV)
    model.load_state_dict(sd)
    dbatch = [t.to(DEV) for t in batch]
    model.eval()
    with torch.no_grad():
        assert torch.isnan(model(dbatch[:14])).all()
    model.train()
    assert torch.isnan(model(dbatch[:14])).all()


FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
INPUT_BAR = 2e-4      # relative Frobenius error per tensor (tests/test_gpu_input_grads.py)
INPUT_ABS_ZERO = 1e-6  # entity_object_score with one entity object: analytically 0 (unless a mention's object scores are all 0)


@pytest.mark.parametrize("i", range(CASES + FULL_WIDTH_CASES + EXTRA_CASES))
def test_random_configuration_input_gradients_against_the_oracle(i):
    """The same draws as the sweep above, backward into the batch tensors (drin_backward_ex): a seeded random non-empty subset
    of the ten float tensors are leaves (all ten in every fourth case), frozen and trainable models alternate.  Each requested
    gradient against fp64 oracle autograd (relu kinks: the bounded flip excuse of the parameter sweep), unrequested leaves keep
    .grad None, structural zeros are exact, and in the all-ten cases a run with the first leaf alone gives the same bits."""
    cfg, B, precision, seed = _draw(i)
    sd = synth.make_state_dict(cfg, 3 + i)
    T = cfg.max_entity_attr_token_len
    batch = synth.make_batch(cfg, B, seed % 100000, min_span=1, max_span=3, min_tokens=min(3, T))
    if cfg.token_level_entities and T >= 3:
        batch[8][0, 0, :] = 1
        batch[8][-1, -1, :] = 0
        batch[8][-1, -1, :3] = 1
    batch = batch[:14]
    g = np.random.Generator(np.random.Philox(key=[2027, i]))
    fields = list(FLOAT_INPUTS)
    if i % 4 == 0:
        want = fields
    else:
        want = [f for f in fields if g.random() < 0.4] or [fields[int(g.integers(0, len(fields)))]]
    frozen = i % 2 == 1
    G = torch.from_numpy(g.standard_normal(size=(B, cfg.num_candidates_model)).astype(np.float32))

    def run(leaves_):
        model = Model(cfg, precision=precision).to(DEV)
        model.load_state_dict(sd)
        if frozen:
            model.requires_grad_(False)
        x = [t.to(DEV) for t in batch]
        for j in leaves_:
            x[j] = x[j].detach().clone().requires_grad_(True)
        (model(x) * G.to(DEV)).sum().backward()
        for j in set(fields) - set(leaves_):
            assert x[j].grad is None, f"case {i}: {FLOAT_INPUTS[j]} was not requested but got a gradient"
        if frozen:
            assert all(p.grad is None for p in model.parameters())
        return {j: x[j].grad.detach().cpu() for j in leaves_}

    got = run(want)
    if i % 4 == 0:
        alone = run([want[0]])
        assert torch.equal(alone[want[0]], got[want[0]]), f"case {i}: {FLOAT_INPUTS[want[0]]} alone differs from the all-ten run"

    thr = 2e-5 if precision == "bf16x3_all" else 1e-6

    def grads(dtype, flip=()):
        p = {k: v.to(dtype) for k, v in sd.items()}
        xs = [t.to(dtype).requires_grad_(True) if j in FLOAT_INPUTS else t for j, t in enumerate(batch)]
        with _relu_spy(thr, flip) as spy:
            out = O.forward(p, xs, dtype=dtype, **_oracle_kwargs(cfg))
        assert bool(torch.isfinite(out).all()), f"case {i}: oracle scores not all finite"
        (out * G.to(dtype)).sum().backward()
        return {j: xs[j].grad for j in want}, spy.near

    ref, near = grads(torch.float64)
    # what is zero by the slice rules is exactly zero: mention-text rows outside seq[b, start:end], token rows (not token 0)
    # outside 1..ntok-2; and a tensor whose every gradient is zero (its edge switched off) is zero on every element
    L = batch[0].shape[1]
    if 0 in got:
        for b in range(B):
            rows = [t for t in range(L) if t not in range(L)[int(batch[2][b]):int(batch[3][b])]]
            assert bool((got[0][b, rows] == 0).all()), f"case {i}: mention_text rows outside the span of mention {b}"
    if 7 in got and batch[7].dim() == 4:
        ntok = batch[8].sum(-1)
        for b in range(B):
            for n in range(ntok.shape[1]):
                rows = [t for t in range(1, T) if t not in range(T)[1:int(ntok[b, n]) - 1]]
                assert bool((got[7][b, n, rows] == 0).all()), f"case {i}: entity_text token rows of pair ({b}, {n})"

    cond = {}
    nonlocal_bar = [INPUT_BAR]

    def conditioning(j):
        # the object-score gradients cancel analytically up to the 1e-9 of model.py:92 (tests/test_gpu_input_grads.py,
        # CANCELLING): a miss of the bar there is measured against the fp32 oracle's own distance, as the parameter sweep does
        if not cond:
            r32, _n = grads(torch.float32)
            cond.update({k: ((v.double() - ref[k]).norm().item() / max(ref[k].norm().item(), 1e-30)) if v is not None else 0.0
                         for k, v in r32.items()})
        return cond[j]

    def mismatches_against(yardstick):
        out_ = []
        for j, r in yardstick.items():
            gj = got[j].double()
            if r is None:              # the score does not reach this tensor (e.g. one layer: no image vertex, no ii edge)
                if not bool((gj == 0).all()):
                    out_.append(f"case {i}: {FLOAT_INPUTS[j]} does not reach the score, the library's gradient is not 0")
                continue
            r = r.double()
            if bool((r == 0).all()):
                if not bool((gj == 0).all()):
                    out_.append(f"case {i}: {FLOAT_INPUTS[j]} is structurally zero, the library's is not")
                continue
            if j == 11 and batch[11].shape[-1] == 1 and r.abs().max().item() <= INPUT_ABS_ZERO:
                if gj.abs().max().item() > INPUT_ABS_ZERO:
                    out_.append(f"case {i}: entity_object_score {gj.abs().max().item():.1e} where it is analytically 0")
                continue
            rel = (gj - r).norm().item() / r.norm().item()
            if rel > nonlocal_bar[0] and j in (6, 11) and ref[j] is not None:
                rel = rel / max(1.0, 10 * conditioning(j) / nonlocal_bar[0])
            if rel > nonlocal_bar[0]:
                out_.append(f"case {i}: {FLOAT_INPUTS[j]} off by {rel:.2e} ({cfg}, B={B}, {precision}, frozen={frozen})")
        return out_

    mismatches = mismatches_against(ref)
    if mismatches and near:
        import itertools
        units = [(c, j) for c, j, _v in near]
        if len(units) <= 4:
            subsets = [s_ for n_ in range(1, len(units) + 1) for s_ in itertools.combinations(units, n_)]
        else:
            subsets = [(u,) for u in units[:15]] + [tuple(units)]
        excused = next((s_ for s_ in subsets if not mismatches_against(grads(torch.float64, s_)[0])), None)
        if excused is None and cfg.gcn_vertex_activation == "relu" and precision == "bf16x3_all":
            # the vertex encoders' input gradients are made from the same vertex gradients as their dW, which the parameter
            # sweep above holds to 4 x 5e-4 in exactly this class (relu vertices under split-bf16 everywhere: case 6 here,
            # mention_text 1.0e-3 with the fp32 oracle itself at 4e-7); the same bound, after the flips have been tried
            nonlocal_bar[0] = 4 * 5e-4
            excused = () if not mismatches_against(ref) else None
        assert excused is not None, (f"{mismatches[0]} - and no flip of the {len(units)} relu input(s) within {thr:g} of the kink "
                                     f"explains it")
        print(f"case {i}: {len(mismatches)} input gradient(s) agree with the fp64 oracle flipped at {len(excused)} relu input(s)")
    else:
        assert not mismatches, mismatches[0]
    print(f"case {i}: leaves {[FLOAT_INPUTS[j] for j in want]} frozen={frozen} {precision}: ok")
