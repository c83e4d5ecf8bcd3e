"""-m gpu: DRIN with the transformer / none mention encoders (drin_amd/drin_encoders.py).
  * scores and layer-0 taps against the reference's goldens (tests/golden/drin_encoders.npz): 1e-4 (bf16x3) / 1e-5 (f32), the
    project's bars, on both attention cores for one case;
  * every parameter gradient and every batch-tensor gradient against the fp64 restatement (tests/drin_encoder_restatement.py,
    pinned to the goldens by tests/test_drin_encoders_host.py) evaluated at the library's own max positions and dropout masks, at
    dropout 0 and 0.1: 2e-4 of each tensor's max|ref| (DESIGN.md sections 16-20).  The loss is the reference's triplet loss: its
    gradient G w.r.t. the fp64 scores is what both sides backpropagate (a hinge that sits within rounding of its kink would
    otherwise be on in one and off in the other);
  * five Adam steps through MELRunner lower the loss, and two runs give the same bits.
Every test prints its measured maxima.  The loss of the batch that holds the empty span is NaN (the reference's too): the
gradient test of that case runs on its other rows."""
import numpy as np
import pytest
import torch

from drin_amd.attention import dropout_keep
from drin_amd.train import MELRunner, make_adam
from oracle import drin_oracle as O
from tests.drin_encoder_inputs import CASES, EMPTY_SPAN_CASE, EMPTY_SPAN_ROW, MAX, encoder_inputs, rows_without_nan
from tests.drin_encoder_restatement import encoder_forward
from tests.test_drin_encoders_host import case_model, golden
from tests.test_ghmfc_host import compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
GRAD_TOL = 2e-4
FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}


def device_batch(name, rows=None, leaves=False):
    batch = encoder_inputs(name)
    B = batch[0].shape[0]
    if rows is not None:
        batch = [t[rows] if t.shape[0] == B else t for t in batch]
    batch = [t.to(DEV) for t in batch]
    if leaves:
        for i in FLOAT_INPUTS:
            batch[i] = batch[i].detach().clone().requires_grad_(True)
    return batch


def precisions(name):
    return ("bf16x3", "f32")


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_goldens(name):
    cfg, B = CASES[name][0], CASES[name][1]
    paths = set()
    for precision, fused in (("bf16x3", True), ("bf16x3", False), ("f32", True), ("f32", False)):
        model = case_model(name, precision, fused=fused).to(DEV).eval()
        batch = device_batch(name)
        scores = model(batch[:14])
        paths.add(model.last_path)
        tag = f"{name} {precision} {model.last_path}"
        assert fused or model.last_path == "layers"
        assert not scores.requires_grad and tuple(scores.shape) == (B, cfg.num_candidates_model)
        want = golden(name, "scores")
        compare(scores, want, TOL[precision] / max(np.nanmax(np.abs(want)), 1e-30), f"{tag} scores vs golden")
        if name == EMPTY_SPAN_CASE:
            assert torch.isnan(scores[EMPTY_SPAN_ROW]).all() and int(torch.isnan(scores).any(1).sum()) == 1
        if cfg.mention_final_representation == MAX:
            idx = model.max_indices
            assert set(idx) == {"edge", "text"} and all(t.dtype == torch.int32 and tuple(t.shape) == (B, cfg.bert_embed_dim) for t in idx.values())
            assert int(idx["edge"][0, 0]) == cfg.max_mention_sentence_len - 1                 # the padded position attains the maximum
            assert int(idx["edge"][1, 2]) == 1                                               # the exact tie: the lowest position
        else:
            assert model.max_indices == {}
        taps = model.forward_traced(batch[:14])
        compare(taps["scores"], want, TOL[precision] / max(np.nanmax(np.abs(want)), 1e-30), f"{tag} traced scores vs golden")
        for key in ("mt0", "mi0", "et0", "ei0"):
            compare(taps[key], golden(name, key), TOL[precision], f"{tag} {key} vs golden")
        edges = taps["edges0"][..., 0] if cfg.gcn_edge_feature == "vector" else taps["edges0"]
        compare(edges, golden(name, "edges0"), TOL[precision], f"{tag} edges0 vs golden")
    # the folded inference path where Model._route would take it for the linear model: two dynamic scalar-edge layers
    folds = cfg.num_gcn_layers == 2 and cfg.gcn_edge_feature == "scaler"
    assert paths == ({"prepared", "layers"} if folds else {"layers"}), paths


def test_both_attention_cores_match_the_golden():
    name = "tr_max"
    want = golden(name, "scores")
    for core in ("fma", "mfma"):
        model = case_model(name, "bf16x3", core=core).to(DEV).eval()
        scores = model(device_batch(name)[:14])
        compare(scores, want, TOL["bf16x3"] / np.abs(want).max(), f"{name} core={core} scores vs golden")


def stream_keeps(model, p):
    """every mask of the most recent training forward, regenerated on the host from the stream's log, in draw order (CPU)"""
    s = model.dropout_stream
    return [dropout_keep(s.seed, call, B, H, Lq, Lk, p) for call, B, H, Lq, Lk in s.log]


def reference(model, cpu_batch, keeps, p):
    """(fp64 scores, G = d triplet loss / d scores, {parameter: gradient}, {batch position: gradient}) at model.max_indices"""
    cfg = model.cfg
    sd = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.state_dict().items()}
    batch = [t.double() if t.is_floating_point() else t for t in cpu_batch[:14]]
    for i in FLOAT_INPUTS:
        batch[i].requires_grad_(True)
    at = {k: v.long().cpu() for k, v in model.max_indices.items()}
    scores = encoder_forward(sd, batch, cfg, at_edge=at.get("edge"), at_vertex=at.get("text"), keeps=keeps, p=p)
    leaf = scores.detach().requires_grad_(True)
    O.triplet_loss(cpu_batch[14].double(), leaf, cfg.triplet_margin).backward()
    scores.backward(leaf.grad)
    return scores.detach(), leaf.grad, {k: v.grad for k, v in sd.items()}, {i: batch[i].grad for i in FLOAT_INPUTS}


def check_gradients(tag, model, batch, ref_params, ref_inputs):
    worst = 0.0
    top = max(float(g.abs().max()) for g in ref_params.values() if g is not None)
    for k, p in model.named_parameters():
        ref = ref_params[k]
        if ref is None or float(ref.abs().max()) == 0.0:
            assert p.grad is None or not p.grad.any(), k                  # the score does not depend on it
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        diff, r = (p.grad.double().cpu() - ref).abs(), ref
        if k.endswith("in_proj_bias"):                                   # the key bias: its true gradient is zero (softmax ignores a
            E = ref.numel() // 3                                         # constant added to every key) - against the model's largest gradient
            ratio = float(diff[E:2 * E].max()) / top
            assert ratio <= GRAD_TOL, (k, "key bias", ratio)
            keep = torch.ones_like(ref, dtype=torch.bool)
            keep[E:2 * E] = False
            diff, r = diff[keep], ref[keep]
        ratio = float(diff.max()) / float(r.abs().max())
        worst = max(worst, ratio)
        assert ratio <= GRAD_TOL, (k, ratio)
    for i, field in FLOAT_INPUTS.items():
        got, ref = batch[i].grad, ref_inputs[i]
        if ref is None or float(ref.abs().max()) <= 1e-6 * top:          # analytically zero (one entity object, no zero score row)
            assert got is None or float(got.abs().max()) <= 1e-6 * max(top, 1.0), field
            continue
        assert got is not None and torch.isfinite(got).all(), field
        ratio = float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())
        worst = max(worst, ratio)
        assert ratio <= GRAD_TOL, (field, ratio)
    print(f"{tag} gradients: worst tensor {worst:.2e} of its max|ref|")


# dropout 0 for every case; 0.1 wherever there is something to drop (the "none" encoder has no dropout at all)
GRAD_RUNS = [(n, 0.0) for n in CASES] + [(n, 0.1) for n in CASES if CASES[n][0].mention_final_layer_name == "transformer"]


@pytest.mark.parametrize("name,dropout", GRAD_RUNS)
def test_gradients_against_fp64_at_the_librarys_positions_and_masks(name, dropout):
    rows = rows_without_nan(name)
    cpu_batch = [t[rows] if t.shape[0] == CASES[name][1] else t for t in encoder_inputs(name)]
    for precision in precisions(name):
        model = case_model(name, precision, dropout=dropout, seed=21).to(DEV).train()
        batch = device_batch(name, rows, leaves=True)
        scores = model(batch[:14])
        keeps = stream_keeps(model, dropout) if dropout > 0 else None
        if dropout > 0:
            assert len(keeps) == 4 * model.cfg.transformer_num_layers      # four draws per layer
        ref_scores, G, ref_params, ref_inputs = reference(model, cpu_batch, keeps, dropout)
        tag = f"{name} {precision} dropout={dropout}"
        err = float((scores.detach().double().cpu() - ref_scores).abs().max())
        print(f"{tag}: scores max abs err vs fp64 = {err:.3g}")
        assert err <= TOL[precision]
        scores.backward(G.float().to(DEV))
        check_gradients(tag, model, batch, ref_params, ref_inputs)


def five_steps():
    name = "tr_max"
    cfg = CASES[name][0].with_(metrics_topk=(1,))                       # two gold columns: top-1 is the only k that fits
    model = case_model(name, "bf16x3", seed=3).to(DEV)                   # transformer_dropout 0.1 (args.py:64): the training steps draw
    runner = MELRunner(cfg, model, DEV)
    opt = make_adam(model, 1e-2)
    assert isinstance(opt, torch.optim.Adam)
    batch = encoder_inputs(name)
    before = runner.run_epoch([batch], 1, None).loss                     # eval: no dropout, the same batch
    steps = [runner.run_epoch([batch], 0, opt).loss for _ in range(5)]
    after = runner.run_epoch([batch], 1, None).loss
    runner.close()
    return [before] + steps + [after], [p.detach().clone() for p in model.parameters()]


def test_five_adam_steps_lower_the_loss_and_repeat_bit_for_bit():
    losses, params = five_steps()
    again, params2 = five_steps()
    print("tr_max five Adam steps through MELRunner, loss before | per step | after:", " ".join(f"{v:.6f}" for v in losses))
    assert losses[-1] < losses[0]                                        # the eval loss of the batch it trained on
    assert losses == again and all(torch.equal(a, b) for a, b in zip(params, params2))


def test_a_sliced_call_reports_the_whole_batchs_max_positions():
    """A batch above MAX_CALL_MENTIONS is scored in slices (mentions are independent): `max_indices` is the whole batch's.  With
    the "none" encoder both rows' positions come from the raw block alone, so they equal the one call's exactly; the scores of
    calls of different sizes agree to fp32 re-association, 5e-6 (the bound `Model.MAX_CALL_MENTIONS` documents)."""
    name = "none_max"
    model = case_model(name, "f32", fused=False).to(DEV).eval()
    batch = device_batch(name)[:14]
    whole, at = model(batch), {k: v.clone() for k, v in model.max_indices.items()}
    model.MAX_CALL_MENTIONS = 2                                           # B = 3: slices of 2 and 1
    sliced = model(batch)
    gap = float((sliced - whole).abs().max())
    print(f"sliced vs whole call, {name}: max abs gap = {gap:.3g}")
    assert gap <= 5e-6 and set(model.max_indices) == {"edge", "text"}
    assert all(torch.equal(model.max_indices[k], at[k]) and tuple(at[k].shape) == (3, 16) for k in at)
