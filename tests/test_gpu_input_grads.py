"""-m gpu: gradients w.r.t. the batch tensors (drin_backward_ex, drin_pool_bwd; `Model` routes batch tensors that require
grad into its autograd Function).  The reference's Model.forward is plain torch, so `loss.backward()` reaches every float
tensor of the 14-item batch; these tests hold the drop-in to that: the reference's own gradients (tests/golden/input_grads.npz),
fp64 oracle autograd at reference batch sizes, frozen-model attribution, bf16 leaves (the in-place token pooling path included),
trainable entity tables, NaN confinement, bit-stable repeats and the C ABI with no parameter gradients."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig, wikimel_config
from drin_amd.model import EntityTable, IndexedBatch, Model, _Call, _fill_params, _param_list
from oracle import drin_oracle as O
from oracle.cases import TINY, build_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOAT_INPUTS = {0: "mention_text", 4: "mention_image", 5: "mention_object", 6: "mention_object_score", 7: "entity_text",
                9: "entity_image", 10: "entity_object", 11: "entity_object_score", 12: "miet_similarity", 13: "mtei_similarity"}
FULL = ["tiny_wd", "tiny_wm", "tiny_wd_edges_1010", "tiny_wd_static", "tiny_wd_layers3", "tiny_wd_vector", "tiny_wm_silu_relu"]
BAR = 2e-4        # relative Frobenius error per tensor (the bar of the parameter gradients)
ABS_ZERO = 1e-6   # entity_object_score with one entity object and no zero object-score row: analytically 0


def rel_err(got, ref) -> float:
    got = np.asarray(got.detach().double().cpu() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(ref.detach().double().cpu() if torch.is_tensor(ref) else ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def check(field, got, ref, bar=BAR, ke1=False):
    assert got is not None, f"{field}: no gradient"
    assert tuple(got.shape) == tuple(ref.shape), field
    r = np.asarray(ref.detach().double().cpu() if torch.is_tensor(ref) else ref, np.float64)
    if ke1 and field == "entity_object_score" and np.abs(r).max() <= ABS_ZERO:
        assert got.detach().abs().max().item() <= ABS_ZERO, field
        return
    e = rel_err(got, ref)
    assert e <= bar, (field, e)


def leaves(batch, dtype=None):
    out = [t.to(DEV) for t in batch[:14]]
    for i in FLOAT_INPUTS:
        t = out[i].to(dtype) if dtype is not None else out[i]
        out[i] = t.detach().clone().requires_grad_(True)
    return out


def model_for(cfg, sd, precision="bf16x3"):
    m = Model(cfg, precision=precision).to(DEV)
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    return m


def weights(shape, seed):
    return torch.from_numpy(np.random.Generator(np.random.Philox(key=[seed, 3])).standard_normal(size=tuple(shape), dtype=np.float32))


def oracle_grads(cfg, sd, batch, G, dtype=torch.float64):
    """fp64 autograd of the oracle (pinned to the reference by tests/test_input_grads_oracle.py) on the batch as given."""
    inputs = [t.detach().cpu() for t in batch[:14]]
    for i in FLOAT_INPUTS:
        inputs[i] = inputs[i].to(dtype).requires_grad_(True)
    p = {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    scores = O.forward(p, inputs, dtype=dtype, **O.config_kwargs(cfg))
    (scores * G.to(dtype)).sum().backward()
    return {FLOAT_INPUTS[i]: inputs[i].grad for i in FLOAT_INPUTS}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "input_grads.npz"))


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", FULL)
def test_input_grads_match_the_reference(golden, name, precision):
    cfg, sd, batch = build_case(name)
    m = model_for(cfg, sd, precision)
    x = leaves(batch)
    scores = m(x)
    (scores * torch.from_numpy(golden[f"{name}/G"]).to(DEV)).sum().backward()
    for i, field in FLOAT_INPUTS.items():
        check(field, x[i].grad, golden[f"{name}/{field}"], ke1=x[11].shape[-1] == 1)


@pytest.mark.parametrize("name", ["wd_b4", "wm_b2"])
def test_input_grads_full_width_cases_match_the_reference(golden, name):
    cfg, sd, batch = build_case(name)
    m = model_for(cfg, sd)
    x = leaves(batch)
    (m(x) * torch.from_numpy(golden[f"{name}/G"]).to(DEV)).sum().backward()
    for i, field in FLOAT_INPUTS.items():
        l2 = float(golden[f"{name}/{field}_l2"])
        got = x[i].grad.double()
        if field == "entity_object_score" and l2 <= ABS_ZERO:
            assert got.abs().max().item() <= ABS_ZERO
            continue
        assert abs(got.norm().item() - l2) <= BAR * l2, field
        assert abs(got.sum().item() - float(golden[f"{name}/{field}_sum"])) <= BAR * l2 * np.sqrt(got.numel()), field


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("geometry", ["wikidiverse_b64", "wikidiverse_b128", "wikimel_b8"])
def test_input_grads_at_reference_sizes_match_fp64_oracle(geometry, precision):
    """WikiDiverse B = 64 (and B = 128: >= 1024 pairs, the split-bf16 dX products), WikiMEL N = 101, T = 64 at B = 8."""
    if geometry.startswith("wikidiverse"):
        cfg, B = DrinConfig(), int(geometry.split("_b")[1])
    else:
        cfg, B = wikimel_config(), 8
    sd = synth.make_state_dict(cfg, 7)
    batch = synth.make_batch(cfg, B, 21)
    m = model_for(cfg, sd, precision)
    x = leaves(batch)
    G = weights((B, cfg.num_candidates_model), 5)
    (m(x) * G.to(DEV)).sum().backward()
    ref = oracle_grads(cfg, sd, batch, G)
    for i, field in FLOAT_INPUTS.items():
        check(field, x[i].grad, ref[field], ke1=x[11].shape[-1] == 1)


def _tiny_wm():
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=6, max_entity_attr_token_len=6, **TINY)
    return cfg, synth.make_state_dict(cfg, 8), synth.make_batch(cfg, 3, 31)


def test_frozen_model_attribution_equals_unfrozen_run_and_leaves_params_without_grad():
    cfg, sd, batch = _tiny_wm()
    G = weights((3, cfg.num_candidates_model), 1).to(DEV)
    m = model_for(cfg, sd)
    x = leaves(batch)
    (m(x) * G).sum().backward()
    m2 = model_for(cfg, sd).requires_grad_(False)
    y = leaves(batch)
    s = m2(y)
    assert s.grad_fn is not None
    (s * G).sum().backward()
    for i, field in FLOAT_INPUTS.items():
        assert torch.equal(x[i].grad, y[i].grad), field
    assert all(p.grad is None for p in m2.parameters())


def test_param_grads_unchanged_by_feature_grads_and_repeat_bits():
    cfg, sd, batch = _tiny_wm()
    G = weights((3, cfg.num_candidates_model), 2).to(DEV)
    m = model_for(cfg, sd)
    (m([t.to(DEV) for t in batch[:14]]) * G).sum().backward()        # drin_backward: no batch tensor requires grad
    plain = [p.grad.clone() for p in m.parameters() if p.grad is not None]
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = leaves(batch)
        (m(x) * G).sum().backward()                                   # drin_backward_ex
        with_feats = [p.grad.clone() for p in m.parameters() if p.grad is not None]
        assert len(with_feats) == len(plain) and all(torch.equal(a, b) for a, b in zip(plain, with_feats))
        runs.append([x[i].grad.clone() for i in FLOAT_INPUTS])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("geometry", ["tiny_wm", "wikimel_b2"])
def test_bf16_leaves_get_bf16_gradients(geometry):
    """Six bf16 feature leaves: the token block is pooled in place (drin_pool_bwd writes its gradient in bf16), the other five
    are widened by _Call and torch's ToCopyBackward narrows their gradients.  Bar: the oracle's fp64 gradient on the widened
    values, rounded to bf16 (2^-9 relative per element) plus the path's own bar."""
    if geometry == "tiny_wm":
        cfg, sd, batch = _tiny_wm()
    else:
        cfg = wikimel_config()
        sd, batch = synth.make_state_dict(cfg, 7), synth.make_batch(cfg, 2, 41)
    batch = list(batch[:14])
    for i in (0, 4, 5, 7, 9, 10):
        batch[i] = batch[i].to(torch.bfloat16)
    x = [t.to(DEV) for t in batch]
    for i in FLOAT_INPUTS:
        x[i] = x[i].detach().clone().requires_grad_(True)
    G = weights((len(batch[0]), cfg.num_candidates_model), 3)
    m = model_for(cfg, sd)
    (m(x) * G.to(DEV)).sum().backward()
    ref = oracle_grads(cfg, sd, [t.float() if t.is_floating_point() else t for t in batch], G)
    for i, field in FLOAT_INPUTS.items():
        assert x[i].grad.dtype == x[i].dtype, field
        check(field, x[i].grad.float(), ref[field], bar=BAR + 2.0 ** -8, ke1=True)


def test_trainable_entity_table_accumulates_per_row_gradients():
    cfg = DrinConfig(**TINY)
    sd = synth.make_state_dict(cfg, 8)
    E, B = 9, 4
    tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1), 1, 51)
    men = synth.make_batch(cfg, B, 52)
    cand = torch.randint(0, E, (B, cfg.num_candidates_model), generator=torch.Generator().manual_seed(3))
    cand[0, :3] = 2                                                     # one entity three times in a list
    tensors = [tab[7][0], tab[9][0], tab[10][0], tab[11][0]]
    dev_t = [t.to(DEV).requires_grad_(True) for t in tensors]
    table = EntityTable(dev_t[0], None, dev_t[1], dev_t[2], dev_t[3])
    ib = IndexedBatch([t.to(DEV) for t in men[:7]], table, cand.to(DEV), men[12].to(DEV), men[13].to(DEV))
    G = weights((B, cfg.num_candidates_model), 4)
    m = model_for(cfg, sd)
    (m(ib) * G.to(DEV)).sum().backward()
    # oracle: fp64 autograd through the same gather
    ts = [t.double().requires_grad_(True) for t in tensors]
    seq = [t.double() if t.is_floating_point() else t for t in men[:7]]
    seq += [ts[0][cand], torch.zeros(B, dtype=torch.int64), ts[1][cand], ts[2][cand], ts[3][cand], men[12].double(), men[13].double()]
    p = {k: v.double() for k, v in sd.items()}
    (O.forward(p, seq, dtype=torch.float64, **O.config_kwargs(cfg)) * G.double()).sum().backward()
    for name, got, ref in zip(("entity_text", "entity_image", "entity_object", "entity_object_score"), dev_t, ts):
        check(name, got.grad, ref.grad, ke1=True)


def test_empty_span_nan_stays_in_its_mention():
    cfg = DrinConfig(**TINY)
    sd = synth.make_state_dict(cfg, 8)
    batch = synth.make_batch(cfg, 3, 11)
    batch[3][1] = batch[2][1]                                          # end == start: NaN scores for mention 1
    m = model_for(cfg, sd)
    x = leaves(batch)
    G = weights((3, cfg.num_candidates_model), 6)
    (m(x) * G.to(DEV)).sum().backward()
    ref = oracle_grads(cfg, sd, batch, G)
    keep = [0, 2]
    for i, field in FLOAT_INPUTS.items():
        got = x[i].grad[keep]
        assert torch.isfinite(got).all(), field
        check(field, got, ref[field][keep], ke1=True)


def test_c_abi_backward_ex_without_parameter_gradients():
    """drin_backward_ex(grads = NULL) straight through the C ABI equals the frozen Model's input gradients."""
    cfg, sd, batch = _tiny_wm()
    m = model_for(cfg, sd).requires_grad_(False)
    x = leaves(batch)
    G = weights((3, cfg.num_candidates_model), 7).to(DEV)
    (m(x) * G).sum().backward()
    lib = _lib.load()
    xs = [t.detach() for t in x]
    call = _Call(m.cfg, xs, _lib.PREC_BF16X3)
    params = tuple(p.detach().contiguous() for p in _param_list(m))
    pc = _lib.DrinParamsC()
    _fill_params(pc, params, call.per_layer)
    ws = call.workspace(True)
    scores = torch.empty(call.B, call.N, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.drin_forward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), scores.data_ptr(),
                                1, None, stream))
    outs = {f: torch.empty_like(xs[i]) for i, f in FLOAT_INPUTS.items()}
    ig = _lib.DrinInputGradsC()
    for f, t in outs.items():
        setattr(ig, f, t.data_ptr())
    n = lib.drin_input_grad_scratch_bytes(C.byref(call.cfg))
    assert n > 0
    scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
    ig.scratch, ig.scratch_bytes = scratch.data_ptr(), n
    g = G.contiguous()
    _lib.check(lib.drin_backward_ex(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), g.data_ptr(),
                                    None, C.byref(ig), None, stream))
    torch.cuda.synchronize()
    for i, f in FLOAT_INPUTS.items():
        assert torch.equal(outs[f], x[i].grad), f
    # the scratch is required, its size checked
    ig.scratch_bytes = n - 1
    assert lib.drin_backward_ex(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), g.data_ptr(),
                                None, C.byref(ig), None, stream) == _lib.E_WORKSPACE
