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
    (m([t.to(DEV) for t in batch[:14]]) * G).sum().backward()        # drin_backward_ex, no input_grads: no batch tensor requires grad
    plain = [p.grad.clone() for p in m.parameters() if p.grad is not None]
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = leaves(batch)
        (m(x) * G).sum().backward()                                   # drin_backward_ex with input_grads
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


# ---- thresholds, corners and tails of drin_backward_ex -----------------------------------------------------------------------
# The cases below go where the input-gradient kernels branch: the split-bf16 pair_dx products at M = B N >= 1024 pairs (and row
# counts that are no multiple of a tile), the bf16 token block above that threshold, the inner feature dims (k_axis_mean_bwd on
# all three call sites), the LDS limit of the object pairs (Km Ke <= 64), Python-slice corners of the span and token means,
# frozen vs trainable models, calls split by MAX_CALL_MENTIONS and the C ABI's refusals.  Besides the per-tensor bar, what is
# structurally zero must be exactly zero.

def structural_zero_rows(batch):
    """Rows whose gradient is exactly zero by the slice rules (Python slices, not the oracle's masks): mention-text rows outside
    seq[b, start:end], and entity token rows other than token 0 outside feat[b, n, 1:ntok-1]."""
    B, L = batch[0].shape[:2]
    mt = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        mt[b, list(range(L)[int(batch[2][b]):int(batch[3][b])])] = False
    et = None
    if batch[7].dim() == 4:
        T = batch[7].shape[2]
        ntok = batch[8].sum(-1)
        et = torch.ones(tuple(ntok.shape) + (T,), dtype=torch.bool)
        et[..., 0] = False                                              # token 0: the text-text edge's row
        for v in ntok.unique().tolist():
            et[(ntok == v)[..., None] & torch.isin(torch.arange(T), torch.tensor(list(range(T)[1:v - 1]), dtype=torch.long))] = False
    return mt, et


# The object-score gradients are differences of terms that cancel analytically up to the 1e-9 of model.py:92 (with one object
# on a side, d score = g S eps / (W + eps)^2 against terms of size g S / (W + eps)): where that residue is what remains, fp32
# resolves it no better than the reference's own fp32 autograd does.  For these two tensors only, a miss of BAR is measured
# against the fp32 oracle's distance from the fp64 one - the conditioning rule of the parameter sweep (test_gpu_fuzz.py).
CANCELLING = ("mention_object_score", "entity_object_score")
COND_FACTOR = 10


def check_grads(got, ref, batch, bar=BAR, ke1=None, rows=None, ref32=None):
    """Every tensor of `got` against `ref` (fp64 oracle); exact zeros where the slice rules or a switched-off edge make the
    gradient zero.  `rows`: compare only these mentions.  `ref32`: a callable giving the fp32 oracle's gradients (CANCELLING)."""
    if ke1 is None:
        ke1 = batch[11].shape[-1] == 1
    mt0, et0 = structural_zero_rows(batch)
    for field, g in got.items():
        r = ref[field]
        if rows is not None:
            g, r = g[rows], r[rows]
        assert g is not None, field
        if field == "mention_text":
            z = mt0 if rows is None else mt0[rows]
            assert bool((g.detach().cpu()[z] == 0).all()), "mention_text: a row outside the clipped span is not exactly 0"
        if field == "entity_text" and et0 is not None:
            z = et0 if rows is None else et0[rows]
            assert bool((g.detach().cpu()[z] == 0).all()), "entity_text: a token row outside 1..ntok-2 is not exactly 0"
        if bool((r == 0).all()):
            assert bool((g == 0).all()), f"{field}: the gradient is structurally zero, the library's is not"
            continue
        if field in CANCELLING and ref32 is not None and rel_err(g, r) > bar:
            r32 = ref32()[field]
            cond = rel_err(r32 if rows is None else r32[rows], r)
            check(field, g.float(), r, bar=max(bar, COND_FACTOR * cond), ke1=ke1)
            continue
        check(field, g.float(), r, bar=bar, ke1=ke1)


def lazy_oracle32(cfg, sd, batch, G):
    cache = []

    def get():
        if not cache:
            cache.append(oracle_grads(cfg, sd, batch, G, dtype=torch.float32))
        return cache[0]
    return get


def run_input_grads(cfg, sd, batch, G, precision="bf16x3", want=None, frozen=False, dtype=None):
    """Model -> sum(scores * G) -> backward with the fields `want` (FLOAT_INPUTS keys, default all ten) as leaves."""
    m = model_for(cfg, sd, precision)
    if frozen:
        m.requires_grad_(False)
    want = list(FLOAT_INPUTS) if want is None else list(want)
    x = [t.to(DEV) for t in batch[:14]]
    for i in want:
        t = x[i].to(dtype) if dtype is not None and i in (0, 4, 5, 7, 9, 10) else x[i]
        x[i] = t.detach().clone().requires_grad_(True)
    scores = m(x)
    (scores * G.to(DEV)).sum().backward()
    for i in set(FLOAT_INPUTS) - set(want):
        assert x[i].grad is None
    return scores.detach(), {FLOAT_INPUTS[i]: x[i].grad for i in want}


def _wm(B, T, **kw):
    return wikimel_config(max_entity_attr_token_len=T, **kw), B


PAIR_DX = {"wikimel_b10_t8": lambda: _wm(10, 8),         # M = 1 010: exact fp32 below the threshold
           "wikimel_b11_t8": lambda: _wm(11, 8),         # M = 1 111: split-bf16, a ragged last tile
           "wikimel_b16_t64": lambda: _wm(16, 64),       # M = 1 616 at the reference's token count
           "wikidiverse_b93": lambda: (DrinConfig(), 93),   # M = 1 023
           "wikidiverse_b94": lambda: (DrinConfig(), 94)}   # M = 1 034


@pytest.mark.parametrize("geometry", list(PAIR_DX))
def test_pair_dx_threshold_and_tails_match_fp64_oracle(geometry):
    """Both precisions around the M = 1024 switch of pair_dx, at pair counts that are no multiple of a tile; the entity-text dX
    lands in g_pool and in k_token_block_bwd for WikiMEL."""
    cfg, B = PAIR_DX[geometry]()
    sd = synth.make_state_dict(cfg, 7)
    batch = synth.make_batch(cfg, B, 23)
    G = weights((B, cfg.num_candidates_model), 8)
    ref, ref32 = oracle_grads(cfg, sd, batch, G), lazy_oracle32(cfg, sd, batch, G)
    for precision in ("f32", "bf16x3"):
        _s, got = run_input_grads(cfg, sd, batch, G, precision)
        check_grads(got, ref, batch, ref32=ref32)


def test_timed_training_shape_matches_fp64_oracle_in_mention_slices_and_repeats_bits():
    """WikiMEL B = 64, T = 64 (tools/input_grad_bench.py's shape), all ten leaves, one call per precision; the oracle runs on
    four 16-mention slices (mentions are independent in Model.forward) to stay near 1 GB of host memory per slice."""
    cfg, B = _wm(64, 64)
    sd = synth.make_state_dict(cfg, 7)
    batch = synth.make_batch(cfg, B, 29)
    G = weights((B, cfg.num_candidates_model), 9)
    runs = {}
    for precision in ("bf16x3", "f32"):
        _s, a = run_input_grads(cfg, sd, batch, G, precision)
        _s, b = run_input_grads(cfg, sd, batch, G, precision)
        for f in a:
            assert torch.equal(a[f], b[f]), (precision, f)
        runs[precision] = {f: t.cpu() for f, t in a.items()}
        del a, b
    for b0 in range(0, B, 16):
        part = [t[b0:b0 + 16] if torch.is_tensor(t) and t.dim() > 0 and t.shape[0] == B else t for t in batch[:14]]
        ref, ref32 = oracle_grads(cfg, sd, part, G[b0:b0 + 16]), lazy_oracle32(cfg, sd, part, G[b0:b0 + 16])
        for precision, got in runs.items():
            check_grads({f: t[b0:b0 + 16] for f, t in got.items()}, ref, part, ref32=ref32)
        del ref


def test_bf16_leaves_above_the_pair_threshold():
    """WikiMEL B = 16, T = 64 (M = 1 616) with six bf16 feature leaves: the in-place pooled token block and drin_pool_bwd's bf16
    stores above the split-bf16 threshold.  Bar of test_bf16_leaves_get_bf16_gradients."""
    cfg, B = _wm(16, 64)
    sd = synth.make_state_dict(cfg, 7)
    batch = list(synth.make_batch(cfg, B, 43)[:14])
    for i in (0, 4, 5, 7, 9, 10):
        batch[i] = batch[i].to(torch.bfloat16)
    G = weights((B, cfg.num_candidates_model), 10)
    _s, got = run_input_grads(cfg, sd, batch, G)
    for i, f in FLOAT_INPUTS.items():
        assert got[f].dtype == batch[i].dtype, f
    widened = [t.float() if t.is_floating_point() else t for t in batch]
    ref = oracle_grads(cfg, sd, widened, G)
    check_grads(got, ref, widened, bar=BAR + 2.0 ** -8, ke1=True, ref32=lazy_oracle32(cfg, sd, widened, G))


def _inner_batch(cfg, B, k, seed):
    batch = list(synth.make_batch(cfg, B, seed)[:14])
    g = torch.Generator().manual_seed(seed)
    N, R, Km, Ke = cfg.num_candidates_model, cfg.resnet_embed_dim, cfg.object_topk_mention, cfg.object_topk_entity
    batch[5] = torch.randn(B, Km, k, R, generator=g)
    batch[9] = torch.randn(B, N, k, R, generator=g)
    batch[10] = torch.randn(B, N, Ke, k, R, generator=g)
    return batch


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("width", ["tiny", "full"])
def test_inner_feature_dims_backward(width, k):
    """mention objects [B, Km, k, R], entity image [B, N, k, R], entity objects [B, N, Ke, k, R]: k_axis_mean_bwd on all three."""
    cfg = DrinConfig(object_topk_entity=2, **TINY) if width == "tiny" else DrinConfig(dataset_name="wikimel", num_candidates_data=20,
                                                                                      max_entity_attr_token_len=6)
    B = 3
    sd = synth.make_state_dict(cfg, 7)
    batch = _inner_batch(cfg, B, k, 60 + k)
    G = weights((B, cfg.num_candidates_model), 11)
    ref, ref32 = oracle_grads(cfg, sd, batch, G), lazy_oracle32(cfg, sd, batch, G)
    for precision in ("f32", "bf16x3"):
        _s, got = run_input_grads(cfg, sd, batch, G, precision)
        check_grads(got, ref, batch, ref32=ref32)


def _object_batch(cfg, B, seed):
    batch = list(synth.make_batch(cfg, B, seed)[:14])
    batch[5][0, 1].zero_()           # a zero-norm mention object row (the nxr > cos_eps branch)
    batch[10][1, 2, 0].zero_()       # a zero-norm entity object row (the nyr > cos_eps branch)
    batch[6][2].zero_()              # every object score of mention 2 zero: miei = 0 / (0 + 1e-9)
    return batch


@pytest.mark.parametrize("km,ke", [(8, 8), (64, 1)])
def test_object_pair_limit_backward(km, ke):
    """Km Ke = 64 object pairs (the k_miei_bwd_pair LDS limit) with zero-norm object rows and an all-zero object-score mention."""
    cfg = DrinConfig(object_topk_mention=km, object_topk_entity=ke, num_candidates_data=6, **TINY)
    B = 4
    sd = synth.make_state_dict(cfg, 7)
    batch = _object_batch(cfg, B, 66)
    G = weights((B, cfg.num_candidates_model), 12)
    ref, ref32 = oracle_grads(cfg, sd, batch, G), lazy_oracle32(cfg, sd, batch, G)
    for precision in ("f32", "bf16x3"):
        _s, got = run_input_grads(cfg, sd, batch, G, precision)
        for b in range(B):              # per mention: the zero-norm rows (1 / cos_eps) and the 1e-9 denominator dwarf the rest
            check_grads(got, ref, batch, rows=[b], ref32=ref32)


@pytest.mark.parametrize("km,ke", [(65, 1), (13, 5)])
def test_object_pairs_above_the_limit_are_refused_by_backward(km, ke):
    """Km Ke = 65: the forward runs, the input gradients are refused with a clear error and nothing is handed back."""
    cfg = DrinConfig(object_topk_mention=km, object_topk_entity=ke, num_candidates_data=4, **TINY)
    sd = synth.make_state_dict(cfg, 7)
    batch = synth.make_batch(cfg, 2, 67)
    m = model_for(cfg, sd)
    x = leaves(batch)
    scores = m(x)
    with pytest.raises(_lib.DrinError, match="64 object pairs"):
        (scores * weights(tuple(scores.shape), 13).to(DEV)).sum().backward()
    for i, f in FLOAT_INPUTS.items():
        assert x[i].grad is None, f
    assert all(p.grad is None for p in m.parameters())


def test_span_and_token_corners_end_to_end():
    """Python-slice corners of the span mean (negative start / end, end > L, start at 0) and of the token mean (ntok in
    {0, 1, 2, 3, T}, masks with holes) through Model: forward and input gradients.  Pairs with ntok in {1, 2} have an empty
    token slice: their mention's scores are NaN and its gradients carry the fp64 oracle's NaN / zero pattern; every other
    mention is finite and within the bar."""
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=4, max_entity_attr_token_len=6, **TINY)
    L, T, B = cfg.max_mention_sentence_len, 6, 8
    sd = synth.make_state_dict(cfg, 7)
    batch = list(synth.make_batch(cfg, B, 71)[:14])
    spans = [(-4, 12), (1, -2), (-7, -3), (0, 3), (3, 40), (-40, 2), (L - 1, L + 5), (2, 5)]
    batch[2] = torch.tensor([s for s, _e in spans], dtype=torch.int64)
    batch[3] = torch.tensor([e for _s, e in spans], dtype=torch.int64)
    mask = batch[8]
    mask[:] = 1
    mask[0, 0] = 0                                   # ntok = 0: tokens 1..T-2
    mask[0, 1] = torch.tensor([1, 1, 1, 0, 0, 0])    # ntok = 3: token 1 alone
    mask[0, 2] = torch.tensor([1, 0, 1, 0, 1, 1])    # holes: ntok = 4 -> tokens 1..2, not 1..4
    mask[1, 3] = torch.tensor([0, 0, 0, 0, 0, 1])    # ntok = 1 (a hole at the front): NaN
    mask[2, 0] = torch.tensor([1, 1, 0, 0, 0, 0])    # ntok = 2: NaN
    mask[3, 4] = torch.tensor([1, 1, 1, 1, 0, 1])    # holes: ntok = 5 -> tokens 1..3
    G = weights((B, cfg.num_candidates_model), 14)
    ref_s = O.forward({k: v.double() for k, v in sd.items()}, batch, dtype=torch.float64)
    nan_rows = [1, 2]
    assert bool(torch.isnan(ref_s[nan_rows]).all()) and bool(torch.isfinite(ref_s[[b for b in range(B) if b not in nan_rows]]).all())
    ref = oracle_grads(cfg, sd, batch, G)
    keep = [b for b in range(B) if b not in nan_rows]
    for precision in ("f32", "bf16x3"):
        scores, got = run_input_grads(cfg, sd, batch, G, precision)
        scores = scores.cpu().double()
        assert torch.equal(torch.isnan(scores), torch.isnan(ref_s)), precision
        assert (scores[keep] - ref_s[keep]).abs().max().item() <= 2e-5, precision
        for f, g in got.items():
            g, r = g.detach().cpu().double()[nan_rows], ref[f][nan_rows]
            assert torch.equal(torch.isnan(g), torch.isnan(r)), (precision, f, "NaN pattern")
            assert bool((g[r == 0] == 0).all()), (precision, f, "zero pattern")
            assert bool(torch.isfinite(got[f][keep]).all()), (precision, f)
        check_grads(got, ref, batch, rows=keep, ref32=lazy_oracle32(cfg, sd, batch, G))


@pytest.mark.parametrize("geometry", ["wikimel_b11_bf16x3", "wikimel_b16_f32", "wikimel_b12_f32", "wikidiverse_b1100_f32",
                                      "two_candidates_b800_f32"])
def test_frozen_and_trainable_models_give_the_same_input_gradient_bits(geometry):
    """The weight-gradient flush runs between the layer loop and the input gradients only when parameters want gradients:
    the input gradients must not depend on it.  M = 1 111 (split-bf16) and the exact-fp32 single-type scratch window
    geometries of test_gpu_round4.py."""
    cfg, B = {"wikimel_b11_bf16x3": lambda: _wm(11, 8), "wikimel_b16_f32": lambda: _wm(16, 4), "wikimel_b12_f32": lambda: _wm(12, 4),
              "wikidiverse_b1100_f32": lambda: (DrinConfig(), 1100),
              "two_candidates_b800_f32": lambda: (DrinConfig(num_candidates_data=1), 800)}[geometry]()
    precision = geometry.rsplit("_", 1)[1]
    sd = synth.make_state_dict(cfg, 8)
    batch = synth.make_batch(cfg, B, 31)
    G = weights((B, cfg.num_candidates_model), 15)
    _s, a = run_input_grads(cfg, sd, batch, G, precision)
    _s, b = run_input_grads(cfg, sd, batch, G, precision, frozen=True)
    for f in a:
        assert torch.equal(a[f], b[f]), f


def test_calls_split_by_max_call_mentions_give_the_one_call_input_gradients(monkeypatch):
    cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=6, max_entity_attr_token_len=6, **TINY)
    B = 10
    sd = synth.make_state_dict(cfg, 8)
    batch = synth.make_batch(cfg, B, 32)
    G = weights((B, cfg.num_candidates_model), 16)
    _s, whole = run_input_grads(cfg, sd, batch, G)
    monkeypatch.setattr(Model, "MAX_CALL_MENTIONS", 4)              # 10 mentions -> three calls
    _s, split = run_input_grads(cfg, sd, batch, G)
    ref, ref32 = oracle_grads(cfg, sd, batch, G), lazy_oracle32(cfg, sd, batch, G)
    for f in whole:
        if f in CANCELLING and rel_err(whole[f], ref[f]) > BAR:
            continue                    # a cancellation residue (see CANCELLING): both calls are held to the oracle below instead
        assert rel_err(split[f], whole[f]) <= 2e-4, f
    check_grads(whole, ref, batch, ref32=ref32)
    check_grads(split, ref, batch, ref32=ref32)


SENTINEL = -7.25


def _abi_setup(cfg, B, seed):
    """A trainable Model's forward through the C ABI (keep_for_backward), plus sentinel-filled input and parameter gradients."""
    sd = synth.make_state_dict(cfg, 8)
    m = model_for(cfg, sd)
    xs = [t.to(DEV) for t in synth.make_batch(cfg, B, seed)[:14]]
    call = _Call(m.cfg, xs, _lib.PREC_BF16X3)
    params = tuple(p.detach().contiguous() for p in _param_list(m))
    pc = _lib.DrinParamsC()
    _fill_params(pc, params, call.per_layer)
    ws = call.workspace(True)
    scores = torch.empty(call.B, call.N, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    _lib.check(lib.drin_forward(C.byref(call.cfg), C.byref(call.batch), C.byref(pc), ws.data_ptr(), ws.numel(), scores.data_ptr(),
                                1, None, stream))
    outs = {f: torch.full(tuple(xs[i].shape), SENTINEL, dtype=torch.float32, device=DEV) for i, f in FLOAT_INPUTS.items()}
    ig = _lib.DrinInputGradsC()
    for f, t in outs.items():
        setattr(ig, f, t.data_ptr())
    n = lib.drin_input_grad_scratch_bytes(C.byref(call.cfg))
    scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
    ig.scratch, ig.scratch_bytes = scratch.data_ptr(), n
    grads = [torch.full_like(p, SENTINEL) for p in params]
    gc = _lib.DrinParamGradsC()
    _fill_params(gc, grads, call.per_layer)
    g = torch.ones(call.B, call.N, dtype=torch.float32, device=DEV)
    keep = (xs, call, params, ws, scores, scratch, g)

    def backward(cfg_c=None, batch_c=None):
        return lib.drin_backward_ex(C.byref(cfg_c or call.cfg), C.byref(batch_c or call.batch), C.byref(pc), ws.data_ptr(),
                                    ws.numel(), g.data_ptr(), C.byref(gc), C.byref(ig), None, stream)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in list(outs.values()) + grads)
    return backward, ig, outs, untouched, keep


def test_c_abi_backward_ex_refusals_precede_every_launch():
    """Each refusal of drin_backward_ex returns its code before anything is written: every input and parameter gradient keeps
    its sentinel.  Table form, entity_text_cls without batch.entity_text_cls, a misaligned output, Km Ke > 64; and the bf16
    drin_pool_bwd with embed_dim % 8 != 0."""
    lib = _lib.load()
    # (a geometry the table-form backward itself supports - bf16x3, D and R multiples of 32, >= 1024 pairs, one entity object -
    #  so that the input gradients' own refusal is the one reached)
    backward, ig, outs, untouched, keep = _abi_setup(DrinConfig(), 94, 81)
    xs, call = keep[0], keep[1]
    # table form: the same rows as a table of B N entities read through an identity index
    c_tab = _lib.DrinConfigC.from_buffer_copy(call.cfg)
    c_tab.num_entities = call.B * call.N
    b_tab = _lib.DrinBatchC.from_buffer_copy(call.batch)
    index = torch.arange(call.B * call.N, dtype=torch.int64, device=DEV).view(call.B, call.N)
    b_tab.entity_index = index.data_ptr()
    assert backward(c_tab, b_tab) == _lib.E_UNSUPPORTED
    assert "table-form" in lib.drin_last_error().decode()
    assert untouched()
    # entity_text_cls without the pooled-ahead batch field
    cls = torch.full((call.B, call.N, call.D), SENTINEL, dtype=torch.float32, device=DEV)
    ig.entity_text_cls = cls.data_ptr()
    assert backward() == _lib.E_NULL
    assert untouched() and bool((cls == SENTINEL).all())
    ig.entity_text_cls = None
    # a misaligned output
    ig.mention_image = outs["mention_image"].data_ptr() + 4
    assert backward() == _lib.E_ALIGN
    assert untouched()
    ig.mention_image = outs["mention_image"].data_ptr()
    # and the untouched call itself runs (the refusals above were not a broken setup)
    _lib.check(backward())
    torch.cuda.synchronize()
    assert not untouched()
    # Km Ke = 65 object pairs
    backward, ig, outs, untouched, keep = _abi_setup(DrinConfig(object_topk_mention=13, object_topk_entity=5, num_candidates_data=3,
                                                                **TINY), 2, 82)
    assert backward() == _lib.E_UNSUPPORTED
    assert "64 object pairs" in lib.drin_last_error().decode()
    assert untouched()
    # bf16 token block with embed_dim % 8 != 0
    c = _lib.DrinConfigC()
    lib.drin_default_config(C.byref(c))
    c.batch, c.num_candidates, c.embed_dim, c.entity_tokens, c.feature_dtype = 2, 3, 68, 5, _lib.FEAT_BF16
    mask = torch.ones(2, 3, 5, dtype=torch.int64, device=DEV)
    gp = torch.ones(2, 3, 68, dtype=torch.float32, device=DEV)
    out = torch.full((2, 3, 5, 68), SENTINEL, dtype=torch.bfloat16, device=DEV)
    assert lib.drin_pool_bwd(C.byref(c), mask.data_ptr(), gp.data_ptr(), gp.data_ptr(), out.data_ptr(),
                             torch.cuda.current_stream().cuda_stream) == _lib.E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
