"""No GPU: the restatement of the per-entity cache rows (tests/cache_rows_restatement.py) checked against itself, against
`oracle/precision_emulation.py` and against the oracle - and the REASON tests/test_gpu_cache_rows.py scores one field at a time
under a power-of-two factor, as assertions: at unit scale the scores hardly see a defect planted in fv_i (below the bar of the
cached path's score tests), under the factor they see it at 4 x the bar or more, while the reference's own fp32-vs-fp64 spread
under the same factor stays below a quarter of the bar."""
import pytest
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig
from drin_amd.model import EntityTable, IndexedBatch
from oracle import drin_oracle as O
from oracle import precision_emulation as PE
from tests import cache_rows_restatement as CR

TINY = dict(bert_embed_dim=64, gcn_embed_dim=64, resnet_embed_dim=128, max_mention_sentence_len=12, resnet_num_region=5)   # tests/test_gpu_round4.py

# what the consumer test multiplies each fp16 field by (2^k): the smallest factors of the issue's CPU experiment that put a
# 4-column defect at >= 4 x the score bar at every width (this file asserts it at the guarded one)
EXPONENTS = {"fv_t": 4, "fv_i": 8, "ohat": 4}


def score_bar(D: int) -> float:
    """The bar of the cached path's scores against the oracle (tests/test_gpu_round4.py:379)."""
    return 2.5e-5 if D < 256 else 1e-5


def consumer_config(D: int, R: int, **kw) -> DrinConfig:
    """WikiMEL layout (token blocks, T = 5), 21 candidates (two 16-candidate workgroups of the cached path, the second ragged),
    default activations, dynamic edges, at widths D / R."""
    base = dict(dataset_name="wikimel", num_candidates_data=20, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
                resnet_num_region=3, max_mention_sentence_len=12, max_entity_attr_token_len=5)
    base.update(kw)
    cfg = DrinConfig(**base)
    cfg.validate()
    return cfg


def table_case(cfg: DrinConfig, E: int, B: int, seed: int):
    """(table tensors on the host: text, mask or None, image, object, score), the 15-sequence of B mentions, candidates [B, N]."""
    tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1), 1, seed)
    tables = (tab[7][0], tab[8][0] if cfg.token_level_entities else None, tab[9][0], tab[10][0], tab[11][0])
    men = synth.make_batch(cfg, B, seed + 1)
    cand = torch.randint(0, E, (B, cfg.num_candidates_model), generator=torch.Generator().manual_seed(seed))
    return tables, men, cand


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---- 1. the layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", CR.FORMATS)
@pytest.mark.parametrize("D,R", [(64, 128), (264, 64), (64, 520), (768, 2048)])
def test_decode_and_encode_are_inverse_bit_for_bit(D, R, fmt):
    cfg = consumer_config(D, R)
    E = 5
    g = torch.Generator().manual_seed(D + R)
    rnd = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    f = {k: rnd(E, D) for k in ("h_t", "h_i", "chat")}
    f["tail"] = rnd(E, 4)
    f["h_t"][1, 3] = float("nan")
    if fmt == "mixed_f16":
        f["units"] = {"fv_t": rnd(E, D).half(), "fv_i": rnd(E, D).half(), "ohat": rnd(E, R).half()}
    else:
        f.update(fv_t=rnd(E, D), fv_i=rnd(E, D), ohat=rnd(E, R))
    raw = CR.encode(f, cfg, fmt)
    assert raw.dtype == torch.uint8 and raw.numel() == E * CR.row_floats(D, R, fmt) * 4
    back = CR.decode(raw, cfg, fmt)
    for k in ("h_t", "h_i", "chat", "tail"):
        assert torch.equal(_bits(back[k]), _bits(f[k])), k
    assert torch.equal(_bits(back["sg"]), _bits(f["tail"][:, 0]))
    for k in CR.F16_FIELDS:
        if fmt == "mixed_f16":
            assert torch.equal(_bits(back["units"][k]), _bits(f["units"][k])), k
            assert torch.equal(back[k], f["units"][k].double() * f["tail"][:, CR.TAIL_SLOT[k], None].double()), k
        else:
            assert torch.equal(_bits(back[k]), _bits(f[k])), k
    # every byte of a row belongs to exactly one field: arbitrary bytes survive decode -> encode
    noise = torch.randint(0, 256, (raw.numel(),), dtype=torch.uint8, generator=g)
    assert torch.equal(CR.encode(CR.decode(noise, cfg, fmt), cfg, fmt), noise)
    # the interleave itself, spelled out once: halves 8 c4 .. 8 c4 + 3 of the fv block are fv_t[4 c4 ..], the next four fv_i[4 c4 ..]
    if fmt == "mixed_f16":
        halves = raw.view(torch.float16).view(E, -1)[:, 2 * 3 * D:2 * 4 * D]
        c4 = D // 4 - 1
        assert torch.equal(halves[:, 8 * c4:8 * c4 + 4], f["units"]["fv_t"][:, 4 * c4:4 * c4 + 4])
        assert torch.equal(halves[:, 8 * c4 + 4:8 * c4 + 8], f["units"]["fv_i"][:, 4 * c4:4 * c4 + 4])
        assert torch.equal(raw.view(torch.float16).view(E, -1)[:, 2 * 4 * D:2 * 4 * D + R], f["units"]["ohat"])
    # scaling one field by 2^k and back is exact and touches nothing else
    for field, k in EXPONENTS.items():
        buf = raw.clone()
        CR.scale_field_in_place(buf, cfg, fmt, field, k)
        up = CR.decode(buf, cfg, fmt)
        assert torch.equal(up[field].double(), back[field].double() * 2.0 ** k)
        for other in ("h_t", "h_i", "chat", "sg") + tuple(x for x in CR.F16_FIELDS if x != field):
            assert torch.equal(_bits(up[other]), _bits(back[other])), (field, other)
        CR.scale_field_in_place(buf, cfg, fmt, field, -k)
        assert torch.equal(buf, raw)


# ---- 2. the scale rule and the conversion ---------------------------------------------------------------------------------------
def test_scaled_f16_against_the_emulation_and_the_documented_rule():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 264, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-40, 40, (64, 1), generator=g).double())
    assert torch.equal(CR.scaled_f16(x), PE._scaled_f16(x))
    units, scale = CR.scaled_f16_parts(x)
    m = units.double().abs().amax(-1)
    assert ((m >= 0.5) & (m <= 1.0)).all()              # (0.5, 1] before the conversion, which may round down to 0.5 itself
    assert torch.equal(torch.exp2(torch.log2(scale).round()), scale)
    # a row whose max is exactly a power of two: that element's unit is 1.0 (0x3C00), the scale is the max itself
    p = x[:4].clone()
    p = p / p.abs().amax(-1, keepdim=True) * 0.999
    p[:, 7] = 1.0
    p = p * torch.tensor([[1.0], [4.0], [2.0 ** -20], [2.0 ** 100]], dtype=torch.float64)
    units, scale = CR.scaled_f16_parts(p)
    assert torch.equal(scale[:, 0], p[:, 7]) and (units[:, 7].view(torch.int16) == 0x3C00).all()
    assert torch.equal(CR.scaled_f16(p), PE._scaled_f16(p))
    # a zero row: scale 1, zero units; the emulation agrees on the value
    z = torch.zeros(2, 16, dtype=torch.float64)
    units, scale = CR.scaled_f16_parts(z)
    assert (scale == 1).all() and (units.view(torch.int16) == 0).all() and torch.equal(CR.scaled_f16(z), PE._scaled_f16(z))
    # NaN / infinite max: scale 1
    for bad in (float("nan"), float("inf")):
        assert CR.field_scale(torch.tensor([bad])).item() == 1.0
    # a denormal max: the scale stops at 2^-126 (the emulation is not defined below 1e-30: it flushes such a row to zero)
    d = torch.tensor([[1e-40, -3e-41, 0.0, 2e-42]], dtype=torch.float64)
    units, scale = CR.scaled_f16_parts(d)
    assert scale.item() == 2.0 ** -126
    assert torch.equal(units, (d * 2.0 ** 126).float().half()) and units[0, 0].item() > 0
    # the top binade: the scale is clamped to 2^126, the units leave (0.5, 1] but stay finite fp16
    h = torch.randn(1, 264, generator=g, dtype=torch.float64)
    h = h / h.abs().max() * 3e38
    units, scale = CR.scaled_f16_parts(h)
    assert scale.item() == 2.0 ** 126 and torch.isfinite(units).all() and 1.0 < units.double().abs().max().item() <= 4.0
    both_normal = (h.abs() / 2.0 ** 128) >= 2.0 ** -14                 # the emulation scales by 2^128: its units go subnormal earlier
    assert both_normal.sum() > 200
    assert torch.equal(CR.scaled_f16(h)[both_normal], PE._scaled_f16(h)[both_normal])
    # the rule at and around every power of two fp32 can hold
    e = torch.arange(-149, 128)
    p2 = torch.exp2(e.double())
    want = torch.exp2(e.clamp(-126, 126).double())
    assert torch.equal(CR.field_scale(p2), want)
    up = p2 * (1 + 2.0 ** -23)
    assert torch.equal(CR.field_scale(up[e >= -126]), torch.exp2((e[e >= -126] + 1).clamp(-126, 126).double()))


# ---- 3. the restatement is the same model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dataset_name="wikimel", num_candidates_data=20, max_entity_attr_token_len=10, **TINY),
                                dict(num_candidates_data=20, **TINY),
                                dict(num_candidates_data=20, gcn_edge_type="static", **TINY)],
                         ids=["tiny_wikimel", "tiny_wikidiverse", "tiny_wikidiverse_static"])
def test_fields64_through_the_cached_arithmetic_reproduce_the_oracle(kw):
    cfg = DrinConfig(**kw)
    sd = synth.make_state_dict(cfg, 8)
    tables, men, cand = table_case(cfg, 23, 5, 71)
    ib = IndexedBatch(men[:7], EntityTable(*tables), cand, men[12], men[13])
    ref = O.forward(sd, ib.gathered(), dtype=torch.float64, **O.config_kwargs(cfg))
    assert torch.isfinite(ref).all()
    f = CR.fields64(cfg, sd, *tables)
    got = CR.scores_from_fields(cfg, sd, f, men[:7], cand, men[12], men[13])
    err = (got - ref).abs().max().item()
    print(f"{cfg.dataset_name} {cfg.gcn_edge_type}: fields64 through the cached arithmetic vs O.forward in fp64: {err:.2e}")
    assert err <= 1e-12
    # and `scores_with_rounded_cache_fields` without a rounded field is that forward too (dynamic, default activations)
    if cfg.gcn_edge_type == "dynamic":
        assert (PE.scores_with_rounded_cache_fields(sd, ib.gathered()) - ref).abs().max().item() <= 1e-12


# ---- 4. why the consumer test scores one field at a time under a factor -----------------------------------------------------------
def _zero_last_quad(x):
    x = x.clone()
    x[..., -4:] = 0
    return x


def _swap_quads(x):
    """float4 columns 1 and 2 swapped."""
    x = x.clone()
    a, b = slice(4, 8), slice(8, 12)
    x[..., a], x[..., b] = x[..., b].clone(), x[..., a].clone()
    return x


def test_scores_see_a_defect_in_one_field_only_under_its_factor():
    """The guarded case of the measurement this test restates: widths 264 / 520, WikiMEL layout, 4 mentions x 21 candidates drawn
    by `synth.make_device_batch(cfg, 4, 5, "cpu")`, seed-7 weights; every pair's entity rows as one table of B N rows."""
    D, R, B = 264, 520, 4
    cfg = consumer_config(D, R)
    sd = synth.make_state_dict(cfg, 7)
    batch = synth.make_device_batch(cfg, B, 5, "cpu")[:14]
    E = B * cfg.num_candidates_model
    tables = tuple(t.reshape(E, *t.shape[2:]) for t in batch[7:12])
    cand = torch.arange(E).view(B, -1)
    bar = score_bar(D)
    f32 = CR.fields(cfg, sd, *tables, dtype=torch.float32)
    q = CR.scaled_f16
    emu = lambda field, rnd: PE.scores_with_rounded_cache_fields(sd, batch, (field,), rnd=rnd)   # noqa: E731
    clean = PE.scores_with_rounded_cache_fields(sd, batch)
    print(f"\nmax |score change| at D={D} R={R} B={B} N={cfg.num_candidates_model} (bar {bar:g}):")
    print(f"{'field':6} {'2^k':>5} {'zero quad @1':>13} {'swap quads @1':>14} {'zero quad @2^k':>15} {'swap quads @2^k':>16} "
          f"{'fp16 rounding':>14} {'fp32 ref spread f32/mixed':>26} {'scores move':>12}")
    for field, k in EXPONENTS.items():
        s = 2.0 ** k
        unit = {n: (emu(field, d) - clean).abs().max().item() for n, d in (("zero", _zero_last_quad), ("swap", _swap_quads))}
        up = emu(field, lambda x: x * s)
        amp = {n: (emu(field, lambda x, d=d: d(x) * s) - up).abs().max().item() for n, d in (("zero", _zero_last_quad), ("swap", _swap_quads))}
        rounding = (emu(field, q) - clean).abs().max().item()
        moved = (up - clean).abs().max().item()
        # the reference's own spread: the field as torch evaluates it in fp32 against the fp64 field, both stored alike
        x32 = f32[field][cand].double()
        spread = {}
        for name, store in (("f32", lambda x: x), ("mixed", q)):
            a = emu(field, lambda x, st=store: st(x32) * s)
            b = emu(field, lambda x, st=store: st(x) * s)
            spread[name] = (a - b).abs().max().item()
        print(f"{field:6} {k:5d} {unit['zero']:13.2e} {unit['swap']:14.2e} {amp['zero']:15.2e} {amp['swap']:16.2e} {rounding:14.2e} "
              f"{spread['f32']:12.2e} / {spread['mixed']:.2e} {moved:12.2e}")
        if field == "fv_i":                                             # the blind spot: both defects below the bar at unit scale
            assert unit["zero"] < bar and unit["swap"] < bar, unit
        assert min(amp.values()) >= 4 * bar, (field, amp)
        assert max(spread.values()) <= bar / 4, (field, spread)
        assert torch.isfinite(up).all() and moved < 0.5                  # the factor does not saturate the edges into a constant
