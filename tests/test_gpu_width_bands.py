"""-m gpu: the GUARDED width forms of the row kernels against the oracle.

Every width-templated kernel of the scoring and training paths is built tiny (widths up to 256), exact (768 / 2048) and, in
between, guarded: the exact form's register slots behind `c4 < D4` guards, reductions over lanes that hold nothing, LDS rows sized
for 768 / 2048 while the row is shorter.  The other files run the two ends (64 / 128 and 768 / 2048); this one walks a hand-picked
table of widths through the every-path check of tests/helpers.py (inference, training forward, parameter gradients against fp64,
table form, the per-entity cache in both row formats - the fuzz sweep's bars, no new numbers).  Each case first asks
`drin_width_class` which form every family takes at its widths and asserts the band its comment claims, so a gate that moves
turns the case red instead of leaving a form untested (the gates themselves: tests/test_width_class_host.py).

Split-bf16 precision at a width that is no multiple of 32 has no bf16 operand planes: the folded path then runs its fp32 row
kernels with the contractions split on the fly (`planes = false`), training runs layer by layer as ever, and the two routes that
need planes - the table form of the folded path and the per-entity cache - refuse with the library's own error.  The cases assert
exactly that per route: scores inside the bar, or that error; DESIGN.md section 25 has the table.
Measured maxima: profiles/width_bands_parity.txt."""
import ctypes as C

import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig
from drin_amd.model import Model
from oracle import drin_oracle as O
from tests.helpers import config_c, every_path_against_the_oracle, width_class, width_classes

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11
T, G, X, NB = "tiny", "guarded", "exact", "not-built"

# (D, R): the band of each family the case is there for - "family" on fp32 cache rows, "family@mixed" on DRIN_CACHE_MIXED_F16 rows,
# ln_backward: V of k_layernorm_gelu_bwd<V> - and why the width is in the table
WIDTHS = {
    # top of tiny: every lane of the one-quad kernels is full
    (256, 256): dict(entity_stream=T, pair_rows=T, cache_rows=T, cached_pairs=T, ln_backward=1,
                     **{"cache_pack@mixed": T, "cached_pairs@mixed": T}),
    # first D past tiny: 65 / 66 quads, one or two lanes hold a second quad; pair kernels <3,false>, LN backward V = 2
    (260, 64): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=2, **{"cached_pairs@mixed": NB}),
    # ... and the mixed-cache variant of it (mixed rows need widths % 8): k_cache_pack_mixed<3> with one lane past the first slot
    (264, 64): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=2,
                    **{"cache_pack@mixed": G, "cached_pairs@mixed": G}),
    # D tiny, R just past: stream, cache build and fp32 cached pairs go guarded-wide while the pair kernels stay one-quad; mixed
    # cached pairs <1,2> with two lanes in the second image slot
    (64, 264): dict(entity_stream=G, pair_rows=T, cache_rows=G, cached_pairs=G, ln_backward=1,
                    **{"cache_pack@mixed": T, "cached_pairs@mixed": T}),
    # top of the mixed tiny band: <1,2> with the second slot full
    (64, 512): dict(entity_stream=G, pair_rows=T, cached_pairs=G, **{"cached_pairs@mixed": T}),
    # first R past the mixed tiny band
    (64, 520): dict(entity_stream=G, pair_rows=T, cached_pairs=G, **{"cache_pack@mixed": T, "cached_pairs@mixed": G}),
    # mid band, % 32: bf16 planes under split-bf16; LN backward V = 2 with both slots full
    (512, 1024): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=2,
                      **{"cache_pack@mixed": G, "cached_pairs@mixed": G}),
    # R exact, D not: nothing may take EXACT.  % 32
    (736, 2048): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=3,
                      **{"cache_pack@mixed": G, "cached_pairs@mixed": G}),
    # D exact, R not: the pair kernels (and the pack) EXACT while stream, cache build and cached pairs are guarded.  % 32
    (768, 2016): dict(entity_stream=G, pair_rows=X, cache_rows=G, cached_pairs=G, ln_backward=3,
                      **{"cache_pack@mixed": X, "cached_pairs@mixed": G}),
    # one or two quads short of exact in both widths: only the last lanes of the last slot are off.  % 8: mixed cache too
    (760, 2040): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=3,
                      **{"cache_pack@mixed": G, "cached_pairs@mixed": G}),
    # ... % 4 only: fp32 rows
    (764, 2044): dict(entity_stream=G, pair_rows=G, cache_rows=G, cached_pairs=G, ln_backward=3,
                      **{"cache_pack@mixed": NB, "cached_pairs@mixed": NB}),
    # first D the folded path refuses: layer by layer only; LayerNorm forward and backward, fourth slot with one lane
    (772, 128): dict(entity_stream=NB, pair_rows=NB, cache_rows=NB, cached_pairs=NB, ln_backward=4, **{"cached_pairs@mixed": NB}),
    # top of validate_config's D, R > 2048: the generic k_miei; V = 4 with every slot full
    (1024, 2056): dict(entity_stream=NB, pair_rows=NB, cache_rows=NB, cached_pairs=NB, ln_backward=4),
}

# what the library says when a route of the folded model needs bf16 operand planes the width cannot have
TABLE_REFUSAL = r"drin_forward_prepared: entity_index needs the split-bf16 precision"
CACHED_REFUSAL = r"drin_forward_cached: split-bf16 precision needs embed_dim % 32 == 0 \(got \d+\)"


def _config(dataset, D, R, **kw):
    base = dict(dataset_name=dataset, num_candidates_data=5, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
                resnet_num_region=3, max_mention_sentence_len=9, max_entity_attr_token_len=5)
    base.update(kw)
    cfg = DrinConfig(**base)
    cfg.validate()
    return cfg


def _assert_bands(cfg, claims, label):
    """The case's claims against `drin_width_class`; every family's band goes into the printed line."""
    on = {fmt: width_classes(cfg, fmt) for fmt in ("f32", "mixed_f16")}
    for key, want in claims.items():
        family, _, rows = key.partition("@")
        got = on["mixed_f16" if rows == "mixed" else "f32"][family]
        assert got == want, f"{label}: {key} is {got!r}, the case is there for {want!r}"
    f32, mixed = on["f32"], on["mixed_f16"]
    print(f"{label} bands: stream {f32['entity_stream']}, pair {f32['pair_rows']}, cache rows {f32['cache_rows']}, cached pairs "
          f"{f32['cached_pairs']}; mixed rows: pack {mixed['cache_pack']}, cached pairs {mixed['cached_pairs']}; LN backward V = {f32['ln_backward']}")
    return f32


def _refusals(cfg, precision, folded):
    """(table_refusal, cached_refusal) of a split-bf16 case whose widths have no bf16 planes; (None, None) wherever every route scores."""
    D, R = cfg.gcn_embed_dim, cfg.resnet_embed_dim
    if precision != "bf16x3_all" or not folded:
        return None, None
    return (TABLE_REFUSAL if D % 32 or R % 32 else None), (CACHED_REFUSAL if D % 32 else None)


def _gemm_planes_launches(model, batch):
    """Launches of the bf16-planes contraction kernels in one inference call."""
    model.eval()
    with torch.no_grad():
        _lib.profile_begin()
        model(batch[:14])
        prof = _lib.profile_end()
    return prof["gemm_planes"][1]


def _run(cfg, B, precision, label, claims):
    bands = _assert_bands(cfg, claims, label)
    folded = bands["entity_stream"] != NB
    table_refusal, cached_refusal = _refusals(cfg, precision, folded)
    got = every_path_against_the_oracle(cfg, B, precision, SEED, label, table_refusal=table_refusal, cached_refusal=cached_refusal)
    D, R = cfg.gcn_embed_dim, cfg.resnet_embed_dim
    if got["cache"]:
        print(f"{label}: cache rows " + ", ".join(f"{fmt} {e if isinstance(e, str) else format(e, '.1e')}" for fmt, e in got["cache"].items()))
    if precision == "bf16x3_all" and folded:
        # the folded path of a split-bf16 model: its pair-sized contractions on bf16 planes where D and R are multiples of 32, else
        # `planes = false` - the fp32 row kernels, no planes kernel at all
        n = _gemm_planes_launches(got["model"], got["batch"])
        assert (n > 0) == (D % 32 == 0 and R % 32 == 0), f"{label}: {n} planes-kernel launches at D={D} R={R}"
        print(f"{label}: folded path under split-bf16 with planes = {'true' if n else 'false'} ({n} planes launches); table form "
              f"{'refuses' if table_refusal else 'scores'}, cache {'refuses' if cached_refusal else 'scores'}")
    return got


@pytest.mark.parametrize("precision", ["f32", "bf16x3_all"])
@pytest.mark.parametrize("dataset", ["wikidiverse", "wikimel"])
@pytest.mark.parametrize("D,R", list(WIDTHS), ids=[f"{d}x{r}" for d, r in WIDTHS])
def test_width_band_every_path_against_the_oracle(D, R, dataset, precision):
    """B = 3 mentions x 6 candidates, 3 regions, 9 mention tokens, T = 5; WikiDiverse (pooled entity text: TOKENS = false) and
    WikiMEL (token blocks: TOKENS = true)."""
    cfg = _config(dataset, D, R)
    label = f"{D}x{R} {dataset} {precision}"
    if (D, R) == (772, 128):
        assert _lib.load().drin_fused_supported(C.byref(config_c(D, R))) == _lib.E_UNSUPPORTED
        assert b"outside the built instantiations" in _lib.load().drin_last_error()
    _run(cfg, 3, precision, label, WIDTHS[(D, R)])


@pytest.mark.parametrize("precision", ["f32", "bf16x3_all"])
@pytest.mark.parametrize("D,R,N", [(764, 2044, 100), (512, 1024, 100), (64, 520, 100), (512, 1024, 32)],
                         ids=["764x2044_n100", "512x1024_n100", "64x520_n100", "512x1024_n32"])
def test_chunk_tails_at_a_guarded_width(D, R, N, precision):
    """B = 11 mentions: at 100 candidates 1 111 pairs - four 32-candidate chunks with a ragged last one, past the 1 024-pair gates of
    the GEMM module; at 32, one full chunk plus one candidate.  WikiMEL layout (token blocks)."""
    cfg = _config("wikimel", D, R, num_candidates_data=N)
    claims = {k: v for k, v in WIDTHS[(D, R)].items() if k in ("entity_stream", "pair_rows", "cached_pairs", "cached_pairs@mixed")}
    _run(cfg, 11, precision, f"{D}x{R} N={N + 1} B=11 {precision}", claims)


@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("D,R", [(512, 1024), (260, 64)], ids=["512x1024", "260x64"])
def test_generic_activation_twins_at_a_guarded_width(D, R, act):
    """`k_pair_layer1` / `k_pair_final` <3,false,true> and `k_cached_pairs<3,8,false,true>`: the GENERIC_ACT twins of the guarded
    forms (the same bands; the activation picks the twin)."""
    cfg = _config("wikimel", D, R, gcn_vertex_activation=act)
    claims = dict(entity_stream=G, pair_rows=G, cached_pairs=G)
    if D % 8 == 0:
        claims["cached_pairs@mixed"] = G
    for precision in ("f32", "bf16x3_all"):
        _run(cfg, 3, precision, f"{D}x{R} {act} {precision}", claims)
    # at the exact width a generic activation has no exact form: the library says so
    assert width_class(768, 2048, "pair_rows", vertex_activation=act) == G
    assert width_class(768, 2048, "cached_pairs", vertex_activation=act) == G


def test_static_edges_mixed_pack_with_zero_units():
    """Static edges at (512, 1024): the mixed-f16 cache rows carry no edge-update fields - `k_cache_pack_mixed<3>` packs zero
    units under unit scales - and the cached pairs read none."""
    cfg = _config("wikidiverse", 512, 1024, gcn_edge_type="static")
    claims = {"cache_rows": G, "cache_pack@mixed": G, "cached_pairs@mixed": G}
    for precision in ("f32", "bf16x3_all"):
        got = _run(cfg, 3, precision, f"512x1024 static {precision}", claims)
        assert got["cache"].keys() == {"f32", "mixed_f16"}


def test_bf16_stored_features_at_a_guarded_width():
    """FT = __bf16 instantiations of the guarded stream kernel at (512, 1024) - image and object rows in the PAIR layout, eight
    columns per lane and load - on the folded path: inputs and bar of tests/test_gpu_parity.py::test_bf16_stored_features (the
    oracle on the same stored values widened to fp32, 1e-5; the library's own fp32-feature run, 4e-6)."""
    feature_slots = (0, 4, 5, 7, 9, 10)
    for dataset in ("wikidiverse", "wikimel"):
        cfg = _config(dataset, 512, 1024)
        assert width_classes(cfg)["entity_stream"] == G
        sd = synth.make_state_dict(cfg, 9)
        stored = [t.to(torch.bfloat16) if i in feature_slots else t for i, t in enumerate(synth.make_batch(cfg, 3, 31)[:14])]
        widened = [t.float() if t.dtype == torch.bfloat16 else t for t in stored]
        ref = O.forward(sd, widened, **O.config_kwargs(cfg))
        assert torch.isfinite(ref).all()
        model = Model(cfg, precision="bf16x3_all").to(DEV).eval()
        model.load_state_dict(sd)
        with torch.no_grad():
            _lib.profile_begin()
            s_bf16 = model([t.to(DEV) for t in stored])
            prof = _lib.profile_end()
            s_f32 = model([t.to(DEV) for t in widened])
        assert prof["stream"][1] == 1, "the fused path reads the bf16 features in place"
        err, own = (s_bf16.cpu() - ref).abs().max().item(), (s_bf16 - s_f32).abs().max().item()
        print(f"512x1024 {dataset} bf16-stored features: max |score - oracle(widened)| = {err:.3e}, vs fp32-feature run {own:.3e}")
        assert err <= 1e-5 and own <= 4e-6
