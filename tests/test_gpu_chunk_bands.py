"""-m gpu: the CANDIDATE-CHUNK and TOKEN-COUNT bands of the scoring kernels against the oracle.

The inference kernels cut a mention's candidate list into workgroups by the size of the call - the folded path 16 / 48 / 128
candidates per workgroup below 1 024 / below 2 048 / from 2 048 mentions (`FusedLayout::build`), the cached path 16, or 64 / 128 in
its exact instantiation (`cached_chunk_candidates`) - and every kernel re-derives `per = ceil(N / chunks)`, wave w of a workgroup
taking candidates `n_begin + w + 4 k`.  The list lengths here sit on the boundaries of that walk: one chunk (the direct-layout branch
of `k_entity_stream`), N = S, S +- 1, 2 S, a ragged last chunk of one candidate with three idle waves, `chunks` of 4 / 5 / 8 / 9
(the four-at-a-time loop of `k_reduce_stream_partials` with and without its tail), one / four / eight full 16-candidate groups of
`k_cached_pairs` and a last group of one.  Each case first asks `drin_workgroups_per_mention` which cut its call takes and asserts
the count its table claims, so a gate that moves turns the case red instead of leaving a form untested (the gates themselves:
tests/test_chunk_bands_host.py).  Every inference route is scored twice and must give the same bits.

The bars are the project's own: 1e-5 in exact fp32 and in `Model()`'s default precision, 2e-5 in `bf16x3_all`, 3e-5 for
`mixed_f16` cache rows at D < 256.  At B >= 1 024 the oracle scores the first, middle and last four mentions, and the WHOLE
output is held, at the same bar, to the same mentions scored in calls of 512 - the 16-candidate cut that section (a) pins - which
is the check that sees a wrong workgroup anywhere in the grid.

The token walk of `k_entity_stream` is a second count loop: section (e) writes the entity mask itself, so that a chosen number of
kept tokens lands on every boundary of the 8-unrolled, flat (two bf16 rows at a time), 4-unrolled and scalar-tail walks, and on both
sides of the 64-lane mask count.

DESIGN.md section 27 maps the cases to the boundaries; measured maxima and times: profiles/chunk_bands_parity.txt."""
import functools

import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig
from drin_amd.model import EntityTable, IndexedBatch, Model, _split_mentions
from oracle import drin_oracle as O
from tests.helpers import every_path_against_the_oracle, width_classes, workgroups_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
E = 23                                   # rows of the entity table behind every table-form case
FEATURE_SLOTS = (0, 4, 5, 7, 9, 10)      # the six feature tensors of the 14-sequence


def _config(dataset, N, D, R, T=5, **kw):
    base = dict(dataset_name=dataset, num_candidates_data=N - 1, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
                resnet_num_region=3, max_mention_sentence_len=9, max_entity_attr_token_len=T)
    base.update(kw)
    cfg = DrinConfig(**base)
    cfg.validate()
    return cfg


def _per(N, chunks):
    return -(-N // chunks)


def _bar(precision, D, fmt=None):
    tol = 2e-5 if precision == "bf16x3_all" else 1e-5
    return 3e-5 if fmt == "mixed_f16" and D < 256 else tol


def _assert_cut(cfg, B, precision, label, folded=None, cached=None):
    """The case's claims against `drin_workgroups_per_mention`; returns what the library answers for both paths."""
    got_f = workgroups_of(cfg, B, False, precision)
    got_c = workgroups_of(cfg, B, True, precision, num_entities=E)
    if folded is not None:
        assert got_f == folded, f"{label}: the folded path cuts the list into {got_f} workgroups, the case is there for {folded}"
    if cached is not None:
        assert got_c == cached, f"{label}: the cached path cuts the list into {got_c} workgroups, the case is there for {cached}"
    return got_f, got_c


@functools.lru_cache(maxsize=8)
def _state(D, R, act):
    return synth.make_state_dict(_config("wikidiverse", 2, D, R, gcn_vertex_activation=act), 7)


def _model(cfg, precision):
    model = (Model(cfg) if precision == "bf16x3" else Model(cfg, precision=precision)).to(DEV).eval()
    if precision == "bf16x3":
        assert model.precision == _lib.PREC_BF16X3          # `Model()`'s default arithmetic
    model.load_state_dict(_state(cfg.gcn_embed_dim, cfg.resnet_embed_dim, cfg.gcn_vertex_activation))
    model.validate_indices = False
    return model


def _table_batch(cfg, B, seed, men):
    """An `IndexedBatch` of the mention side `men` over an E-row `EntityTable`, as tests/helpers.py builds it."""
    N = cfg.num_candidates_model
    tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1), 1, seed % 1000 + 7)
    table = EntityTable(tab[7][0], tab[8][0] if cfg.token_level_entities else None, tab[9][0], tab[10][0], tab[11][0]).to(DEV)
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, E, (B, N), generator=g).to(DEV)
    sims = (20.0 + 5.0 * torch.randn(2, B, N, generator=g)).to(DEV)
    return IndexedBatch(list(men[:7]), table, cand, sims[0], sims[1])


def _rows_of(batch, rows):
    if isinstance(batch, IndexedBatch):
        return IndexedBatch([t[rows] for t in batch.mention], batch.table, batch.candidates[rows],
                            batch.miet_similarity[rows], batch.mtei_similarity[rows])
    return [t[rows] for t in batch]


def _host(batch):
    seq = batch.gathered() if isinstance(batch, IndexedBatch) else batch
    return [t.cpu() for t in seq[:14]]


def _sampled(B):
    """First, middle and last four mentions (all of them when the call has fewer)."""
    rows = sorted(set(range(min(4, B))) | set(range(max(0, B // 2 - 2), min(B, B // 2 + 2))) | set(range(max(0, B - 4), B)))
    return torch.tensor(rows, device=DEV)


def _score_routes(cfg, B, precision, label, band, seed, routes=("gathered", "table", "f32", "mixed_f16"), folded=None, cached=None):
    """Inference only.  Every route of `routes` - the gathered 14-sequence, the table form without a cache, the per-entity cache
    in either row format - for B mentions: the cut asserted first, two runs the same bits, the sampled mentions against the oracle
    at the route's bar and, from B > 512, the whole output against calls of 512 at the same bar.  One printed line per route."""
    N, D = cfg.num_candidates_model, cfg.gcn_embed_dim
    got_f, got_c = _assert_cut(cfg, B, precision, label, folded, cached)
    model = _model(cfg, precision)
    sd = _state(D, cfg.resnet_embed_dim, cfg.gcn_vertex_activation)
    cache_only = set(routes) <= {"f32", "mixed_f16"}         # then the per-pair entity rows are not needed: a lone answer slot
    full = synth.make_device_batch(cfg.with_(num_candidates_data=0) if cache_only else cfg, B, seed, DEV)[:14]
    ib = _table_batch(cfg, B, seed, full)
    rows = _sampled(B)
    refs, errs = {}, {}
    with torch.no_grad():
        for route in routes:
            batch = full if route == "gathered" else ib
            if route in ("f32", "mixed_f16"):
                ib.table.enable_cache(True, format=route)
            else:
                ib.table.enable_cache(False)
            chunks = got_c if route in ("f32", "mixed_f16") else got_f
            out = model(batch)
            assert out.shape == (B, N) and torch.isfinite(out).all(), f"{label} {route}"
            assert torch.equal(out, model(batch)), f"{label} {route}: a second run gives other bits"
            kind = "gathered" if route == "gathered" else "table"
            if kind not in refs:
                refs[kind] = O.forward(sd, _host(_rows_of(batch, rows)), **O.config_kwargs(cfg))
                assert torch.isfinite(refs[kind]).all(), f"{label}: a degenerate draw - the oracle's scores are not all finite"
            tol = _bar(precision, D, route if route in ("f32", "mixed_f16") else None)
            err = (out[rows].cpu() - refs[kind]).abs().max().item()
            small = None
            if B > 512:
                parts = torch.cat([model(part) for part in _split_mentions(batch, 512)], 0)
                small = (out - parts).abs().max().item()
            print(f"chunk band {band}: N={N} chunks={chunks} per={_per(N, chunks)} B={B} D={D} R={cfg.resnet_embed_dim} {cfg.dataset_name} "
                  f"{precision} path={route}: max |score - oracle| {err:.2e} over {len(rows)} mentions"
                  + (f", whole output against calls of 512 {small:.2e}" if small is not None else ""))
            assert err <= tol, f"{label} {route}: {err:.2e} > {tol}"
            if small is not None:
                assert small <= tol, f"{label} {route}: {small:.2e} from the same mentions in calls of 512 (> {tol})"
            errs[route] = (err, small)
    ib.table.enable_cache(False)
    model.check_indices()                                    # every candidate row was inside the table
    return errs


# ---- (a) the 16-candidate band, every path ----------------------------------------------------------------------------------------
# N: (chunks, what the length hits)
BAND_16 = {
    1: (1, "direct-layout branch, one candidate: waves 1-3 idle"), 2: (1, "direct layout"), 3: (1, "direct layout"),
    4: (1, "direct layout, one candidate per wave"), 5: (1, "direct layout, wave 0 takes two"), 16: (1, "a full chunk"),
    17: (2, "per = 9: uneven waves"), 20: (2, "per = 10"), 21: (2, "per = 11, a last chunk of 10"), 33: (3, "per = 11"),
    49: (4, "one unrolled trip of the reduce, no tail; last chunk of 10"), 64: (4, "four full chunks"),
    65: (5, "one trip plus a tail of 1"), 81: (6, "per = 14: a trip plus a tail of 2"), 113: (8, "two trips, no tail"),
    129: (9, "two trips plus a tail of 1"),
}


@pytest.mark.parametrize("precision", ["f32", "bf16x3_all"])
@pytest.mark.parametrize("dataset", ["wikidiverse", "wikimel"])
@pytest.mark.parametrize("N", list(BAND_16))
def test_16_candidate_band_every_path_against_the_oracle(N, dataset, precision):
    """B = 3 mentions at D = 64 / R = 128, T = 5, through the every-path check of tests/helpers.py: inference on the folded path,
    the training forward, the parameter gradients against fp64 (the layer-by-layer kernels loop four candidates at a time plus a
    tail: `k_layer_aggregate`), the table form and both cache formats (from N = 2: a lone answer slot has no table form in the
    helper).  The whole-batch fp64 gradient check stays on at every N: the largest case is 387 pairs."""
    chunks, _why = BAND_16[N]
    cfg = _config(dataset, N, 64, 128)
    label = f"16-band N={N} {dataset} {precision}"
    _assert_cut(cfg, 3, precision, label, folded=chunks, cached=chunks)
    got = every_path_against_the_oracle(cfg, 3, precision, 100 + N, label, same_bits=True)
    cache = ", ".join(f"cache {fmt} {e:.1e}" for fmt, e in got["cache"].items())
    print(f"chunk band 16: N={N} chunks={chunks} per={_per(N, chunks)} B=3 D=64 R=128 {dataset} {precision} path=every: inference "
          f"{got['inference']:.1e} training {got['training']:.1e} table {got['table'] if got['table'] is None else format(got['table'], '.1e')}"
          + (f" {cache}" if cache else ""))
    if N >= 2:
        assert got["cache"].keys() == {"f32", "mixed_f16"} and got["table"] is not None


# ---- (b), (c) the 48- and the 128-candidate band of the folded path -----------------------------------------------------------------
BAND_48 = {1: 1, 47: 1, 48: 1, 49: 2, 97: 3, 145: 4, 193: 5, 385: 9}       # N: chunks at 1 024 <= B < 2 048
BAND_128 = {1: 1, 5: 1, 127: 1, 128: 1, 129: 2, 257: 3, 385: 4, 513: 5}    # N: chunks at B >= 2 048


def _large_call_cases():
    out = []
    for band, B, table, guarded_n, mel_n in (("48", 1024, BAND_48, 49, (49, 97)), ("128", 2048, BAND_128, 129, (129, 257))):
        out += [(band, B, N, 64, 64, "wikidiverse", table[N]) for N in table]
        out += [(band, B, guarded_n, 320, 512, "wikidiverse", table[guarded_n])]
        out += [(band, B, N, 64, 64, "wikimel", table[N]) for N in mel_n]
    out += [("48", 2047, 49, 64, 64, "wikidiverse", 2),     # the top of the band
            ("16", 1023, 49, 64, 64, "wikidiverse", 4)]     # ... and one mention below it: the gate itself
    return out


@pytest.mark.parametrize("precision", ["f32", "bf16x3_all"])
@pytest.mark.parametrize("band,B,N,D,R,dataset,chunks", _large_call_cases(),
                         ids=[f"band{c[0]}_b{c[1]}_n{c[2]}_{c[3]}x{c[4]}_{c[5]}" for c in _large_call_cases()])
def test_large_call_bands_of_the_folded_path(band, B, N, D, R, dataset, chunks, precision):
    """48 candidates per workgroup from 1 024 mentions, 128 from 2 048: the gathered batch, the table form and both cache formats
    (the cached path keeps 16 candidates at these widths: `ceil(N / 16)` workgroups at any B).  D = 64 / R = 64, one guarded pair
    (320 / 512) per band, WikiDiverse layout plus WikiMEL with T = 5 at the two smallest multi-chunk lengths."""
    cfg = _config(dataset, N, D, R)
    label = f"{band}-band B={B} N={N} {D}x{R} {dataset} {precision}"
    _score_routes(cfg, B, precision, label, band, 200 + N, folded=chunks, cached=-(-N // 16))


# ---- (d) the group walk of the cached exact form ----------------------------------------------------------------------------------
# N: (chunks, what the 16-candidate groups of a workgroup look like) at B < 2 048: 64 candidates per workgroup
EXACT_GROUPS = {
    1: (1, "one group of one candidate"), 3: (1, "wave 3 idle"), 4: (1, "one candidate per wave"), 5: (1, "wave 0 takes two"),
    16: (1, "one full group, no look-ahead"), 17: (1, "a second group of one candidate, waves 1-3 idle"),
    63: (1, "three groups plus a ragged one of 15"), 64: (1, "exactly four groups"), 65: (2, "per = 33: 16 + 16 + 1"),
    80: (2, "per = 40: 16 + 16 + 8"), 81: (2, "per = 41, a last chunk of 40"), 129: (3, "per = 43"), 257: (5, "per = 52"),
}


def _exact_config(N, act="gelu"):
    return _config("wikimel", N, 768, 2048, T=4, max_mention_sentence_len=16, resnet_num_region=4, gcn_vertex_activation=act)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("N", list(EXACT_GROUPS))
def test_cached_exact_form_group_walk(N, precision):
    """D = 768 / R = 2048, gelu, B = 2 in table form through both cache formats: `k_cached_pairs<3, 8, true>` walks a chunk of up to
    64 candidates in groups of 16 with the index / row look-ahead across the group boundary."""
    cfg = _exact_config(N)
    assert width_classes(cfg)["cached_pairs"] == "exact" and width_classes(cfg, "mixed_f16")["cached_pairs"] == "exact"
    _score_routes(cfg, 2, precision, f"cached exact N={N} {precision}", "cached-64", 300 + N, routes=("f32", "mixed_f16"),
                  cached=EXACT_GROUPS[N][0])


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("N,chunks", [(128, 1), (129, 2)], ids=["n128_eight_full_groups", "n129_per_65"])
def test_cached_exact_form_128_candidate_workgroups(N, chunks, precision):
    """B = 2 048: 128 candidates per workgroup - one chunk of eight full groups, then two chunks of `per` = 65 (16 x 4 + 1).  Twelve
    mentions against the oracle, the whole output against calls of 512 (64 candidates per workgroup)."""
    cfg = _exact_config(N)
    assert workgroups_of(cfg, 512, True, precision, num_entities=E) == -(-N // 64)
    _score_routes(cfg, 2048, precision, f"cached exact B=2048 N={N} {precision}", "cached-128", 400 + N, routes=("f32", "mixed_f16"),
                  cached=chunks)


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
def test_exact_widths_with_silu_vertices_keep_one_group_per_workgroup(precision):
    """768 / 2048 with silu vertices, N = 65: `k_cached_pairs<3, 8, false, true>` - five workgroups of `per` = 13, the one-group
    form at the exact widths."""
    cfg = _exact_config(65, act="silu")
    assert width_classes(cfg)["cached_pairs"] == "guarded"
    _score_routes(cfg, 2, precision, f"cached 768x2048 silu N=65 {precision}", "cached-16", 365, routes=("f32", "mixed_f16"), cached=5)


@pytest.mark.parametrize("route,precision", [("table", "bf16x3_all"), ("f32", "bf16x3_all")], ids=["k_entity_stream", "k_cached_pairs"])
def test_out_of_range_index_at_the_end_of_a_ragged_last_chunk(route, precision):
    """B = 2 048 x N = 129 at D = 64: the folded path walks two chunks of `per` = 65 (the last one 64 long), the cached path nine of
    `per` = 15 (the last one 9 long).  A candidate row past the table, planted at the LAST candidate of one mention: the kernels
    clamp and report it - `Model.check_indices()` raises and names the pair - and every other mention scores the bits of the
    clean run."""
    B, N, b0 = 2048, 129, 1500
    cfg = _config("wikidiverse", N, 64, 64)
    label = f"bad index, {route}"
    _assert_cut(cfg, B, precision, label, folded=2, cached=9)
    model = _model(cfg, precision)
    men = synth.make_device_batch(cfg.with_(num_candidates_data=0), B, 77, DEV)
    good = _table_batch(cfg, B, 78, men)
    good.table.enable_cache(route != "table", format="f32")
    rows = good.candidates.clone()
    rows[b0, N - 1] = E + 7
    bad = IndexedBatch(good.mention, good.table, rows, good.miet_similarity, good.mtei_similarity)
    clamped = IndexedBatch(good.mention, good.table, rows.clamp(0, E - 1), good.miet_similarity, good.mtei_similarity)
    others = torch.arange(B, device=DEV) != b0
    with torch.no_grad():
        s_good = model(good)
        model.check_indices()                                         # nothing to report
        s_bad = model(bad)
        with pytest.raises(IndexError, match=rf"row {E + 7} at pair {b0 * N + N - 1} "):
            model.check_indices()
        model.check_indices()                                         # cleared by the raise
        assert torch.equal(s_bad[others], s_good[others]), f"{label}: a mention other than the planted one changed"
        assert torch.equal(s_bad, model(clamped))                     # the planted pair scored the clamped row
        model.check_indices()
    good.table.enable_cache(False)
    print(f"chunk band bad-index: N={N} chunks={2 if route == 'table' else 9} per={65 if route == 'table' else 15} B={B} path={route}: "
          f"reported, {int(others.sum())} other mentions bit-equal, max |planted mention - clean| "
          f"{(s_bad[b0] - s_good[b0]).abs().max().item():.2e}")


# ---- (e) token counts on the boundaries of the stream kernel's token walk -----------------------------------------------------------
KEPT = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 17)       # kept tokens (`stop - 1`): every trip count and tail of the 8 / 4 / 2 / 1 walks
TOKEN_WIDTHS = {"tiny": (64, 128), "guarded": (320, 512), "exact": (768, 2048)}


def _kept_counts(B, N, T):
    """[B, N] kept-token counts.  T = 20: `KEPT` cycled over the candidates, shifted by one per (mention, chunk of 13) so that the
    four waves of a workgroup (candidates `n_begin + w + 4 k`) meet different counts in every chunk: wave 0 (four slots a chunk)
    meets all thirteen, waves 1-3 (three slots a chunk, twelve in all) twelve of them each.  Longer T: T - 2 (every token is a mask
    token) and 1, alternating."""
    if T == 20:
        return torch.tensor([[KEPT[(n + 2 * b + n // 13) % len(KEPT)] for n in range(N)] for b in range(B)])
    return torch.tensor([[T - 2 if (n + b) % 2 == 0 else 1 for n in range(N)] for b in range(B)])


def test_token_count_table_reaches_every_wave():
    """The claim of `_kept_counts`, from the walk `n_begin + w + 4 k` over two chunks of `per` = 13 (needs no device)."""
    kept = _kept_counts(2, 26, 20)
    met = {w: set() for w in range(4)}
    for b in range(2):
        for n in range(26):
            met[(n % 13) % 4].add(int(kept[b, n]))
    assert met[0] == set(KEPT) and all(len(met[w]) == 12 for w in (1, 2, 3))
    assert set.union(*(set(KEPT) - met[w] for w in (1, 2, 3))) == {1, 2, 3}      # each missing count is met by the three other waves


@pytest.mark.parametrize("T", [20, 63, 64, 65, 129])
@pytest.mark.parametrize("features", ["f32", "bf16"])
@pytest.mark.parametrize("width", list(TOKEN_WIDTHS))
def test_token_counts_on_the_walk_boundaries(width, features, T):
    """WikiMEL layout on the folded path, B = 2, N = 26 (N = 5 at T = 129 and the exact width), the entity mask written here.  fp32
    rows: the 4-unrolled walk and its scalar tail in the tiny, guarded and exact forms (exact fp32, 1e-5).  bf16-stored rows, read
    in place (`bf16x3_all`, 2e-5, against the oracle on the stored values widened to fp32): the 8-unrolled walk at DV = 1, the
    guarded 4-unrolled one, the flat two-rows-at-a-time walk at D = 768.  T > 64: a second trip of the 64-lane mask count."""
    D, R = TOKEN_WIDTHS[width]
    B, N = 2, 5 if (T == 129 and width == "exact") else 26
    cfg = _config("wikimel", N, D, R, T=T)
    precision = "bf16x3_all" if features == "bf16" else "f32"
    label = f"token walk {width} {features} T={T}"
    assert width_classes(cfg)["entity_stream"] == width
    chunks, _ = _assert_cut(cfg, B, precision, label, folded=1 if N == 5 else 2)
    batch = synth.make_batch(cfg, B, 500 + T)[:14]
    kept = _kept_counts(B, N, T)
    batch[8] = (torch.arange(T)[None, None, :] < (kept + 2)[:, :, None]).to(torch.int64)      # mean over tokens 1 .. ntok - 2
    assert int(batch[8].sum(-1).max()) <= T
    if features == "bf16":
        batch = [t.to(torch.bfloat16) if i in FEATURE_SLOTS else t for i, t in enumerate(batch)]
    widened = [t.float() if t.dtype == torch.bfloat16 else t for t in batch]
    ref = O.forward(_state(D, R, "gelu"), widened, **O.config_kwargs(cfg))
    assert torch.isfinite(ref).all()
    model = _model(cfg, precision)
    dbatch = [t.to(DEV) for t in batch]
    with torch.no_grad():
        _lib.profile_begin()
        out = model(dbatch)
        prof = _lib.profile_end()
        assert prof["stream"][1] == 1, f"{label}: the folded path reads the rows in place, one pass of the stream kernel"
        assert torch.equal(out, model(dbatch)), f"{label}: a second run gives other bits"
    err, tol = (out.cpu() - ref).abs().max().item(), _bar(precision, D)
    print(f"chunk band tokens: N={N} chunks={chunks} per={_per(N, chunks)} B={B} D={D} R={R} T={T} {features} rows {precision} path=gathered "
          f"kept counts {sorted(set(kept.flatten().tolist()))}: max |score - oracle| {err:.2e}")
    assert err <= tol, f"{label}: {err:.2e} > {tol}"

