"""-m gpu: the rows of the per-entity cache (`drin_build_entity_cache`: `k_entity_cache_rows`, `k_cache_pack_mixed`, four table-sized
GEMMs; read by `k_cached_pairs`), FIELD BY FIELD against fp64 (tests/cache_rows_restatement.py).

Every other test of the cache looks at final scores, and the scores are nearly blind to three of the seven fields - that is why
those three may be fp16 at all (tests/test_cache_rows_host.py asserts the blindness).  Here:
  A. the builder: every field of every row of a 37-row table decoded from `table._cache` and compared with the restatement -
     slack from the reference's own fp32 (or emulated split-bf16) distance to fp64, half an fp16 ulp derived - plus the exact
     properties of the scale rule, the tail and the static-edge rows;
  B. the consumer: one fp16 field at a time multiplied by an exact 2^k inside the built cache, scored, and compared with the fp64
     emulation under the same factor, at the bar the cached path's score tests already use;
  C. fields nobody may read are filled with NaN: the scores keep their bits;
  D. a table of one builder slab (262 144 rows) plus five: the rows on both sides of the slab boundary, and every row's c^ and sg.
Measured maxima and the deliberately wrong libraries this file was run against: profiles/cache_rows_parity.txt."""
import pytest
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig
from drin_amd.model import EntityTable, IndexedBatch, Model
from oracle import precision_emulation as PE
from tests import cache_rows_restatement as CR
from tests.helpers import width_classes
from tests.test_cache_rows_host import EXPONENTS, consumer_config, score_bar, table_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, G, X = "tiny", "guarded", "exact"
MARGIN = 5                                                  # as tests/helpers.py takes for gradients against the fp32 oracle's distance
E_ROWS, MENTIONS = 37, 3                                    # 37 rows: the last workgroup of the one-wave-per-entity kernels has one live wave
TOKENS = 10
TOKEN_COUNTS = (0, 1, 2, 3, 6, 7, 10)                       # rows 0 .. 6 of a token-level table: the slice corners and the 4-unrolled loop's tails
ROW_ZERO_IMAGE, ROW_ZERO_OBJECT, ROW_ZERO_SCORES, ROW_TINY_OBJECT, ROW_ONE_HOT, ROW_ONE_HOT_X3 = 8, 9, 10, 11, 12, 13
SEED = 71

# (D, R): (cache_rows band, cache_pack band on mixed rows)
BANDS = {(64, 128): (T, T), (512, 1024): (G, G), (768, 2048): (X, X), (264, 64): (G, G), (64, 520): (G, T), (760, 2040): (G, G)}
BUILDER_CASES = [(D, R, p) for (D, R) in ((64, 128), (512, 1024), (768, 2048)) for p in ("f32", "bf16x3_all")] + \
                [(D, R, "f32") for (D, R) in ((264, 64), (64, 520), (760, 2040))]


def _model(cfg, sd, precision):
    m = Model(cfg, precision=precision).to(DEV).eval()
    m.load_state_dict(sd)
    return m


def _on_device(tables, men, cand):
    table = EntityTable(*tables).to(DEV)
    return table, IndexedBatch([t.to(DEV) for t in men[:7]], table, cand.to(DEV), men[12].to(DEV), men[13].to(DEV))


def _assert_bands(cfg, D, R, fmt):
    got = width_classes(cfg, fmt)
    assert got["cache_rows"] == BANDS[(D, R)][0], (D, R, fmt, got)
    if fmt == "mixed_f16":
        assert got["cache_pack"] == BANDS[(D, R)][1], (D, R, got)


def _planted_tables(cfg, seed):
    """A 37-row table with the rows this file is about planted in it (host tensors)."""
    tables, men, _ = table_case(cfg, E_ROWS, MENTIONS, seed)
    text, mask, image, obj, score = [None if t is None else t.clone() for t in tables]
    if mask is not None:
        for e, n in enumerate(TOKEN_COUNTS):
            mask[e] = (torch.arange(TOKENS) < n).to(mask.dtype)
    image[ROW_ZERO_IMAGE] = 0
    obj[ROW_ZERO_OBJECT] = 0
    score[ROW_ZERO_SCORES] = 0
    tiny = obj[ROW_TINY_OBJECT, 0]
    tiny *= 1e-12 / tiny.norm()                             # below cosine_eps = 1e-8: the clamp, not the norm, divides
    if cfg.object_topk_entity == 1:
        for row, col, es in ((ROW_ONE_HOT, 5, 1.0), (ROW_ONE_HOT_X3, cfg.resnet_embed_dim - 3, 3.0)):
            obj[row] = 0
            obj[row].view(-1)[col] = 1.0
            score[row, 0] = es
    cand = 7 + torch.randint(0, E_ROWS - 7, (MENTIONS, cfg.num_candidates_model), generator=torch.Generator().manual_seed(seed))
    return (text, mask, image, obj, score), men, cand


def _row_slack(ref, err):
    """[rows]: MARGIN x the largest |err| of the row, at least 4 fp32 ulps of the row's largest |ref| (NaN rows: compared by pattern)."""
    if ref.dim() == 1:
        ref, err = ref[:, None], err[:, None]
    top = ref.abs().nan_to_num(0.0).amax(-1)
    ulp = torch.where(top > 0, torch.exp2(torch.floor(torch.log2(top.clamp_min(1e-300))) - 23), torch.zeros_like(top))
    return torch.maximum(MARGIN * err.abs().nan_to_num(0.0).amax(-1), 4 * ulp)


def _slacks(cfg, sd, tables, f64, precision):
    """{field: [rows]} - the reference's own distance from fp64.  f32 model: the field as torch evaluates it in fp32 on the host.
    bf16x3_all model: what a split-bf16 product of the field's table-sized GEMM misses (`_rounded_product_error(., ., "x3")`);
    the fields no GEMM touches (c^, o^, sg) are fp32 row arithmetic in every precision."""
    f32 = CR.fields(cfg, sd, *tables, dtype=torch.float32)
    err = {k: f32[k].double() - f64[k] for k in ("h_t", "h_i", "fv_t", "fv_i", "chat", "ohat", "sg")}
    if precision == "bf16x3_all":
        fw = CR.folded_weights64(sd)
        image = tables[2].double()
        x = {"t": f64["x_t"], "i": image.mean(-2) if image.dim() == 3 else image}
        for k in ("h_t", "h_i", "fv_t", "fv_i"):
            err[k] = PE._rounded_product_error(x[k[-1]], fw[k], "x3")
    return {k: _row_slack(f64[k], e) for k, e in err.items()}, f32


def _check_f32_field(name, got, ref, slack, label, misses):
    """|got - ref| <= slack per element; the same NaN pattern.  Returns (max |err|, max err / slack); an element past its slack
    goes into `misses` (asserted empty at the end of the case, so that one miss does not hide the checks behind it)."""
    if ref.dim() == 1:
        got, ref = got[:, None], ref[:, None]
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"{label} {name}: NaN pattern differs from the restatement's"
    err = (got.double() - ref).abs()
    fin = ~torch.isnan(ref)
    over = fin & (err > slack[:, None])
    if over.any():
        r, c = over.nonzero()[(err / slack[:, None].clamp_min(1e-300))[over].argmax()].tolist()
        misses.append(f"{label} {name}: {int(over.sum())} element(s) in {int(over.any(-1).sum())} row(s) past their slack, worst (row {r}, col {c}): "
                      f"|err| {err[r, c].item():.3e} > slack {slack[r].item():.3e} ({MARGIN * err[r, c].item() / slack[r].item():.1f} x the reference's own distance)")
    ratio = (err / slack[:, None].clamp_min(1e-300))[fin & (slack[:, None] > 0)]
    return err[fin].max().item(), (ratio.max().item() if ratio.numel() else 0.0)


def _is_pow2_in_range(s):
    mant, exp = torch.frexp(s.double())
    return (mant == 0.5) & (exp >= -125) & (exp <= 127)


def _check_f16_field(name, units, scale, ref, slack, label, misses):
    """The mixed rows' form of a field: power-of-two scale in range, largest |unit| in (0.5, 1] (0.5 itself only by rounding), |unit x scale - ref| <= 2^-12 scale
    + slack (half an fp16 ulp of the top binade, derived), the restatement's scale unless the row's max is within slack of a
    power of two.  Returns (max |err|, max err / bound, the rows that used that excuse)."""
    assert _is_pow2_in_range(scale).all(), f"{label} {name}: a scale is no power of two in [2^-126, 2^126]: {scale[~_is_pow2_in_range(scale)][:4].tolist()}"
    nan_row, top = torch.isnan(ref).any(-1), ref.abs().nan_to_num(0.0).amax(-1)
    assert torch.equal(torch.isnan(units), torch.isnan(ref)), f"{label} {name}: NaN pattern differs from the restatement's"
    assert (scale[nan_row] == 1).all(), f"{label} {name}: a NaN row carries a scale other than 1"
    zero_row = ~nan_row & (top == 0)
    assert (scale[zero_row] == 1).all() and (units[zero_row] == 0).all(), f"{label} {name}: a zero row is not zero units under scale 1"
    live = ~nan_row & ~zero_row
    umax = units.double().abs().amax(-1)
    s = scale.double()
    # max |x| / scale lies in (0.5, 1]; the conversion may round a largest element within half an ulp above 0.5 down to 0.5 itself
    in_range = ((umax > 0.5) | ((umax == 0.5) & (top <= (0.5 + 2.0 ** -12) * s + slack))) & (umax <= 1.0)
    assert in_range[live].all(), f"{label} {name}: largest |unit| outside (0.5, 1]: {umax[live & ~in_range][:4].tolist()}"
    bound = 2.0 ** -12 * s + slack
    err = (units.double() * s[:, None] - ref).abs()
    over = live[:, None] & (err > bound[:, None])
    if over.any():
        r, c = over.nonzero()[(err / bound[:, None])[over].argmax()].tolist()
        misses.append(f"{label} {name}: {int(over.sum())} element(s) in {int(over.any(-1).sum())} row(s) past their bound, worst (row {r}, col {c}): "
                      f"|err| {err[r, c].item():.3e} > 2^-12 scale {2.0 ** -12 * s[r].item():.3e} + slack {slack[r].item():.3e}")
    want = CR.field_scale(top)
    differs = live & (s != want)
    excused = []
    for r in differs.nonzero().flatten().tolist():
        edge = min(s[r].item(), want[r].item())            # the power of two the two maxima lie on either side of
        assert abs(top[r].item() - edge) <= slack[r].item() and max(s[r].item(), want[r].item()) == 2 * edge, \
            f"{label} {name}: row {r} has scale {s[r].item():g}, the restatement {want[r].item():g} (max |ref| {top[r].item():.9g})"
        excused.append(r)
    return err[live].max().item(), (err / bound[:, None])[live].max().item(), excused


# ---- A. the builder, every field ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["wikimel", "wikidiverse"], ids=["tokens", "pooled"])
@pytest.mark.parametrize("D,R,precision", BUILDER_CASES, ids=[f"{d}x{r}-{p}" for d, r, p in BUILDER_CASES])
def test_builder_every_field_against_fp64(D, R, precision, layout):
    """37 entities, 3 mentions x 6 candidates; Ke in {1, 3}, dynamic and static edges, both row formats where the widths allow the
    mixed one.  Token-level tables carry 0, 1, 2, 3, 6, 7 and 10 tokens in rows 0 .. 6 (T = 10): the Python-slice corners of the
    token mean (1 and 2 tokens: an empty slice, NaN; 0 tokens: tokens 1 .. T - 2) and both the unrolled and the tail loop.

    What this test found: with the `f32` builder adding the K products of an output in ONE k-ordered fp32 chain, a few elements of
    h_t / h_i / fv_i at (512, 1024), (768, 2048) and (760, 2040) were up to 6.7 x the reference's own distance from fp64 (2.80e-6
    against a slack of 2.08e-6) where the margin is 5; a k-ordered chain restated on the host has the same 2.4e-6, torch's blocked
    matmul 5.7e-7.  The builder now adds K in slices of 512 under DRIN_PREC_F32 (`cache_gemm_nt`, csrc/entity_cache.hip): at
    most 0.79 of the slack at every width (profiles/cache_rows_parity.txt)."""
    misses = []
    for Ke, edges in ((1, "dynamic"), (3, "dynamic"), (1, "static"), (3, "static")):
        cfg = DrinConfig(dataset_name=layout, num_candidates_data=5, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R,
                         resnet_num_region=3, max_mention_sentence_len=9, max_entity_attr_token_len=TOKENS, object_topk_entity=Ke,
                         gcn_edge_type=edges)
        cfg.validate()
        sd = synth.make_state_dict(cfg, 7)
        tables, men, cand = _planted_tables(cfg, SEED)
        f64 = CR.fields64(cfg, sd, *tables)
        slack, f32 = _slacks(cfg, sd, tables, f64, precision)
        if layout == "wikimel":                            # the planted token counts give the NaN rows the slice rule says
            assert torch.isnan(f64["h_t"]).all(-1).nonzero().flatten().tolist() == [1, 2]
        for k in CR.F16_FIELDS:                             # the seed: the restatement alone never sits astride a power of two
            fin = ~torch.isnan(f64[k]).any(-1)
            assert torch.equal(CR.field_scale(f32[k].double().abs().amax(-1))[fin], CR.field_scale(f64[k].abs().amax(-1))[fin]), k
        table, ib = _on_device(tables, men, cand)
        model = _model(cfg, sd, precision)
        dyn = edges == "dynamic"
        decoded = {}
        formats = ("f32", "mixed_f16") if D % 8 == 0 and R % 8 == 0 else ("f32",)
        for fmt in formats:
            _assert_bands(cfg, D, R, fmt)
            label = f"{D}x{R} {layout} Ke={Ke} {edges} {precision} {fmt}"
            with torch.no_grad():
                table.enable_cache(True, format=fmt, force=True)
                model(ib)
            assert table.cache_format_used == fmt and table._cache.numel() == E_ROWS * CR.row_floats(D, R, fmt) * 4
            dec = decoded[fmt] = CR.decode(table._cache.cpu(), cfg, fmt)
            line, excused = [], []
            for k in ("h_t", "h_i", "chat", "sg"):
                line.append((k,) + _check_f32_field(k, dec[k], f64[k], slack[k], label, misses))
            for k in CR.F16_FIELDS:
                if k != "ohat" and not dyn:
                    continue                                # static edges: no edge-update rows (asserted below / in test C)
                if fmt == "f32":
                    line.append((k,) + _check_f32_field(k, dec[k], f64[k], slack[k], label, misses))
                else:
                    a, b, ex = _check_f16_field(k, dec["units"][k], dec["tail"][:, CR.TAIL_SLOT[k]], f64[k], slack[k], label, misses)
                    line.append((k, a, b))
                    excused += [(k, r) for r in ex]
            assert len(excused) <= 1, f"{label}: rows {excused} have a max within slack of a power of two - more than one of {E_ROWS}"
            print(f"cache rows {label}: " + ", ".join(f"{k} {a:.1e} ({b:.2f} of its bound)" for k, a, b in line) +
                  (f"; scale excused for {excused}" if excused else ""))
            # planted rows
            assert (dec["h_i"][ROW_ZERO_IMAGE] == 0).all()
            assert dec["sg"][ROW_ZERO_SCORES].item() == 0.0
            assert (dec["ohat"][ROW_ZERO_OBJECT] == 0).all() and (dec["ohat"][ROW_ZERO_SCORES] == 0).all()
            if fmt == "f32":
                assert (dec["tail"][:, 1:] == 0).all()     # the 3 pad floats are written (as zeros)
            else:
                s_o = dec["tail"][:, 3]
                assert s_o[ROW_ZERO_OBJECT].item() == 1.0 and (dec["units"]["ohat"][ROW_ZERO_OBJECT] == 0).all()
                if Ke == 1:
                    one, three = dec["units"]["ohat"][ROW_ONE_HOT].view(torch.int16), dec["units"]["ohat"][ROW_ONE_HOT_X3]
                    assert s_o[ROW_ONE_HOT].item() == 1.0 and one[5].item() == 0x3C00 and int((one != 0).sum()) == 1
                    assert s_o[ROW_ONE_HOT_X3].item() == 4.0 and three[R - 3].item() == 0.75 and int((three != 0).sum()) == 1
                if not dyn:                                 # static edges: zero units, unit scales
                    assert (dec["units"]["fv_t"] == 0).all() and (dec["units"]["fv_i"] == 0).all()
                    assert (dec["tail"][:, 1:3] == 1).all()
        if len(decoded) == 2:                               # what both formats keep as fp32 has the same bits in both
            a, b = decoded["f32"], decoded["mixed_f16"]
            for k in ("h_t", "h_i", "chat", "sg"):
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{D}x{R} {layout} Ke={Ke} {edges} {precision}: {k} differs between the formats"
        table.enable_cache(False)
    assert not misses, f"{len(misses)} field(s) past their slack:\n" + "\n".join(misses)


# ---- B. the consumer, one field at a time at raised sensitivity -----------------------------------------------------------------
CONSUMER_CASES = [(64, 128, "f32"), (64, 128, "bf16x3_all"), (264, 520, "f32"), (768, 2048, "f32"), (768, 2048, "bf16x3_all")]


@pytest.mark.parametrize("fmt", CR.FORMATS)
@pytest.mark.parametrize("D,R,precision", CONSUMER_CASES, ids=[f"{d}x{r}-{p}" for d, r, p in CONSUMER_CASES])
def test_consumer_reads_each_f16_field_where_and_how_it_is_stored(D, R, precision, fmt):
    """One of fv_t, fv_i, o^ of the BUILT cache times an exact 2^k (tests/test_cache_rows_host.py: the factor at which a
    4-column defect in that field moves the scores by >= 4 x the bar, while the reference's own spread stays below a quarter of
    it); the scores against the fp64 emulation whose same field is stored alike and multiplied alike - at the bar the cached
    path's scores already have against the oracle.  The cache is the one the first call built, and scaling back restores its bits."""
    cfg = consumer_config(D, R)
    sd = synth.make_state_dict(cfg, 7)
    tables, men, cand = table_case(cfg, E_ROWS, 4, SEED)
    table, ib = _on_device(tables, men, cand)
    model = _model(cfg, sd, precision)
    bar = score_bar(D)
    gathered = [t.cpu() for t in ib.gathered()]
    q = CR.scaled_f16 if fmt == "mixed_f16" else (lambda x: x)
    with torch.no_grad():
        table.enable_cache(True, format=fmt, force=True)
        first = model(ib)
        cache, key = table._cache, table._cache_key
        ptr, before = cache.data_ptr(), cache.clone()
        plain = (first.cpu() - PE.scores_with_rounded_cache_fields(sd, gathered, CR.F16_FIELDS if fmt == "mixed_f16" else (), rnd=q)).abs().max().item()
        assert plain <= bar, plain
        line = [f"as built {plain:.1e}"]
        for field, k in EXPONENTS.items():
            CR.scale_field_in_place(cache, cfg, fmt, field, k)
            got = model(ib)
            assert table._cache is cache and cache.data_ptr() == ptr and table._cache_key == key, "the cache was rebuilt"
            ref = PE.scores_with_rounded_cache_fields(sd, gathered, (field,), rnd=lambda x: q(x) * 2.0 ** k)
            err = (got.cpu() - ref).abs().max().item()
            moved = (got - first).abs().max().item()
            line.append(f"{field} x 2^{k} {err:.1e} (scores moved {moved:.1e})")
            assert torch.isfinite(got).all() and moved > 4 * bar, (field, moved)     # the factor reached the scores
            assert err <= bar, f"{D}x{R} {precision} {fmt}: {field} x 2^{k}: {err:.2e} > {bar:g}"
            CR.scale_field_in_place(cache, cfg, fmt, field, -k)
            assert torch.equal(cache, before)
            assert torch.equal(model(ib), first), f"{field}: scaling back by 2^-{k} did not restore the scores' bits"
    print(f"cached pairs {D}x{R} {precision} {fmt} N={cfg.num_candidates_model}: max |score - emulation| " + ", ".join(line) + f" (bar {bar:g})")
    table.enable_cache(False)


# ---- C. fields nobody may read ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,R", [(64, 128), (264, 520), (768, 2048)], ids=["64x128", "264x520", "768x2048"])
def test_fields_nobody_may_read_are_not_read(D, R):
    """Static edges: the builder leaves fv_t / fv_i of the fp32 rows unwritten and packs zero units under unit scales into the
    mixed ones; `k_cached_pairs` must read neither.  The 3 floats after sg in the fp32 row are padding.  Each is filled with
    NaN in place: the scores keep the bits of the call before."""
    nan = float("nan")
    for edges in ("static", "dynamic"):
        cfg = consumer_config(D, R, gcn_edge_type=edges)
        sd = synth.make_state_dict(cfg, 7)
        table, ib = _on_device(*table_case(cfg, E_ROWS, 4, SEED))
        model = _model(cfg, sd, "f32")
        with torch.no_grad():
            for fmt in CR.FORMATS:
                table.enable_cache(True, format=fmt, force=True)
                first = model(ib)
                assert torch.isfinite(first).all()
                cache = table._cache
                if fmt == "f32":
                    CR.field_view(cache, cfg, fmt, "tail")[:, 1:] = nan
                    if edges == "static":
                        CR.field_view(cache, cfg, fmt, "fv_t").fill_(nan)
                        CR.field_view(cache, cfg, fmt, "fv_i").fill_(nan)
                elif edges == "static":
                    CR.field_view(cache, cfg, fmt, "fv").view(torch.int32).fill_(0x7E007E00)      # fp16 NaN, twice
                    CR.field_view(cache, cfg, fmt, "tail")[:, 1:3] = nan
                else:
                    continue                                                                      # mixed rows, dynamic edges: every byte is read
                torch.cuda.synchronize()
                assert table._cache is cache and torch.isnan(CR.field_view(cache, cfg, fmt, "tail")).any()
                assert torch.equal(model(ib), first), f"{D}x{R} {edges} {fmt}: a field nobody may read reached the scores"
        table.enable_cache(False)


# ---- D. the second slab --------------------------------------------------------------------------------------------------------------
def test_second_builder_slab_reuses_its_scratch_correctly():
    """E = 262 144 + 5 (one full builder slab plus a tail), pooled text, widths 64 / 128, Ke = 1, both formats: the pooled-text
    scratch and the fp32 scratch of the two fp16 products are reused from the first slab to the second.  Rows 0, 262 143 (the
    first slab's ends), all five rows of the second slab and 8 seeded rows against fp64 as in A; over ALL rows, on the device:
    |c^| = 1 to 1e-6 and the sg slot equal to the object score (Ke = 1: one term, exact)."""
    slab = 262144
    E = slab + 5
    D, R = 64, 128
    cfg = DrinConfig(num_candidates_data=5, bert_embed_dim=D, gcn_embed_dim=D, resnet_embed_dim=R, resnet_num_region=3,
                     max_mention_sentence_len=9, object_topk_entity=1)
    sd = synth.make_state_dict(cfg, 7)
    g = torch.Generator(device=DEV).manual_seed(3)
    tables = (torch.randn(E, D, device=DEV, generator=g), None, torch.randn(E, R, device=DEV, generator=g),
              torch.randn(E, 1, R, device=DEV, generator=g), torch.rand(E, 1, device=DEV, generator=g))
    table = EntityTable(*tables)
    men = synth.make_batch(cfg, MENTIONS, 5)
    pick = torch.Generator().manual_seed(4)
    rows = torch.cat([torch.tensor([0, slab - 1, slab, slab + 1, slab + 2, slab + 3, E - 1]), torch.randint(1, slab - 1, (8,), generator=pick)])
    cand = rows[torch.randint(0, rows.numel(), (MENTIONS, cfg.num_candidates_model), generator=pick)]
    cand[0, :3] = torch.tensor([slab - 1, slab, E - 1])
    ib = IndexedBatch([t.to(DEV) for t in men[:7]], table, cand.to(DEV), men[12].to(DEV), men[13].to(DEV))
    host = tuple(None if t is None else t[rows.to(DEV)].cpu() for t in tables)
    f64 = CR.fields64(cfg, sd, *host)
    slack, _ = _slacks(cfg, sd, host, f64, "f32")
    model = _model(cfg, sd, "f32")
    ref = PE.scores_with_rounded_cache_fields(sd, [t.cpu() for t in ib.gathered()])
    for fmt in CR.FORMATS:
        _assert_bands(cfg, D, R, fmt)
        label = f"E={E} {fmt}"
        with torch.no_grad():
            table.enable_cache(True, format=fmt, force=True)
            scores = model(ib)
        cache = table._cache
        assert cache.numel() == E * CR.row_floats(D, R, fmt) * 4
        assert (scores.cpu() - ref).abs().max().item() <= score_bar(D)
        dec = CR.decode(cache.view(torch.float32).view(E, -1)[rows.to(DEV)].cpu(), cfg, fmt)
        line, misses = [], []
        for k in ("h_t", "h_i", "chat", "sg"):
            line.append((k,) + _check_f32_field(k, dec[k], f64[k], slack[k], label, misses))
        excused = []
        for k in CR.F16_FIELDS:
            if fmt == "f32":
                line.append((k,) + _check_f32_field(k, dec[k], f64[k], slack[k], label, misses))
            else:
                a, b, ex = _check_f16_field(k, dec["units"][k], dec["tail"][:, CR.TAIL_SLOT[k]], f64[k], slack[k], label, misses)
                line.append((k, a, b))
                excused += ex
        assert not misses, "\n".join(misses)
        assert len(excused) <= 1, excused
        # every row of both slabs was written
        norm = CR.field_view(cache, cfg, fmt, "chat").double().norm(dim=1)
        worst = (norm - 1).abs().max().item()
        assert worst <= 1e-6, f"{label}: |c^| is off 1 by {worst:.2e} in row {int((norm - 1).abs().argmax())}"
        tail = CR.field_view(cache, cfg, fmt, "tail")
        assert torch.equal(tail[:, 0], tables[4][:, 0]), f"{label}: the sg slot differs from the object score"
        if fmt == "mixed_f16":
            assert _is_pow2_in_range(tail[:, 1:]).all()
            for k, halves in (("ohat", R), ("fv", 2 * D)):
                u = CR.field_view(cache, cfg, fmt, k).contiguous().view(torch.float16).view(E, halves)
                parts = {"ohat": u} if k == "ohat" else {"fv_t": u.view(E, D // 4, 2, 4)[:, :, 0], "fv_i": u.view(E, D // 4, 2, 4)[:, :, 1]}
                for name, units in parts.items():
                    umax = units.reshape(E, -1).abs().amax(1).float()
                    assert ((umax >= 0.5) & (umax <= 1.0)).all(), f"{label}: {name} largest |unit| outside [0.5, 1] in row {int(((umax < 0.5) | (umax > 1)).nonzero()[0])}"
        print(f"cache rows {label} ({rows.numel()} rows of {E}): " + ", ".join(f"{k} {a:.1e} ({b:.2f} of its bound)" for k, a, b in line) +
              f"; all rows: max | |c^| - 1 | {worst:.1e}, sg slot exact")
        table.enable_cache(False)
        del cache
