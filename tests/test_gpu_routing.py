"""-m gpu: which library path `Model.forward` takes for a batch, observed from outside.  For the duration of a case the
scoring entry points on the `CDLL` object of `_lib.load()` are replaced by recorders that note their name and the routing
fields of their config / batch arguments and call through; every case states the exact sequence as a literal and checks
the scores against a `Model(fused=False)` on the gathered tensors (bit for bit where both run the layer-by-layer entry
point on the same values, else inside the bars of the suite: 1e-4 split-bf16, 1e-5 exact fp32).

A record reads `<entry point> p<precision> f<feature_dtype> E<num_entities> T<entity_tokens> c<cache_format> B<batch>`,
then `idx` / `cls` when `drin_batch.entity_index` / `.entity_text_cls` are set, then for `drin_forward_staged`
`keep<keep_for_backward>` and `event` when a parameters-ready event was handed over."""
import contextlib
import functools

import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig, wikimel_config
from drin_amd.model import EntityTable, IndexedBatch, Model
from oracle.cases import TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENTRY_POINTS = ("drin_forward_staged", "drin_forward_prepared", "drin_forward_cached", "drin_build_entity_cache", "drin_prepare",
                "drin_backward_ex", "drin_pool_fwd", "drin_pool_bwd")
_BATCH_SECOND = ("drin_forward_staged", "drin_forward_prepared", "drin_forward_cached", "drin_build_entity_cache",
                 "drin_backward_ex", "drin_pool_fwd")
FEATURE_SLOTS = (0, 4, 5, 7, 9, 10)
TOL = {"f32": 1e-5, "bf16x3": 1e-4, "bf16x3_if16": 1e-4}

WD = DrinConfig(**TINY)                                                                     # N = 11, pooled entity text
WM = DrinConfig(dataset_name="wikimel", num_candidates_data=12, max_entity_attr_token_len=6, **TINY)   # N = 13, T = 6
# the smallest geometry the table form of the layer-by-layer entry points takes: D = R = 128, and 1024 pairs at B = 11
WIDE = DrinConfig(dataset_name="wikimel", num_candidates_data=100, max_entity_attr_token_len=8, bert_embed_dim=128,
                  gcn_embed_dim=128, resnet_embed_dim=128, max_mention_sentence_len=12, resnet_num_region=5)


@contextlib.contextmanager
def recorded():
    """The list the recorders append to, while the entry points of `ENTRY_POINTS` are replaced on the loaded library."""
    lib, log = _lib.load(), []
    originals = {name: getattr(lib, name) for name in ENTRY_POINTS}

    def recorder(name, fn):
        def call(*args):
            c = args[0]._obj
            line = f"{name[5:]} p{c.precision} f{c.feature_dtype} E{c.num_entities} T{c.entity_tokens} c{c.cache_format} B{c.batch}"
            if name in _BATCH_SECOND:
                b = args[1]._obj
                line += (" idx" if b.entity_index else "") + (" cls" if b.entity_text_cls else "")
            if name == "drin_forward_staged":
                line += f" keep{args[6]}" + (" event" if args[8] is not None else "")
            log.append(line)
            return fn(*args)
        return call

    for name, fn in originals.items():
        setattr(lib, name, recorder(name, fn))
    try:
        yield log
    finally:
        for name, fn in originals.items():
            setattr(lib, name, fn)


@functools.lru_cache(maxsize=None)
def _weights(cfg):
    return synth.make_state_dict(cfg, 8)


def _model(cfg, precision="bf16x3", fused=True, frozen=False, sd=None):
    m = Model(cfg, precision=precision, fused=fused).to(DEV)
    m.load_state_dict(sd or _weights(cfg))
    return m.requires_grad_(not frozen)


def _seq(cfg, B, seed=3):
    return [t.to(DEV) for t in synth.make_batch(cfg, B, seed)[:14]]


def _bf16(seq, slots=FEATURE_SLOTS):
    return [t.to(torch.bfloat16) if i in slots else t for i, t in enumerate(seq)]


def _table_batch(cfg, B, E=30, seed=5, objects=1):
    cfg_t = cfg.with_(num_candidates_data=E - 1, object_topk_entity=objects)
    tab = synth.make_batch(cfg_t, 1, seed)
    table = EntityTable(tab[7][0], tab[8][0], tab[9][0], tab[10][0], tab[11][0]).to(DEV)
    men = _seq(cfg, B, seed + 1)
    cand = torch.randint(0, E, (B, cfg.num_candidates_model), generator=torch.Generator().manual_seed(1)).to(DEV)
    return table, IndexedBatch(men[:7], table, cand, men[12], men[13])


def _bf16_table(table):
    return EntityTable(table.text.bfloat16(), table.mask, table.image.bfloat16(), table.object.bfloat16(), table.object_score)


def _with_table(ib, table):
    return IndexedBatch(ib.mention, table, ib.candidates, ib.miet_similarity, ib.mtei_similarity)


def _check(scores, cfg, seq, precision="bf16x3", equal=False, train=False, sd=None):
    """`scores` against `Model(fused=False)` on `seq` (under the same grad mode when `train`)."""
    ref_model = _model(cfg, "bf16x3" if precision == "bf16x3_if16" else precision, fused=False, sd=sd)
    seq = [t.detach() for t in seq]
    with torch.enable_grad() if train else torch.no_grad():
        ref = ref_model(seq).detach()
    worst = (scores.detach() - ref).abs().max().item() if ref.numel() else 0.0
    print(f"max |scores - layer-by-layer reference| = {worst:.3e}")
    assert scores.shape == ref.shape and scores.dtype == torch.float32
    if equal:
        assert torch.equal(scores.detach(), ref)
    else:
        assert worst <= TOL[precision]


@pytest.fixture
def stream_waits(monkeypatch):
    """The events the current stream was made to wait for (`torch.cuda.Stream.wait_event`), recorded and passed through."""
    waits, wait_event = [], torch.cuda.Stream.wait_event
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", lambda self, ev: (waits.append(ev), wait_event(self, ev))[1])
    return waits


def _pending_update(model):
    ev = torch.cuda.Event()
    ev.record()
    model._params_ready = ev
    return ev


# ---- the 14-sequence -------------------------------------------------------------------------------------------------
def test_inference_is_folded():                                                            # 1
    seq, m = _seq(WD, 3), _model(WD)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["prepare p1 f0 E0 T0 c0 B3", "forward_prepared p1 f0 E0 T0 c0 B3"]
    _check(out, WD, seq)


def test_unfused_model_runs_the_layers():                                                  # 2
    seq, m = _seq(WD, 3), _model(WD, fused=False)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep0"]
    _check(out, WD, seq, equal=True)


@pytest.mark.parametrize("kw", [dict(num_gcn_layers=3), dict(gcn_edge_feature="vector")], ids=["three_layers", "vector_edges"])
def test_geometry_off_the_folded_path_runs_the_layers(kw):                                 # 3, 4
    cfg = WD.with_(**kw)
    seq, m = _seq(cfg, 3), _model(cfg)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep0"]
    _check(out, cfg, seq, equal=True)


def test_exact_fp32_inference_is_folded():                                                 # 5
    seq, m = _seq(WD, 3), _model(WD, "f32")
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["prepare p0 f0 E0 T0 c0 B3", "forward_prepared p0 f0 E0 T0 c0 B3"]
    _check(out, WD, seq, "f32")


def test_if16_reaches_the_library_on_the_folded_path_only():                               # 6
    seq, m = _seq(WD, 3), _model(WD, "bf16x3_if16")
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["prepare p5 f0 E0 T0 c0 B3", "forward_prepared p5 f0 E0 T0 c0 B3"]
    _check(out, WD, seq, "bf16x3_if16")
    cfg = WD.with_(num_gcn_layers=3)
    seq, m = _seq(cfg, 3), _model(cfg, "bf16x3_if16")
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep0"]
    _check(out, cfg, seq, "bf16x3_if16", equal=True)


def test_frozen_model_under_grad_mode_is_folded():                                         # 7
    seq, m = _seq(WD, 3), _model(WD, frozen=True)
    with recorded() as log:
        out = m(seq)
    print(log)
    assert log == ["prepare p1 f0 E0 T0 c0 B3", "forward_prepared p1 f0 E0 T0 c0 B3"]
    assert not out.requires_grad
    _check(out, WD, seq)


def test_batch_tensor_requiring_grad_runs_the_layers_for_backward():                       # 8
    seq, m = _seq(WD, 3), _model(WD, frozen=True)
    seq[0].requires_grad_(True)
    with recorded() as log:
        out = m(seq)
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep1"]
    assert out.requires_grad
    _check(out, WD, seq, equal=True, train=True)


def test_training_step_keeps_for_backward():                                               # 9
    seq, m = _seq(WD, 3), _model(WD)
    with recorded() as log:
        out = m(seq)
        out.sum().backward()
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep1", "backward_ex p1 f0 E0 T0 c0 B3"]
    _check(out, WD, seq, equal=True, train=True)


# ---- bf16-stored features --------------------------------------------------------------------------------------------
def test_bf16_features_are_read_in_place_by_the_folded_path():                             # 10
    seq, m = _bf16(_seq(WD, 3)), _model(WD)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["prepare p1 f1 E0 T0 c0 B3", "forward_prepared p1 f1 E0 T0 c0 B3"]
    _check(out, WD, seq)


def test_bf16_features_are_widened_for_exact_fp32():                                       # 11
    seq, m = _bf16(_seq(WD, 3)), _model(WD, "f32")
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log)
    assert log == ["prepare p0 f0 E0 T0 c0 B3", "forward_prepared p0 f0 E0 T0 c0 B3"]
    _check(out, WD, seq, "f32")


def test_bf16_features_are_widened_once_for_the_layers(monkeypatch):                       # 12
    cfg = WD.with_(num_gcn_layers=3)
    seq, m = _bf16(_seq(cfg, 3)), _model(cfg)
    made = []

    class Counted(_lib.DrinConfigC):                       # every `_Call` describes its tensors in one drin_config
        def __init__(self):
            made.append(1)
            super().__init__()

    monkeypatch.setattr(_lib, "DrinConfigC", Counted)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    monkeypatch.undo()
    print(log, len(made))
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep0"]
    assert len(made) == 1
    _check(out, cfg, seq, equal=True)


def test_partly_bf16_features_are_refused():                                               # 13
    seq, m = _bf16(_seq(WD, 3), FEATURE_SLOTS[:5]), _model(WD)
    with recorded() as log, torch.no_grad(), pytest.raises(ValueError, match="all six feature tensors"):
        m(seq)
    assert log == []


@pytest.mark.parametrize("block_grad", [False, True], ids=["block_constant", "block_requires_grad"])
def test_training_pools_a_bf16_token_block_in_place(block_grad):                           # 14
    cfg = wikimel_config(max_entity_attr_token_len=8)
    sd = synth.make_state_dict(cfg, 8)
    seq = _bf16(_seq(cfg, 2))
    seq[7].requires_grad_(block_grad)
    m = _model(cfg, sd=sd)
    with recorded() as log:
        out = m(seq)
        out.sum().backward()
    print(log)
    assert log == ["pool_fwd p0 f1 E0 T8 c0 B202", "forward_staged p1 f0 E0 T0 c0 B2 cls keep1", "backward_ex p1 f0 E0 T0 c0 B2 cls"] \
        + (["pool_bwd p1 f1 E0 T8 c0 B2"] if block_grad else [])
    assert (seq[7].grad is not None and seq[7].grad.dtype == torch.bfloat16) == block_grad
    _check(out, cfg, [t.float() if t.dtype == torch.bfloat16 else t for t in seq], equal=True, train=True, sd=sd)


# ---- table form: inference -------------------------------------------------------------------------------------------
def test_table_inference_is_folded_over_the_index():                                       # 15
    _table, ib = _table_batch(WM, 3)
    m = _model(WM)
    with recorded() as log, torch.no_grad():
        out = m(ib)
    print(log)
    assert log == ["prepare p1 f0 E30 T6 c0 B3", "forward_prepared p1 f0 E30 T6 c0 B3 idx"]
    _check(out, WM, ib.gathered())


def test_table_inference_in_exact_fp32_gathers():                                          # 16
    _table, ib = _table_batch(WM, 3)
    m = _model(WM, "f32")
    with recorded() as log, torch.no_grad():
        out = m(ib)
    print(log)
    assert log == ["prepare p0 f0 E0 T6 c0 B3", "forward_prepared p0 f0 E0 T6 c0 B3"]
    _check(out, WM, ib.gathered(), "f32")


def test_bf16_tables_are_read_in_place_over_the_index():                                   # 17
    table, ib = _table_batch(WM, 3)
    ib = IndexedBatch(_bf16(ib.mention), _bf16_table(table), ib.candidates, ib.miet_similarity, ib.mtei_similarity)
    m = _model(WM)
    with recorded() as log, torch.no_grad():
        out = m(ib)
    print(log)
    assert log == ["prepare p1 f1 E30 T6 c0 B3", "forward_prepared p1 f1 E30 T6 c0 B3 idx"]
    _check(out, WM, ib.gathered())


@pytest.mark.parametrize("precision,p", [("bf16x3", 1), ("f32", 0)])
def test_entity_cache_is_built_once_then_scored_from(precision, p):                        # 18
    table, ib = _table_batch(WM, 3)
    table.enable_cache()
    m = _model(WM, precision)
    with recorded() as log, torch.no_grad():
        first = m(ib)
        mark = len(log)
        second = m(ib)
    print(log)
    assert log[:mark] == [f"prepare p{p} f0 E30 T6 c0 B3", f"build_entity_cache p{p} f0 E30 T6 c0 B3 idx",
                          f"forward_cached p{p} f0 E30 T6 c0 B3 idx"]
    assert log[mark:] == [f"forward_cached p{p} f0 E30 T6 c0 B3 idx"]
    assert torch.equal(first, second)
    _check(first, WM, ib.gathered(), precision)


def test_entity_cache_refuses_a_bf16_table():                                              # 19
    table, ib = _table_batch(WM, 3)
    ib = _with_table(ib, _bf16_table(table).enable_cache())
    with recorded() as log, torch.no_grad(), pytest.raises(ValueError, match="fp32 tables"):
        _model(WM)(ib)
    assert log == []


def test_weight_changed_in_place_rebuilds_folds_and_cache():                               # 20
    table, ib = _table_batch(WM, 3)
    seq = ib.gathered()
    m = _model(WM)
    with torch.no_grad():
        m(seq)
        m(_with_table(ib, table.enable_cache()))
        m.gcn_layers[0].w_h.weight.mul_(0.5)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        with recorded() as log:
            folded = m(seq)
            mark = len(log)
            cached = m(ib)                                # the folds are rebuilt already; the cache is keyed on their generation
    print(log)
    assert log[:mark] == ["prepare p1 f0 E0 T6 c0 B3", "forward_prepared p1 f0 E0 T6 c0 B3"]
    assert log[mark:] == ["build_entity_cache p1 f0 E30 T6 c0 B3 idx", "forward_cached p1 f0 E30 T6 c0 B3 idx"]
    _check(cached, WM, seq, sd=sd)
    _check(folded, WM, seq, sd=sd)


# ---- table form: training --------------------------------------------------------------------------------------------
def _wide(B, **kw):
    return _table_batch(WIDE, B, E=64, **kw)


def test_table_training_reads_pooled_tables_through_the_index_from_1024_pairs():           # 21
    _table, ib = _wide(11)
    m = _model(WIDE)
    with recorded() as log:
        out = m(ib)
        out.sum().backward()
    print(log)
    assert log == ["pool_fwd p0 f0 E0 T8 c0 B64", "forward_staged p1 f0 E64 T0 c0 B11 idx cls keep1", "backward_ex p1 f0 E64 T0 c0 B11 idx cls"]
    _check(out, WIDE, ib.gathered(), equal=True, train=True)
    _table, ib = _wide(10)
    with recorded() as log:
        out = m(ib)
    print(log)
    assert log == ["pool_fwd p0 f0 E0 T8 c0 B64", "forward_staged p1 f0 E0 T0 c0 B10 cls keep1"]
    _check(out, WIDE, ib.gathered(), equal=True, train=True)


def test_table_training_with_two_objects_per_entity_gathers_pooled_rows():                 # 22
    cfg = WIDE.with_(object_topk_entity=2)
    _table, ib = _table_batch(cfg, 11, E=64, objects=2)
    with recorded() as log:
        out = _model(cfg)(ib)
    print(log)
    assert log == ["pool_fwd p0 f0 E0 T8 c0 B64", "forward_staged p1 f0 E0 T0 c0 B11 cls keep1"]
    _check(out, cfg, ib.gathered(), equal=True, train=True)


def test_table_training_on_a_pooled_table_gathers():                                       # 23
    table, ib = _wide(11)
    ib = _with_table(ib, EntityTable(table.text.mean(1), None, table.image, table.object, table.object_score))
    with recorded() as log:
        out = _model(WIDE)(ib)
    print(log)
    assert log == ["forward_staged p1 f0 E0 T0 c0 B11 keep1"]
    _check(out, WIDE, ib.gathered(), equal=True, train=True)


def test_table_tensor_requiring_grad_gathers_token_rows():                                 # 24
    table, ib = _wide(11)
    table.image.requires_grad_(True)
    with recorded() as log:
        out = _model(WIDE)(ib)
        out.sum().backward()
    print(log)
    assert log == ["forward_staged p1 f0 E0 T8 c0 B11 keep1", "backward_ex p1 f0 E0 T8 c0 B11"]
    assert table.image.grad is not None and table.image.grad.shape == table.image.shape
    _check(out, WIDE, ib.gathered(), equal=True, train=True)


def test_table_training_on_a_bf16_table_gathers_pooled_rows():                             # 25
    table, ib = _wide(11)
    ib = _with_table(ib, _bf16_table(table))
    with recorded() as log:
        out = _model(WIDE)(ib)
    print(log)
    assert log == ["pool_fwd p0 f1 E0 T8 c0 B64", "forward_staged p1 f0 E0 T0 c0 B11 cls keep1"]
    _check(out, WIDE, [t.float() if t.dtype == torch.bfloat16 else t for t in ib.gathered()], equal=True, train=True)


# ---- slicing, empty batches, the parameters-ready event ---------------------------------------------------------------
def test_batches_above_the_call_limit_take_one_route_per_slice(monkeypatch):               # 26
    monkeypatch.setattr(Model, "MAX_CALL_MENTIONS", 4)
    seq = _seq(WD, 10)
    with recorded() as log, torch.no_grad():
        out = _model(WD)(seq)
    print(log)
    assert log == ["prepare p1 f0 E0 T0 c0 B4", "forward_prepared p1 f0 E0 T0 c0 B4", "forward_prepared p1 f0 E0 T0 c0 B4",
                   "forward_prepared p1 f0 E0 T0 c0 B2"]
    _table, ib = _table_batch(WM, 10)
    with recorded() as log, torch.no_grad():
        out_t = _model(WM)(ib)
    print(log)
    assert log == ["prepare p1 f0 E30 T6 c0 B4", "forward_prepared p1 f0 E30 T6 c0 B4 idx", "forward_prepared p1 f0 E30 T6 c0 B4 idx",
                   "forward_prepared p1 f0 E30 T6 c0 B2 idx"]
    monkeypatch.undo()
    _check(out, WD, seq)
    _check(out_t, WM, ib.gathered())


def test_empty_sequence_batch_calls_nothing():                                             # 27
    seq = [t[:0] for t in _seq(WD, 3)]
    with recorded() as log, torch.no_grad():
        out = _model(WD)(seq)
    assert log == []
    assert out.shape == (0, WD.num_candidates_model) and out.dtype == torch.float32


def test_empty_table_batch_is_a_folded_call_of_batch_zero():                               # 28
    table, ib = _table_batch(WM, 3)
    empty = IndexedBatch([t[:0] for t in ib.mention], table, ib.candidates[:0], ib.miet_similarity[:0], ib.mtei_similarity[:0])
    # (the library validates the geometry of the empty call, then meets the null pointers of the empty tensors - the index too)
    with recorded() as log, torch.no_grad(), pytest.raises(_lib.DrinError, match="drin_forward_prepared: NULL argument") as err:
        _model(WM)(empty)
    print(log)
    assert log == ["prepare p1 f0 E30 T6 c0 B0", "forward_prepared p1 f0 E30 T6 c0 B0"]
    assert err.value.status == _lib.E_NULL


def test_folded_call_waits_for_a_pending_update(stream_waits):                             # 29
    seq, m = _seq(WD, 3), _model(WD)
    ev = _pending_update(m)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    assert log == ["prepare p1 f0 E0 T0 c0 B3", "forward_prepared p1 f0 E0 T0 c0 B3"]
    assert stream_waits == [ev] and m._params_ready is None
    _check(out, WD, seq)


def test_training_step_hands_a_pending_update_to_the_library(stream_waits):                # 30
    seq, m = _seq(WD, 3), _model(WD)
    _pending_update(m)
    with recorded() as log:
        out = m(seq)
        out.sum().backward()
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep1 event", "backward_ex p1 f0 E0 T0 c0 B3"]
    assert stream_waits == [] and m._params_ready is None
    _check(out, WD, seq, equal=True, train=True)


def test_inference_on_the_layers_with_a_pending_update(stream_waits):                      # 31
    """An inference call that runs the layer-by-layer entry point although the model folds (three layers): what happens to
    the event is the one thing about a route that is not fixed by the results."""
    cfg = WD.with_(num_gcn_layers=3)
    seq, m = _seq(cfg, 3), _model(cfg)
    _pending_update(m)
    with recorded() as log, torch.no_grad():
        out = m(seq)
    print(log, len(stream_waits))
    assert log == ["forward_staged p1 f0 E0 T0 c0 B3 keep0 event"]     # the rule follows the route: "layers" hands the event over
    assert stream_waits == [] and m._params_ready is None
    _check(out, cfg, seq, equal=True)
