"""GHMFC training without a GPU: TrainableModel's parameters against ghmfc.Model's under one seed, the shim, the module's
state dict with a dropout stream, the host-side validation of every row-op and dropout entry point, the scratch-size
queries, the dropout mask function (drin_attention_dropout_keep) and the restatement's own sanity check (the gather form
equals the max form at the fp64 argmax)."""
import ctypes as C
import math
import sys
import types

import pytest
import torch
from torch import nn

from drin_amd import _lib, ghmfc
from drin_amd.attention import DropoutStream, MultiheadAttention, dropout_keep
from drin_amd.ghmfc_train import TrainableModel
from tests.ghmfc_inputs import CASES, KEYS, ghmfc_inputs, geometry
from tests.ghmfc_restatement import ghmfc_scores
from tests.ghmfc_train_restatement import ghmfc_train_scores
from tests.test_ghmfc_host import as_tensors, case_model, cfg_for

ONE = C.c_void_p(16)    # 16-byte aligned, never dereferenced: every check below fails before a launch
ODD = C.c_void_p(20)


def test_trainable_model_draws_the_same_weights_and_loads_checkpoints():
    name = "wd_b1"
    ref = case_model(name)
    torch.manual_seed(CASES[name]["seed"])
    got = TrainableModel(cfg_for(name))
    a, b = ref.state_dict(), got.state_dict()
    assert list(a) == list(b) == KEYS and len(b) == 52
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert [id(p) for p in got.param_list()] == [id(p) for _n, p in got.named_parameters()]
    torch.manual_seed(99)
    other = TrainableModel(cfg_for(name), precision="f32", dropout=0.25, seed=7)
    other.load_state_dict(a)                                          # a ghmfc.Model checkpoint loads
    assert all(torch.equal(a[k], v) for k, v in other.state_dict().items())
    f = other.mention_encoder.intermediate_layer
    attentions = [f.t2v_attention.a2b_attention, f.t2v_attention.b2a_attention, f.v2t_attention.a2b_attention, f.v2t_attention.b2a_attention]
    assert all(isinstance(m, MultiheadAttention) and m.dropout == 0.25 and m.precision == "f32" for m in attentions)
    assert all(m.dropout_stream is other.dropout_stream for m in attentions) and other.dropout_stream.seed == 7
    with pytest.raises(ValueError, match="dropout"):
        TrainableModel(cfg_for(name), dropout=1.0)
    with pytest.raises(RuntimeError, match="GPU only"):               # CPU tensors are refused in both modes
        other.train()(as_tensors(ghmfc_inputs(name), torch.float32))
    with pytest.raises(RuntimeError, match="GPU only"):
        other.eval()(as_tensors(ghmfc_inputs(name), torch.float32))


def test_shim_model_reads_transformer_dropout(monkeypatch):
    args = types.ModuleType("common.args")
    for k, v in dict(dataset_name="wikidiverse", num_candidates_model=4, bert_embed_dim=16, resnet_embed_dim=32,
                     max_mention_sentence_len=12, resnet_num_region=3, transformer_num_heads=2, transformer_dropout=0.3, seed=5).items():
        setattr(args, k, v)
    common = types.ModuleType("common")
    common.args = args
    monkeypatch.setitem(sys.modules, "common", common)
    monkeypatch.setitem(sys.modules, "common.args", args)
    from drin_amd import ghmfc_shim
    m = ghmfc_shim.Model()
    assert isinstance(m, TrainableModel) and m.dropout == 0.3 and m.dropout_stream.seed == 5
    assert m.cfg.embed_dim == 16 and len(m.state_dict()) == 52


def test_attention_with_a_dropout_stream_keeps_torchs_state_dict():
    torch.manual_seed(3)
    ref = nn.MultiheadAttention(24, 4, dropout=0.1, batch_first=True)
    torch.manual_seed(3)
    stream = DropoutStream(seed=11)
    got = MultiheadAttention(24, 4, dropout=0.1, batch_first=True, dropout_stream=stream)
    a, b = ref.state_dict(), got.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[n], b[n]) for n in a)
    assert got.dropout_stream is stream and MultiheadAttention(24, 4, dropout=0.1, batch_first=True).dropout_stream is None
    assert [stream.draw(2, 4, 5, 7), stream.draw(2, 4, 7, 7)] == [0, 1] and stream.log == [(0, 2, 4, 5, 7), (1, 2, 4, 7, 7)]
    x = torch.zeros(2, 3, 24)
    with pytest.raises(RuntimeError, match="GPU only"):               # the dropout refusal is lifted: next is the device
        got.train()(x, x, x)


def test_row_op_entry_points_validate_on_host():
    lib = _lib.load()

    def ln_fwd(x=ONE, mean=ONE, E=16, rows=3):
        return lib.drin_layernorm_res_train_fwd(x, None, ONE, ONE, ONE, mean, ONE, rows, E, 1e-5, None)

    def ln_bwd(x=ONE, dy=ONE, dgamma=ONE, scratch=ONE, floats=1 << 20, E=16, rows=3):
        return lib.drin_layernorm_res_bwd(x, None, ONE, ONE, ONE, dy, ONE, dgamma, ONE, scratch, floats, rows, E, None)

    def max_fwd(x=ONE, idx=ONE, E=16, B=2, S=3):
        return lib.drin_seq_max_train_fwd(x, ONE, idx, B, S, E, None)

    def max_bwd(x=ONE, idx=ONE, E=16, B=2, S=3):
        return lib.drin_seq_max_bwd(x, idx, ONE, B, S, E, None)

    def gate_fwd(x=ONE, E=16, B=2):
        return lib.drin_gate_mix_fwd(x, ONE, ONE, ONE, ONE, B, E, None)

    def gate_bwd(x=ONE, dws=ONE, scratch=ONE, floats=1 << 20, E=16, B=2):
        return lib.drin_gate_mix_bwd(x, ONE, ONE, ONE, ONE, ONE, ONE, dws, ONE, scratch, floats, B, E, None)

    def cos_fwd(x=ONE, E=16, B=2):
        return lib.drin_cosine_rows_fwd(x, ONE, ONE, B, 3, E, 1e-8, None)

    def cos_bwd(x=ONE, scratch=ONE, floats=1 << 20, E=16, B=2):
        return lib.drin_cosine_rows_bwd(x, ONE, ONE, ONE, ONE, scratch, floats, B, 3, E, 1e-8, None)

    def mean(x=ONE, E=16, B=2):
        return lib.drin_entity_token_mean(x, ONE, ONE, B, 6, E, None)

    everyone = (ln_fwd, ln_bwd, max_fwd, max_bwd, gate_fwd, gate_bwd, cos_fwd, cos_bwd, mean)
    for call in everyone:
        assert call(x=None) == _lib.E_NULL, call.__name__
        assert b"NULL" in lib.drin_last_error()
        assert call(x=ODD) == _lib.E_ALIGN, call.__name__
        assert call(E=6) == _lib.E_SHAPE, call.__name__
        assert b"multiple of 4" in lib.drin_last_error()
        assert call(E=0) == _lib.E_SHAPE, call.__name__
    for call in (ln_fwd, ln_bwd, gate_bwd):                           # a row lives in registers: widths up to 2048
        assert call(E=2052) == _lib.E_SHAPE and b"2048" in lib.drin_last_error(), call.__name__
    assert cos_bwd(E=2052) == _lib.E_UNSUPPORTED and b"1024" in lib.drin_last_error()
    for call in (ln_fwd, ln_bwd):
        assert call(rows=0) == _lib.E_SHAPE
    for call in (max_fwd, max_bwd, gate_fwd, gate_bwd, cos_fwd, cos_bwd, mean):
        assert call(B=0) == _lib.E_SHAPE, call.__name__
    assert max_fwd(B=65536) == _lib.E_SHAPE and max_fwd(S=0) == _lib.E_SHAPE and max_bwd(S=0) == _lib.E_SHAPE
    assert ln_fwd(mean=None) == _lib.E_NULL and max_fwd(idx=None) == _lib.E_NULL and max_bwd(idx=None) == _lib.E_NULL
    assert ln_bwd(dy=None) == _lib.E_NULL
    # the column sums need their scratch; a frozen LayerNorm / score Linear needs none
    assert ln_bwd(scratch=None) == _lib.E_NULL and ln_bwd(floats=3) == _lib.E_WORKSPACE
    assert gate_bwd(scratch=None) == _lib.E_NULL and gate_bwd(floats=3) == _lib.E_WORKSPACE
    assert cos_bwd(scratch=None) == _lib.E_NULL and cos_bwd(floats=17) == _lib.E_WORKSPACE
    assert lib.drin_version() == _lib.ABI_VERSION == 12               # additive under ABI 12


def test_dropout_entry_points_validate_on_host():
    lib = _lib.load()

    def fwd(q=ONE, lse=ONE, Lk=8, dh=16, ldq=64, p=0.1):
        return lib.drin_attention_dropout_fwd(q, ldq, ONE, 64, ONE, 64, None, ONE, 64, lse, 2, 4, 7, Lk, dh, p, 1, 2, None)

    def bwd(q=ONE, lse=ONE, Lk=8, dh=16, ldq=64, p=0.1, dv=ONE):
        return lib.drin_attention_dropout_bwd(q, ldq, ONE, 64, ONE, 64, None, ONE, 64, lse, ONE, 64, ONE, 64, ONE, 64, dv, 64, ONE,
                                              2, 4, 7, Lk, dh, p, 1, 2, None)

    for call in (fwd, bwd):
        for p in (1.0, -0.1, 1.5, float("nan")):
            assert call(p=p) == _lib.E_SHAPE and b"[0, 1)" in lib.drin_last_error(), (call.__name__, p)
        for p in (0.0, 0.1):                                          # the undropped path of p = 0 validates the same way
            assert call(q=None, p=p) == _lib.E_NULL and call(lse=None, p=p) == _lib.E_NULL
            assert call(Lk=513, p=p) == _lib.E_SHAPE and b"k_len" in lib.drin_last_error()
            assert call(dh=257, p=p) == _lib.E_SHAPE
            assert call(ldq=63, p=p) == _lib.E_SHAPE and b"ldq" in lib.drin_last_error()
    assert bwd(dv=None) == _lib.E_NULL and b"dk and dv" in lib.drin_last_error()
    buf = (C.c_uint8 * 16)()
    keep = lambda p=0.1, B=1, out=buf: lib.drin_attention_dropout_keep(1, 2, B, 2, 2, 4, p, out)   # noqa: E731
    assert keep() == _lib.OK
    assert keep(p=1.0) == _lib.E_SHAPE and keep(B=0) == _lib.E_SHAPE and keep(out=None) == _lib.E_NULL


def test_scratch_queries_are_positive_and_monotone():
    lib = _lib.load()
    for query in (lib.drin_layernorm_res_bwd_scratch_floats, lib.drin_gate_mix_bwd_scratch_floats):
        for E in (16, 260, 768, 2048):
            sizes = [query(rows, E) for rows in (1, 2, 5, 64, 1000, 1024, 1025, 100000)]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (E, sizes)
            assert query(1, E) >= 2 * E                               # one row of partial sums at least
        assert query(0, 16) == 0 and query(4, 6) == 0 and query(4, 2052) == 0


def test_dropout_mask_function():
    B, H, Lq, Lk = 4, 8, 128, 256                                     # 2^20 elements
    n = B * H * Lq * Lk
    assert n == 1 << 20
    base = dropout_keep(5, 9, B, H, Lq, Lk, 0.1)
    assert base.dtype == torch.bool and tuple(base.shape) == (B, H, Lq, Lk)
    assert torch.equal(base, dropout_keep(5, 9, B, H, Lq, Lk, 0.1))                # a pure function of (seed, call, index)
    for other in (dropout_keep(6, 9, B, H, Lq, Lk, 0.1), dropout_keep(5, 10, B, H, Lq, Lk, 0.1), dropout_keep(5 + (1 << 32), 9, B, H, Lq, Lk, 0.1),
                  dropout_keep(5, 9 + (1 << 32), B, H, Lq, Lk, 0.1)):
        assert 0.1 < (other != base).double().mean().item() < 0.26                 # independent masks differ at 2 p (1 - p) = 0.18
    for p, bound in ((0.1, 1.5e-3), (0.5, 2.4e-3)):
        share = dropout_keep(5, 9, B, H, Lq, Lk, p).double().mean().item()
        print(f"p = {p}: kept share {share:.6f}")
        assert abs(share - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n) <= 1.02 * bound   # (the issue's rounded figures)
    assert dropout_keep(5, 9, B, H, Lq, Lk, 0.0).all()
    # the flat index alone decides: another shape with the same element count gives the same bytes; a lower rate keeps a superset
    assert torch.equal(base.flatten(), dropout_keep(5, 9, 1, 1, 1024, 1024, 0.1).flatten())
    assert (dropout_keep(5, 9, B, H, Lq, Lk, 0.05) | ~base).all()


@pytest.mark.parametrize("name", ["wd_b1", "wd_b5", "heads_5_9"])
def test_gather_form_equals_max_form_at_the_fp64_argmax(name):
    sd = {k: v.double() for k, v in case_model(name).state_dict().items()}
    batch = as_tensors(ghmfc_inputs(name), torch.float64)
    H = geometry(name)["H"]
    with torch.no_grad():
        want = ghmfc_scores(batch, sd, H)
        plain, pre_t, pre_v = ghmfc_train_scores(batch, sd, H, return_pre_max=True)
        gathered = ghmfc_train_scores(batch, sd, H, idx_text=pre_t.argmax(1), idx_image=pre_v.argmax(1))
    assert torch.equal(plain, want) and torch.equal(gathered, want)
    # all-ones keep masks at p = 0 change nothing either
    B, L, P = batch[0].shape[0], batch[0].shape[1], batch[4].shape[1]
    ones = [torch.ones(B, H, a, b, dtype=torch.bool) for a, b in ((L, P), (L, L), (P, L), (P, P))]
    with torch.no_grad():
        assert torch.equal(ghmfc_train_scores(batch, sd, H, keeps=ones, p=0.0), want)


def test_new_wikimel_case_has_no_nan_row():
    from tests.ghmfc_train_inputs import wikimel_no_nan_batch, WM_CASE
    batch = as_tensors(wikimel_no_nan_batch(), torch.float64)
    assert batch[5].dim() == 4 and batch[5].shape[2] == 6 and int(batch[6].sum(-1).min()) >= 3
    torch.manual_seed(WM_CASE["seed"])
    model = ghmfc.Model(ghmfc.GhmfcConfig(dataset_name="wikimel", num_candidates=4, embed_dim=16, image_dim=32, mention_tokens=12,
                                          image_regions=3, num_heads=2, entity_tokens=6))
    sd = {k: v.double() for k, v in model.state_dict().items()}
    with torch.no_grad():
        assert torch.isfinite(ghmfc_scores(batch, sd, 2)).all()
