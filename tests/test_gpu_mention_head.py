"""-m gpu: the mention head of the layer-by-layer entry points (drin_forward_staged_head / drin_backward_head; DESIGN.md
section 22) on the golden cases' geometries.
  * a NULL head and {LINEAR, AVG_EXTRACT} give the bits of drin_forward_staged / drin_backward_ex: the default path did not move;
  * a ROWS head - either representation, with and without an encoded block - against the fp64 restatement
    (tests/drin_encoder_restatement.py) evaluated at the library's own max positions: scores at 1e-4 (bf16x3) / 1e-5 (f32), the
    layer-0 vertex and the edge row equal to the kernel's own entry point bit for bit, every parameter gradient, the raw block's
    and the encoded block's gradient at 2e-4 of max|ref| (the project's bars, DESIGN.md sections 16-20), the loss being the
    reference's triplet loss;
  * grads only, input_grads only, both: the same bits; the mention-text Linear is never read and its gradients never written.
Every test prints its measured maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import DrinConfig
from drin_amd.model import Model, _Call, _fill_params, _param_list
from oracle import drin_oracle as O
from oracle.cases import TINY, build_case
from tests.drin_encoder_restatement import AVG, MAX, head_forward
from tests.test_gpu_mention_rows import bits, mention_rows_fwd

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"bf16x3": 1e-4, "f32": 1e-5}
GRAD_TOL = 2e-4
PREC = {"bf16x3": _lib.PREC_BF16X3, "f32": _lib.PREC_F32}
REPR = {AVG: _lib.REPR_AVG_EXTRACT, MAX: _lib.REPR_MAX_POOL}
KEYS_MT = ("vertex_encoder.mention_text_encoder.final_layer.linear.weight", "vertex_encoder.mention_text_encoder.final_layer.linear.bias")
ZERO_LAYERS = "tiny_wd_layers0"


def case(name):
    if name == ZERO_LAYERS:                                             # the score reads the layer-0 vertices alone
        cfg = DrinConfig(num_gcn_layers=0, **TINY)
        return cfg, synth.make_state_dict(cfg, 8), synth.make_batch(cfg, 3, 41)
    return build_case(name)


class Setup:
    """One case on the device: the linear model as the parameter container, the call's C structs, an encoded block."""

    def __init__(self, name, precision, encoded):
        self.cfg, sd, batch = case(name)
        self.sd = sd
        self.batch = [t.to(DEV) for t in batch[:14]]
        self.model = Model(self.cfg, precision=precision).to(DEV)
        self.model.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
        self.call = _Call(self.cfg, self.batch, PREC[precision])
        self.params = _param_list(self.model)
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        self.keys = [name_of[id(p)] for p in self.params]             # state-dict names in the C structs' order
        self.tensors, self.pc = self.call.param_struct(self.params)
        B, L, D = self.batch[0].shape
        g = torch.Generator(device=DEV).manual_seed(17)
        self.encoded = torch.randn(B, L, D, device=DEV, generator=g) if encoded else None
        self.shape = (B, L, D)
        self.N = self.cfg.num_candidates_model

    def head(self, encoder, representation, grad_encoded=None, with_encoded=True, keep_positions=False):
        """`keep_positions`: the head of a backward pass alone - max_index as the forward pass left it."""
        B, _L, D = self.shape
        h = _lib.DrinMentionHeadC()
        h.struct_size, h.encoder, h.representation = C.sizeof(h), encoder, representation
        if not keep_positions:
            self.idx = torch.full((2, B, D), -5, dtype=torch.int32, device=DEV)
        if encoder == _lib.MENTION_ROWS:
            h.max_index = self.idx.data_ptr()
            if self.encoded is not None and with_encoded:
                h.encoded = self.encoded.data_ptr()
            if grad_encoded is not None:
                h.grad_encoded = grad_encoded.data_ptr()
        return h

    def forward(self, head, training=True, rows=False, trace=False):
        lib, call = _lib.load(), self.call
        self.ws, scores = call.workspace(training), call.scores()
        pc = self.pc
        if rows:                                                        # the mention-text Linear is not part of the model
            pc = _lib.DrinParamsC()
            _fill_params(pc, (None, None) + tuple(self.tensors[2:]), call.per_layer)
        self.pc_used = pc
        tr, taps = None, {}
        if trace:
            tr = _lib.DrinTraceC()
            B, _L, D = self.shape
            taps = {"mt0": torch.full((B, D), float("nan"), device=DEV)}
            tr.mention_text_vertex[0] = taps["mt0"].data_ptr()
        args = (C.byref(call.cfg), C.byref(call.batch), C.byref(pc), self.ws.data_ptr(), self.ws.numel(), scores.data_ptr(),
                1 if training else 0, None if tr is None else C.byref(tr), None)
        if head == "parent":
            _lib.check(lib.drin_forward_staged(*args, call.stream()))
        else:
            _lib.check(lib.drin_forward_staged_head(*args, None if head is None else C.byref(head), call.stream()))
        return scores, taps

    def backward(self, head, G, want_params=True, want_inputs=("mention_text",), sentinel=None):
        """(parameter gradients or None, {input role: gradient}); the gradient buffers start as zeros, as Model's do."""
        lib, call = _lib.load(), self.call
        grads, gc = None, None
        if want_params:
            grads = [torch.zeros_like(p) for p in self.tensors]
            if sentinel is not None:
                grads[0].fill_(sentinel), grads[1].fill_(sentinel)
            gc = _lib.DrinParamGradsC()
            _fill_params(gc, grads, call.per_layer)
        ig, outs = None, {}
        if want_inputs:
            ig = _lib.DrinInputGradsC()
            for role in want_inputs:
                outs[role] = torch.full(tuple(self.batch[0].shape), float("nan"), device=DEV)
                setattr(ig, role, outs[role].data_ptr())
            self.scratch = call.byte_buffer(lib.drin_input_grad_scratch_bytes(C.byref(call.cfg)))
            ig.scratch, ig.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel()
        args = (C.byref(call.cfg), C.byref(call.batch), C.byref(self.pc_used), self.ws.data_ptr(), self.ws.numel(), G.data_ptr(),
                None if gc is None else C.byref(gc), None if ig is None else C.byref(ig), None)
        if head == "parent":
            _lib.check(lib.drin_backward_ex(*args, call.stream()))
        else:
            _lib.check(lib.drin_backward_head(*args, None if head is None else C.byref(head), call.stream()))
        return grads, outs


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_null_and_linear_heads_give_the_parents_bits(precision):
    s = Setup("tiny_wd", precision, encoded=False)
    G = torch.randn(s.shape[0], s.N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    want_scores, _ = s.forward("parent")
    want_grads, want_in = s.backward("parent", G)
    for head in (None, s.head(_lib.MENTION_LINEAR, _lib.REPR_AVG_EXTRACT)):
        scores, _ = s.forward(head)
        assert torch.equal(bits(scores), bits(want_scores))
        grads, ins = s.backward(head, G)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, want_grads))
        assert torch.equal(bits(ins["mention_text"]), bits(want_in["mention_text"]))
        assert (s.idx == -5).all()                                      # a linear head never touches max_index


def fp64_reference(s, representation, at):
    """(scores, G = d triplet loss / d scores, {key: parameter gradient}, d raw, d encoded) in fp64 at the positions `at`."""
    batch = [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in s.batch]
    batch[0].requires_grad_(True)
    enc = None if s.encoded is None else s.encoded.detach().cpu().double().requires_grad_(True)
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in s.sd.items() if k not in KEYS_MT}
    at = [None, None] if at is None else [a.cpu() for a in at]
    scores = head_forward(p, batch, enc, representation, at_edge=at[0], at_vertex=at[1], **O.config_kwargs(s.cfg))
    y = torch.zeros(scores.shape[0], s.N - 1, dtype=torch.float64)
    y[torch.arange(scores.shape[0]), torch.arange(scores.shape[0]) % (s.N - 1)] = 1.0
    leaf = scores.detach().requires_grad_(True)
    O.triplet_loss(y, leaf).backward()
    G = leaf.grad
    scores.backward(G)
    return scores.detach(), G, {k: v.grad for k, v in p.items()}, batch[0].grad, None if enc is None else enc.grad


def err(got, ref, tag):
    e = float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"{tag}: max err / max|ref| = {e:.3g}")
    return e


CASES = ["tiny_wd", "tiny_wm", "tiny_wd_static", "tiny_wd_edges_1010", "tiny_wd_vector", "tiny_wm_vector_static", ZERO_LAYERS]


@pytest.mark.parametrize("with_encoded", [False, True])
@pytest.mark.parametrize("representation", [AVG, MAX])
@pytest.mark.parametrize("name", CASES)
def test_rows_head_against_fp64(name, representation, with_encoded):
    for precision in ("f32", "bf16x3") if name in ("tiny_wd", "tiny_wm") else ("bf16x3",):
        s = Setup(name, precision, with_encoded)
        tag = f"{name} {representation} encoded={with_encoded} {precision}"
        B, L, D = s.shape
        grad_enc = torch.full(s.shape, float("nan"), device=DEV) if with_encoded else None
        head = s.head(_lib.MENTION_ROWS, REPR[representation], grad_enc)
        scores, taps = s.forward(head, rows=True, trace=True)
        # the layer-0 mention-text vertex and the positions are the kernel's own entry point's, bit for bit
        edge, vert, idx = mention_rows_fwd(s.call.keep[0], s.encoded, s.call.keep[1], s.call.keep[2], REPR[representation])
        assert torch.equal(bits(taps["mt0"]), bits(vert))
        if representation == MAX:
            assert torch.equal(s.idx, idx)
        else:
            assert (s.idx == -5).all()
        at = (s.idx[0].long(), s.idx[1].long()) if representation == MAX else None
        ref_scores, G, ref_p, ref_raw, ref_enc = fp64_reference(s, representation, at)
        assert float((scores.double().cpu() - ref_scores).abs().max()) <= TOL[precision], tag
        print(f"{tag}: scores max abs err = {float((scores.double().cpu() - ref_scores).abs().max()):.3g}")
        # without the trace the dead work of the last layer is skipped: the training forward proper, then backward
        scores, _ = s.forward(head, rows=True)
        Gd = G.float().to(DEV).contiguous()
        grads, ins = s.backward(head, Gd, sentinel=7.0)
        assert (grads[0] == 7.0).all() and (grads[1] == 7.0).all()      # the mention-text Linear's gradients: never written
        keys = s.keys
        assert len(keys) == len(grads) == len(s.sd)
        dead = s.cfg.num_gcn_layers == 0
        for k, g in zip(keys, grads):
            if k in KEYS_MT:
                continue
            ref = ref_p[k]
            if ref is None or float(ref.abs().max()) == 0.0:           # the score does not depend on it
                assert not g.any(), k
                continue
            assert err(g, ref, f"{tag} {k}") <= GRAD_TOL, k
        raw = ins["mention_text"]
        assert not torch.isnan(raw).any()
        if ref_raw is None or float(ref_raw.abs().max()) == 0.0:
            assert not raw.any()                                        # no GCN layer and an encoded block: a zero gradient
            assert dead and with_encoded
        else:
            assert err(raw, ref_raw, tag + " d mention_text") <= GRAD_TOL
        if with_encoded:
            assert not torch.isnan(grad_enc).any()
            assert err(grad_enc, ref_enc, tag + " d encoded") <= GRAD_TOL
            # grads only and input_grads only: the same bits as both at once
            only_p = torch.full(s.shape, float("nan"), device=DEV)
            g2, _ = s.backward(s.head(_lib.MENTION_ROWS, REPR[representation], only_p, keep_positions=True), Gd, want_inputs=())
            assert torch.equal(bits(only_p), bits(grad_enc)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(g2[2:], grads[2:]))
            only_i = torch.full(s.shape, float("nan"), device=DEV)
            h3 = s.head(_lib.MENTION_ROWS, REPR[representation], only_i, keep_positions=True)
            _, in3 = s.backward(h3, Gd, want_params=False)
            assert torch.equal(bits(only_i), bits(grad_enc)) and torch.equal(bits(in3["mention_text"]), bits(raw))


def test_none_avg_uses_one_row_twice():
    """"none" + "avg extract": the edge row and the vertex are the same row; against the linear head with W = I, b = 0 in exact
    fp32 the scores are the same bits (x I^T + 0 is exact)."""
    s = Setup("tiny_wd", "f32", encoded=False)
    D = s.shape[2]
    with torch.no_grad():
        s.params[0].copy_(torch.eye(D, device=DEV)), s.params[1].zero_()
    s.tensors, s.pc = s.call.param_struct(s.params)
    linear, _ = s.forward("parent", training=False)
    rows, _ = s.forward(s.head(_lib.MENTION_ROWS, _lib.REPR_AVG_EXTRACT), training=False, rows=True)
    gap = float((linear - rows).abs().max())
    print(f"none_avg vs linear(W = I): max abs gap = {gap:.3g}")
    assert gap <= TOL["f32"]    # two fp32 evaluations of one function (the two span-mean kernels associate their sums differently)


def test_head_refusals_on_the_device():
    s = Setup("tiny_wd", "f32", encoded=True)
    lib = _lib.load()
    h = s.head(_lib.MENTION_LINEAR, _lib.REPR_MAX_POOL)
    with pytest.raises(_lib.DrinError, match="args.py:12-13") as e:
        s.forward(h)
    assert e.value.status == _lib.E_UNSUPPORTED
    h = s.head(_lib.MENTION_ROWS, _lib.REPR_MAX_POOL)
    h.max_index = None
    with pytest.raises(_lib.DrinError, match="drin_forward_staged_head: head.max_index is NULL") as e:
        s.forward(h, rows=True)
    assert e.value.status == _lib.E_NULL
    h = s.head(_lib.MENTION_ROWS, _lib.REPR_AVG_EXTRACT)
    h.struct_size -= 8
    with pytest.raises(_lib.DrinError, match="struct_size") as e:
        s.forward(h, rows=True)
    assert e.value.status == _lib.E_SHAPE
    assert np.isfinite(s.forward(None)[0].cpu().numpy()).all() and lib.drin_version() == 12


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_folded_path_under_a_head(precision):
    """drin_forward_prepared_head: a NULL head and {LINEAR, AVG_EXTRACT} give drin_forward_prepared's bits; a ROWS head scores as
    the layer-by-layer path does (two evaluations of one function: the path's bar), with the same positions; drin_prepare accepts
    a model without the mention-text Linear."""
    s = Setup("tiny_wd", precision, encoded=True)
    lib, call = _lib.load(), s.call
    assert lib.drin_fused_supported(C.byref(call.cfg)) == _lib.OK
    n = lib.drin_prepared_bytes(C.byref(call.cfg))
    ws = call.byte_buffer(lib.drin_fused_workspace_bytes(C.byref(call.cfg)))
    rows_pc = _lib.DrinParamsC()
    _fill_params(rows_pc, (None, None) + tuple(s.tensors[2:]), call.per_layer)

    def prepared(pc):
        buf = torch.empty(n, dtype=torch.uint8, device=DEV)
        _lib.check(lib.drin_prepare(C.byref(call.cfg), C.byref(pc), buf.data_ptr(), n, call.stream()))
        return buf

    def folded(pc, buf, head, parent=False):
        scores = call.scores()
        args = (C.byref(call.cfg), C.byref(call.batch), C.byref(pc), buf.data_ptr(), ws.data_ptr(), ws.numel(), scores.data_ptr())
        if parent:
            _lib.check(lib.drin_forward_prepared(*args, call.stream()))
        else:
            _lib.check(lib.drin_forward_prepared_head(*args, None if head is None else C.byref(head), call.stream()))
        return scores

    full, lean = prepared(s.pc), prepared(rows_pc)
    want = folded(s.pc, full, None, parent=True)
    assert torch.equal(bits(folded(s.pc, full, None)), bits(want))
    assert torch.equal(bits(folded(s.pc, full, s.head(_lib.MENTION_LINEAR, _lib.REPR_AVG_EXTRACT))), bits(want))
    for representation in (AVG, MAX):
        for with_encoded in (False, True):
            head = s.head(_lib.MENTION_ROWS, REPR[representation], with_encoded=with_encoded)
            got = folded(rows_pc, lean, head)
            idx = s.idx.clone()
            assert torch.equal(bits(folded(s.pc, full, head)), bits(got))          # the Linear's plane is never read
            layers, _ = s.forward(s.head(_lib.MENTION_ROWS, REPR[representation], with_encoded=with_encoded), training=False, rows=True)
            gap = float((got - layers).abs().max())
            print(f"folded vs layers, {representation} encoded={with_encoded} {precision}: max abs gap = {gap:.3g}")
            assert gap <= TOL[precision] and torch.equal(idx, s.idx)
