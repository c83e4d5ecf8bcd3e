"""No GPU: where the capped launchers stop growing their grid, as far as the host can see it (tests/test_gpu_launch_caps.py runs
them past that point; DESIGN.md section 29 holds the inventory).  The GPU cases read the workgroup count of the row backward
kernels back from the scratch queries; here the same arithmetic is pinned at the cap and one row past it, and the entry points
whose grid.y is the batch refuse the first batch that does not fit - before anything is launched (every pointer below is a small
constant that no kernel could dereference)."""
import ctypes as C

import pytest

from drin_amd import _lib

ONE = C.c_void_p(16)      # aligned, never dereferenced
ROW_BWD_BLOCKS = 256      # kRowBwdBlocks of csrc/ghmfc_rows.hip: four rows per workgroup, 1024 rows per trip
cdiv = lambda a, b: -(-a // b)   # noqa: E731


def last():
    return _lib.load().drin_last_error().decode()


@pytest.mark.parametrize("E", [16, 260, 768, 2048])
def test_row_backward_workgroups_stop_growing_at_1024_rows(E):
    lib = _lib.load()
    ln = lambda rows: lib.drin_layernorm_res_bwd_scratch_floats(rows, E) // (2 * E)   # noqa: E731
    gate = lambda rows: lib.drin_gate_mix_bwd_scratch_floats(rows, E) // (2 * E + 4)   # noqa: E731
    assert lib.drin_layernorm_res_bwd_scratch_floats(1025, E) % (2 * E) == 0 and lib.drin_gate_mix_bwd_scratch_floats(1025, E) % (2 * E + 4) == 0
    for blocks in (ln, gate):
        for rows in (1, 4, 5, 1000, 1023, 1024):
            assert blocks(rows) == cdiv(rows, 4), rows                # one trip: a wave per row
        assert blocks(1024) == ROW_BWD_BLOCKS
        for rows in (1025, 2051, 4099, 5003, 100000):                 # the rows of the GPU cases: fewer workgroups than cdiv(rows, 4)
            assert blocks(rows) == ROW_BWD_BLOCKS < cdiv(rows, 4), rows


def test_grid_y_batches_are_refused_one_past_the_limit():
    lib = _lib.load()
    for fn, who in ((lib.drin_seq_max_train_fwd, "drin_seq_max_train_fwd"), (lib.drin_seq_max_bwd, "drin_seq_max_bwd")):
        assert fn(ONE, ONE, ONE, 65536, 2, 8, None) == _lib.E_SHAPE and last() == f"{who}: batch = 65536 is not in [1, 65535]"
    # num_candidates is the grid.x side of the (candidate quads, mention) grid of the cosine kernels
    assert lib.drin_cosine_rows_fwd(ONE, ONE, ONE, 5, 65536, 8, 1e-8, None) == _lib.E_SHAPE and "num_candidates = 65536" in last()
    assert lib.drin_cosine_rows_bwd(ONE, ONE, ONE, ONE, ONE, ONE, 1 << 40, 5, 65536, 8, 1e-8, None) == _lib.E_SHAPE and "num_candidates = 65536" in last()
    assert lib.drin_cosine_rows_indexed_fwd(ONE, ONE, ONE, 9, ONE, 5, 65536, 8, 1e-8, None, None) == _lib.E_SHAPE and "num_candidates = 65536" in last()
    assert lib.drin_table_topk_workspace_bytes(65536, 64, 8, 5, 0) == 0


def _layers_call(batch, n, vector, precision=None, dynamic=True, layers=2, width=8, image_width=None):
    """(config, batch, params) of a layer-by-layer call whose every pointer is the constant 16: what passes the argument checks
    stops at the NULL workspace, before anything could be launched"""
    lib = _lib.load()
    c, b, p = _lib.DrinConfigC(), _lib.DrinBatchC(), _lib.DrinParamsC()
    _lib.check(lib.drin_default_config(C.byref(c)))
    c.batch, c.num_candidates, c.embed_dim, c.image_dim, c.num_layers = batch, n, width, image_width or width, layers
    c.vector_edges, c.dynamic_edges = int(vector), int(dynamic)
    c.precision = _lib.PREC_F32 if precision is None else precision
    for name, _ in _lib.DrinBatchC._fields_:
        if name not in ("entity_text_mask", "entity_index", "entity_text_cls", "index_status"):
            setattr(b, name, 16)
    for name in ("w_mention_text", "b_mention_text", "w_entity_text", "b_entity_text", "w_mention_image", "b_mention_image", "w_entity_image",
                 "b_entity_image"):
        setattr(p, name, 16)
    for l in range(layers):
        for name in ("w_h", "b_h", "w_u", "b_u", "w_v", "b_v", "ln_weight", "ln_bias", "w_m", "b_m"):
            setattr(p.layer[l], name, 16)
    return c, b, p


def _forward(c, b, p):
    return _lib.load().drin_forward(C.byref(c), C.byref(b), C.byref(p), None, 0, ONE, 1, None, None)


def _backward(c, b, p):
    return _lib.load().drin_backward(C.byref(c), C.byref(b), C.byref(p), None, 0, ONE, C.byref(_lib.DrinParamGradsC()), None)


def test_layer_calls_refuse_what_a_launcher_would_refuse_among_the_argument_checks():
    """include/drin_hip.h: drin_forward* / drin_backward* run to their end or refuse before the first launch.  The two sizes a
    launcher of the path refuses are refused by the entry points, with the launchers' own predicates; every size beside them
    goes on to the next check (here: the NULL workspace)."""
    admitted = lambda rc: rc == _lib.E_NULL and last().startswith("workspace is NULL")   # noqa: E731
    # vector edges with a live edge update: the backward stops at 65 535 mentions, the forward does not
    for batch, fits in ((65535, True), (65536, False), (65541, False)):
        call = _layers_call(batch, 2, vector=True)
        assert admitted(_forward(*call)), batch
        rc = _backward(*call)
        assert admitted(rc) if fits else (rc == _lib.E_SHAPE and "vector-edge update" in last() and f"batch = {batch}" in last()), batch
    for kw in (dict(vector=False), dict(vector=True, dynamic=False), dict(vector=True, layers=1)):   # no live vector-edge update
        call = _layers_call(65541, 2, **kw)
        assert admitted(_forward(*call)) and admitted(_backward(*call)), kw
    # the exact-fp32 product of the most rows: 4 M with live vector-edge updates, 2 M otherwise, at most 65 535 * 128
    limit = 65535 * 128
    assert 4 * 65541 * 33 > limit >= 2 * 65541 * 33
    call = _layers_call(65541, 33, vector=True)
    assert _forward(*call) == _lib.E_SHAPE and f"{4 * 65541 * 33} rows" in last() and "split the batch" in last()
    assert admitted(_forward(*_layers_call(65541, 33, vector=False))) and admitted(_backward(*_layers_call(65541, 33, vector=False)))
    n = limit // (2 * 32768)                                          # Model.MAX_CALL_MENTIONS mentions: the most candidates whose 2 M rows fit
    assert admitted(_forward(*_layers_call(32768, n, vector=False))) and admitted(_backward(*_layers_call(32768, n, vector=False)))
    call = _layers_call(32768, n + 1, vector=False)
    assert _forward(*call) == _lib.E_SHAPE and _backward(*call) == _lib.E_SHAPE and "exact-fp32" in last()
    # split-bf16 with reductions that are multiples of 32 never takes that kernel for a pair-sized product: admitted
    wide = dict(vector=False, precision=_lib.PREC_BF16X3, width=64)
    assert admitted(_forward(*_layers_call(32768, n + 1, **wide))) and admitted(_backward(*_layers_call(32768, n + 1, **wide)))
    assert _forward(*_layers_call(32768, n + 1, vector=False, precision=_lib.PREC_BF16X3, width=8)) == _lib.E_SHAPE   # D = 8: exact fp32
    # ... and is asked product by product: with only the image width off the multiples of 32, the one exact-fp32 product is the
    # entity image encoder's, of M rows - 2 M past the limit is admitted, M past it is not
    odd_image = dict(vector=False, precision=_lib.PREC_BF16X3, width=64, image_width=8)
    assert admitted(_forward(*_layers_call(32768, n + 1, **odd_image))) and admitted(_backward(*_layers_call(32768, n + 1, **odd_image)))
    assert _forward(*_layers_call(32768, 2 * n + 2, **odd_image)) == _lib.E_SHAPE and f"{32768 * (2 * n + 2)} rows" in last()
    # vector edges at D = 32: every forward product reduces over D; the backward's dfv W_v over D / 2 = 16, with 2 M rows
    half = dict(vector=True, precision=_lib.PREC_BF16X3, width=32)
    assert admitted(_forward(*_layers_call(32768, n + 1, **half)))
    assert _backward(*_layers_call(32768, n + 1, **half)) == _lib.E_SHAPE and f"{2 * 32768 * (n + 1)} rows" in last()
    # a single untraced layer has one live entity vertex type: W_h over M rows
    assert admitted(_forward(*_layers_call(32768, n + 1, vector=False, layers=1))) and admitted(_backward(*_layers_call(32768, n + 1, vector=False, layers=1)))


def test_prepared_forward_refuses_the_stream_pass_limit_among_its_argument_checks():
    """launch_entity_stream takes at most 65 535 mentions and runs behind the image product, the folded head and the q product:
    drin_forward_prepared asks its predicate first.  (Every pointer NULL: an admitted batch stops at the NULL-argument check.)"""
    lib = _lib.load()
    c = _lib.DrinConfigC()
    _lib.check(lib.drin_default_config(C.byref(c)))
    for batch, fits in ((65535, True), (65536, False), (65541, False)):
        c.batch = batch
        rc = lib.drin_forward_prepared(C.byref(c), None, None, None, None, 0, None, None)
        if fits:
            assert rc == _lib.E_NULL and last() == "drin_forward_prepared: NULL argument"
        else:
            assert rc == _lib.E_SHAPE and f"batch = {batch}" in last() and "entity stream pass" in last()
        assert lib.drin_forward_prepared_head(C.byref(c), None, None, None, None, 0, None, None, None) == rc
