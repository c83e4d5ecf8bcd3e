"""CPU-side checks of the mention representation head: the new symbols exist in the library and in the
ctypes binding, `drin_mention_head` is laid out as the header says, and struct_size mismatch, NULL and misaligned arguments
give the library's error codes and name the entry point - all before any launch, so no GPU is needed."""
import ctypes as C
import os
import subprocess

from drin_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "drin_hip.h")
NEW = ("drin_forward_staged_head", "drin_backward_head", "drin_forward_prepared_head", "drin_mention_rows_fwd", "drin_mention_rows_bwd")
one = C.c_void_p(16)      # aligned, never dereferenced: every check below fails before a launch
odd = C.c_void_p(20)      # not 16-byte aligned
AVG, MAX = _lib.REPR_AVG_EXTRACT, _lib.REPR_MAX_POOL


def last():
    return _lib.load().drin_last_error().decode()


def test_new_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"DRIN_API int {name}(" in header, name
    assert lib.drin_version() == 12 == _lib.ABI_VERSION and _lib.KERNEL_CLASSES == 12      # additive: the ABI stays 12
    assert "mention_rows.hip" in __import__("drin_amd.build", fromlist=["SOURCES"]).SOURCES


def test_mention_head_mirror_matches_the_header(tmp_path):
    fields = [f for f, _ in _lib.DrinMentionHeadC._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(drin_mention_head));']
    lines += [f'  printf("{f} %zu\\n", offsetof(drin_mention_head, {f}));' for f in fields]
    lines += ['  printf("enums %d %d %d %d\\n", DRIN_MENTION_LINEAR, DRIN_MENTION_ROWS, DRIN_REPR_AVG_EXTRACT, DRIN_REPR_MAX_POOL);',
              '  return 0;', '}']
    src, exe = tmp_path / "head.c", tmp_path / "head"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)     # the header is plain C
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.DrinMentionHeadC)
    for f in fields:
        assert int(got[f]) == getattr(_lib.DrinMentionHeadC, f).offset, f
    assert got["enums"].split() == [str(v) for v in (_lib.MENTION_LINEAR, _lib.MENTION_ROWS, AVG, MAX)]


def test_mention_rows_fwd_validates_on_host():
    lib = _lib.load()
    f = lib.drin_mention_rows_fwd
    #        raw, dtype, encoded, start, end, repr, edge_row, vertex_row, max_index, batch, seq_len, width, stream
    assert f(None, 0, None, one, one, AVG, one, one, None, 2, 5, 8, None) == _lib.E_NULL
    assert last() == "drin_mention_rows_fwd: raw is NULL"
    assert f(one, 0, None, one, one, AVG, None, one, None, 2, 5, 8, None) == _lib.E_NULL and "edge_row is NULL" in last()
    assert f(one, 0, None, one, one, AVG, one, None, None, 2, 5, 8, None) == _lib.E_NULL and "vertex_row is NULL" in last()
    assert f(odd, 0, None, one, one, AVG, one, one, None, 2, 5, 8, None) == _lib.E_ALIGN
    assert last() == "drin_mention_rows_fwd: raw is not 16-byte aligned"
    assert f(one, 0, odd, one, one, AVG, one, one, None, 2, 5, 8, None) == _lib.E_ALIGN and "encoded" in last()
    assert f(one, 0, None, None, one, AVG, one, one, None, 2, 5, 8, None) == _lib.E_NULL and "start / end" in last()
    assert f(one, 0, None, None, None, MAX, one, one, None, 2, 5, 8, None) == _lib.E_NULL and "max_index is NULL" in last()
    assert f(one, 0, None, None, None, MAX, one, one, odd, 2, 5, 8, None) == _lib.E_ALIGN and "max_index" in last()
    assert f(one, 0, None, one, one, 2, one, one, one, 2, 5, 8, None) == _lib.E_SHAPE and "representation = 2" in last()
    assert f(one, 3, None, one, one, AVG, one, one, None, 2, 5, 8, None) == _lib.E_SHAPE and "raw_dtype = 3" in last()
    for width in (0, 6, -4):
        assert f(one, 0, None, one, one, AVG, one, one, None, 2, 5, width, None) == _lib.E_SHAPE and "multiple of 4" in last()
    assert f(one, 0, None, one, one, AVG, one, one, None, 0, 5, 8, None) == _lib.E_SHAPE and "batch = 0" in last()
    assert f(one, 0, None, one, one, AVG, one, one, None, 2, 0, 8, None) == _lib.E_SHAPE and "seq_len = 0" in last()


def test_mention_rows_bwd_validates_on_host():
    lib = _lib.load()
    f = lib.drin_mention_rows_bwd
    #        g_edge, g_vertex, start, end, max_index, repr, has_encoded, grad_raw, grad_encoded, batch, seq_len, width, stream
    assert f(one, one, one, one, None, AVG, 0, None, None, 2, 5, 8, None) == _lib.OK          # no destination: nothing to do
    assert f(one, one, one, one, None, AVG, 0, one, one, 2, 5, 8, None) == _lib.E_SHAPE
    assert last().startswith("drin_mention_rows_bwd: grad_encoded without an encoded block")
    assert f(one, one, None, None, None, MAX, 1, one, one, 2, 5, 8, None) == _lib.E_NULL and "max_index is NULL" in last()
    assert f(one, one, None, one, one, AVG, 1, one, one, 2, 5, 8, None) == _lib.E_NULL and "start / end" in last()
    assert f(odd, one, one, one, None, AVG, 1, one, one, 2, 5, 8, None) == _lib.E_ALIGN and "g_edge_row" in last()
    assert f(one, one, one, one, None, AVG, 1, one, odd, 2, 5, 8, None) == _lib.E_ALIGN and "grad_encoded" in last()
    assert f(one, one, one, one, None, AVG, 1, one, one, 2, 5, 10, None) == _lib.E_SHAPE and "multiple of 4" in last()
    assert f(one, one, one, one, None, 9, 1, one, one, 2, 5, 8, None) == _lib.E_SHAPE and "representation = 9" in last()


def _config():
    c = _lib.DrinConfigC()
    _lib.check(_lib.load().drin_default_config(C.byref(c)))
    c.batch = 2
    return c


def _head(encoder, representation, **kw):
    h = _lib.DrinMentionHeadC()
    h.struct_size, h.encoder, h.representation = C.sizeof(h), encoder, representation
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_head_entry_points_validate_the_head_on_host():
    lib = _lib.load()
    c, b = _config(), _lib.DrinBatchC()

    def fwd(h):
        return lib.drin_forward_staged_head(C.byref(c), C.byref(b), None, None, 0, None, 0, None, None, C.byref(h), None)

    def bwd(h):
        return lib.drin_backward_head(C.byref(c), C.byref(b), None, None, 0, None, None, None, None, C.byref(h), None)

    for call, who in ((fwd, "drin_forward_staged_head"), (bwd, "drin_backward_head")):
        h = _head(_lib.MENTION_ROWS, AVG)
        h.struct_size += 8
        assert call(h) == _lib.E_SHAPE and last().startswith(f"{who}: head.struct_size = {C.sizeof(h) + 8}")
        assert call(_head(2, AVG)) == _lib.E_SHAPE and last().startswith(f"{who}: head.encoder = 2")
        assert call(_head(_lib.MENTION_ROWS, 5)) == _lib.E_SHAPE and "head.representation = 5" in last()
        assert call(_head(_lib.MENTION_LINEAR, MAX)) == _lib.E_UNSUPPORTED
        assert last().startswith(f"{who}: {{DRIN_MENTION_LINEAR, DRIN_REPR_MAX_POOL}} is not built") and "args.py:12-13" in last()
        assert call(_head(_lib.MENTION_LINEAR, AVG, encoded=16)) == _lib.E_SHAPE and "DRIN_MENTION_ROWS only" in last()
        assert call(_head(_lib.MENTION_ROWS, AVG, grad_encoded=16)) == _lib.E_SHAPE and "grad_encoded without head.encoded" in last()
        assert call(_head(_lib.MENTION_ROWS, MAX)) == _lib.E_NULL and last().startswith(f"{who}: head.max_index is NULL")
        assert call(_head(_lib.MENTION_ROWS, MAX, max_index=20)) == _lib.E_ALIGN and who in last()
        assert call(_head(_lib.MENTION_ROWS, AVG, encoded=20)) == _lib.E_ALIGN
        # a good head: the next check is the batch's
        assert call(_head(_lib.MENTION_ROWS, MAX, max_index=16, encoded=32)) == _lib.E_NULL and "batch.mention_text is NULL" in last()
        assert call(_head(_lib.MENTION_LINEAR, AVG)) == _lib.E_NULL and "batch.mention_text is NULL" in last()


def test_prepared_head_validates_the_head_on_host():
    lib = _lib.load()
    c, b, p = _config(), _lib.DrinBatchC(), _lib.DrinParamsC()

    def call(h, params=None):
        return lib.drin_forward_prepared_head(C.byref(c), C.byref(b), params, None, None, 0, None, None if h is None else C.byref(h), None)

    who = "drin_forward_prepared_head"
    h = _head(_lib.MENTION_ROWS, AVG)
    h.struct_size = 8
    assert call(h) == _lib.E_SHAPE and last().startswith(f"{who}: head.struct_size = 8")
    assert call(_head(_lib.MENTION_LINEAR, MAX)) == _lib.E_UNSUPPORTED and last().startswith(f"{who}: {{DRIN_MENTION_LINEAR, DRIN_REPR_MAX_POOL}}")
    assert call(_head(_lib.MENTION_ROWS, MAX)) == _lib.E_NULL and last().startswith(f"{who}: head.max_index is NULL")
    assert call(_head(_lib.MENTION_ROWS, MAX, max_index=24)) == _lib.E_ALIGN
    for good in (None, _head(_lib.MENTION_ROWS, MAX, max_index=16), _head(_lib.MENTION_LINEAR, AVG)):
        assert call(good, C.byref(p)) == _lib.E_NULL and last() == "drin_forward_prepared: NULL argument"


def test_rows_head_lets_the_mention_text_linear_be_null():
    """Under DRIN_MENTION_ROWS params->w_mention_text / b_mention_text are never read: NULL passes validation, which then stops at
    the next missing argument; without a rows head the same params are refused."""
    lib = _lib.load()
    c, b, p = _config(), _lib.DrinBatchC(), _lib.DrinParamsC()
    for name, _ in _lib.DrinBatchC._fields_:
        if name not in ("entity_text_mask", "entity_index", "entity_text_cls", "index_status"):
            setattr(b, name, 16)
    for name in ("w_entity_text", "b_entity_text", "w_mention_image", "b_mention_image", "w_entity_image", "b_entity_image"):
        setattr(p, name, 16)
    for l in range(c.num_layers):
        for name in ("w_h", "b_h", "w_u", "b_u", "w_v", "b_v", "ln_weight", "ln_bias"):
            setattr(p.layer[l], name, 16)
    args = (C.byref(c), C.byref(b), C.byref(p), None, 0, None, 0, None, None)
    h = _head(_lib.MENTION_ROWS, AVG)
    assert lib.drin_forward_staged_head(*args, C.byref(h), None) == _lib.E_NULL and last() == "scores is NULL"
    assert lib.drin_forward_staged_head(*args, None, None) == _lib.E_NULL and "vertex encoder tensor NULL" in last()
    assert lib.drin_forward_staged(*args, None) == _lib.E_NULL and "vertex encoder tensor NULL" in last()
    # the Linear NULL and ANOTHER required tensor NULL: refused, in the forward and in the backward (the skip is by position)
    for name in ("w_entity_text", "b_entity_text", "w_mention_image", "b_mention_image", "w_entity_image", "b_entity_image"):
        setattr(p, name, None)
        assert lib.drin_forward_staged_head(*args, C.byref(h), None) == _lib.E_NULL and "vertex encoder tensor NULL" in last(), name
        assert lib.drin_backward_head(C.byref(c), C.byref(b), C.byref(p), None, 0, None, None, None, None, C.byref(h), None) == _lib.E_NULL
        assert "vertex encoder tensor NULL" in last(), name
        setattr(p, name, 20)
        assert lib.drin_forward_staged_head(*args, C.byref(h), None) == _lib.E_ALIGN, name
        setattr(p, name, 16)
    p.layer[0].w_h = None
    assert lib.drin_forward_staged_head(*args, C.byref(h), None) == _lib.E_NULL and "layer 0 tensor NULL" in last()
    p.layer[0].w_h = 16
    assert lib.drin_forward_staged_head(*args, C.byref(h), None) == _lib.E_NULL and last() == "scores is NULL"


def test_prepare_lets_only_the_mention_text_linear_be_null():
    lib = _lib.load()
    c, p = _config(), _lib.DrinParamsC()
    names = ("w_mention_text", "b_mention_text", "w_entity_text", "b_entity_text", "w_mention_image", "b_mention_image", "w_entity_image",
             "b_entity_image")
    for name in names[2:]:
        setattr(p, name, 16)
    for l in range(2):
        for name in ("w_h", "b_h", "w_u", "b_u", "w_v", "b_v", "ln_weight", "ln_bias"):
            setattr(p.layer[l], name, 16)
    n = lib.drin_prepared_bytes(C.byref(c))
    assert n > 0
    assert lib.drin_prepare(C.byref(c), C.byref(p), one, 0, None) == _lib.E_WORKSPACE            # NULL Linear: past the weight check
    for name in ("w_entity_text", "w_mention_image", "w_entity_image", "b_entity_text"):
        setattr(p, name, None)
        assert lib.drin_prepare(C.byref(c), C.byref(p), one, 0, None) == _lib.E_NULL and "only w_mention_text may be" in last(), name
        setattr(p, name, 16)
    p.layer[1].w_h = None
    assert lib.drin_prepare(C.byref(c), C.byref(p), one, 0, None) == _lib.E_NULL
