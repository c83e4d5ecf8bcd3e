"""The grid over which the folded forward's plan (csrc/fused_forward.hip: `folded_plan`) is pinned, and the four answers the library
gives per configuration: `drin_fused_workspace_bytes`, `drin_image_contraction_passes`, `drin_image_contraction_side_tiles`,
`drin_workgroups_per_mention`.  Host-only.  Shared by tools/folded_plan_answers.py, which prints the answers of whatever library
`DRIN_LIB_PATH` selects, and tests/test_folded_plan_host.py, which compares them with tests/golden/folded_plan_answers.txt.

The grid stands on both sides of every gate of the plan: the four precisions x both feature dtypes x gathered rows / tables (the call
`indexed` exactly when the config has tables); the exact widths, the tiny ones, a guarded pair and one that is no multiple of 32 (off
the planes); N either side of the fp16 pass's 64 and of a 16-candidate chunk; pooled and token-level entity text; B either side of
the fp16 pass's half round of tiles (106 | 107 at N = 101), of the side schedule's 1 200 tiles (1011 | 1013) and of the
whole-mention chunk from 2 048 mentions up."""
import ctypes as C
import itertools

from drin_amd import _lib

PRECISIONS = (_lib.PREC_F32, _lib.PREC_BF16X3, _lib.PREC_BF16X3_ALL, _lib.PREC_BF16X3_IF16)
FEATURES = (_lib.FEAT_F32, _lib.FEAT_BF16)
ENTITIES = (0, 1000)
WIDTHS = ((768, 2048), (64, 128), (160, 288), (100, 200))
CANDIDATES = (11, 63, 64, 101)
TOKENS = (0, 8)
BATCHES = (1, 64, 106, 107, 1011, 1013, 2048, 4096)


def grid():
    return itertools.product(PRECISIONS, FEATURES, ENTITIES, WIDTHS, CANDIDATES, TOKENS, BATCHES)


def answers(lib=None):
    """One line per grid point, in grid order: workspace bytes, passes, side tiles, workgroups per mention."""
    lib = lib or _lib.load()
    out = []
    for prec, feat, E, (D, R), N, T, B in grid():
        c = _lib.DrinConfigC()
        _lib.check(lib.drin_default_config(C.byref(c)))
        c.batch, c.num_candidates, c.embed_dim, c.image_dim, c.entity_tokens = B, N, D, R, T
        c.precision, c.feature_dtype, c.num_entities = prec, feat, E
        indexed = 1 if E else 0
        out.append("%d %d %d %d" % (lib.drin_fused_workspace_bytes(C.byref(c)), lib.drin_image_contraction_passes(C.byref(c), indexed),
                                    lib.drin_image_contraction_side_tiles(C.byref(c), indexed),
                                    lib.drin_workgroups_per_mention(C.byref(c), 0)))
    return out
