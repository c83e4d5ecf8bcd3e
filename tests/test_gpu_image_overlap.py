"""The concurrent schedule of the gathered-row image contraction (fused_forward.hip: the side schedule of folded_plan): an eager
`drin_forward_prepared` call runs the first row tiles of x_i C_i^T as persistent workgroups on the library's side stream, under
the entity stream pass, and the rest at full grid behind it; a call under stream capture keeps the one launch.  Every tile is
computed by the same code with the same K split either way, so the scores must be THE SAME BITS: `torch.equal`, no tolerance."""
import ctypes as C

import pytest
import torch

from drin_amd import _lib, synth
from drin_amd.config import wikimel_config
from drin_amd.model import Model

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 101                                   # wikimel: 100 candidates + the answer slot - B N is no multiple of 256 for odd B


def _cfg():
    return wikimel_config(max_entity_attr_token_len=8, max_mention_sentence_len=16, resnet_num_region=4)


def side_tiles(B, precision=_lib.PREC_BF16X3, features=_lib.FEAT_F32, indexed=0):
    lib = _lib.load()
    c = _lib.DrinConfigC()
    _lib.check(lib.drin_default_config(C.byref(c)))
    c.batch, c.num_candidates, c.embed_dim, c.image_dim, c.entity_tokens = B, N, 768, 2048, 8
    c.precision, c.feature_dtype = precision, features
    if indexed:
        c.num_entities = 1000
    return lib.drin_image_contraction_side_tiles(C.byref(c), indexed)


def smallest_concurrent_batch():
    """Smallest odd B (partial last row tile) whose eager call takes the side stream."""
    return next((B for B in range(1, 4096, 2) if side_tiles(B) > 0), None)


@pytest.fixture(scope="module")
def model():
    cfg = _cfg()
    m = Model(cfg, precision="bf16x3").to(DEV).eval()
    m.load_state_dict(synth.make_state_dict(cfg, 7))
    return m


def _batch(B, seed, dtype=torch.float32):
    return synth.make_device_batch(_cfg(), B, seed, torch.device(DEV, 0), dtype=dtype)[:14]


def _eager_and_captured(model, batch):
    with torch.no_grad():
        eager = model(batch).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(batch)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model(batch)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.isfinite(eager).all()
    return eager, captured


def test_the_schedule_engages_below_the_headline_batch():
    B = smallest_concurrent_batch()
    assert B is not None and B < 4096
    assert side_tiles(4096) > 0 and side_tiles(4096, features=_lib.FEAT_BF16) > 0


@pytest.mark.parametrize("features", ["f32", "bf16"])
def test_eager_scores_are_the_captured_call_s_bits(model, features):
    """Concurrent (eager) against serial (captured) at the smallest call that takes the side stream; B N % 256 != 0."""
    B = smallest_concurrent_batch()
    feat = _lib.FEAT_BF16 if features == "bf16" else _lib.FEAT_F32
    assert side_tiles(B, features=feat) > 0 and (B * N) % 256 != 0
    eager, captured = _eager_and_captured(model, _batch(B, 11, torch.bfloat16 if features == "bf16" else torch.float32))
    assert torch.equal(eager, captured)


def test_uneven_xcd_shares(model):
    """A call whose side part is no multiple of 8 row tiles: the eight XCDs' shares of the persistent walk differ."""
    B0 = smallest_concurrent_batch()
    B = next(B for B in range(B0, B0 + 400, 2) if side_tiles(B) % 8 != 0 and (B * N) % 256 != 0)
    eager, captured = _eager_and_captured(model, _batch(B, 12))
    assert torch.equal(eager, captured)


def test_slices_beside_a_tail_split(model):
    """A call whose partly filled last round of tiles is split over K (a few tail tiles: `tail_split_256`): the split belongs to the
    whole product, the side part and the rest take their tiles around it."""
    B0 = smallest_concurrent_batch()
    tiles = lambda B: -(-B * N // 256) * 3                                  # noqa: E731
    B = next(B for B in range(B0, B0 + 400, 2) if 0 < tiles(B) % 256 <= 64 and side_tiles(B) > 0)
    eager, captured = _eager_and_captured(model, _batch(B, 14))
    assert torch.equal(eager, captured)


def test_just_below_the_threshold_the_call_is_serial(model):
    B = smallest_concurrent_batch() - 2
    assert side_tiles(B) == 0
    eager, captured = _eager_and_captured(model, _batch(B, 13))
    assert torch.equal(eager, captured)


def test_back_to_back_calls(model):
    """The second of two calls in a row (same sizes: the allocator hands the second call the first one's workspace) scores what a
    single call scores: the side part of call 2 writes h_image only behind call 1's readers."""
    B = smallest_concurrent_batch()
    first, second = _batch(B, 21), _batch(B, 22)
    with torch.no_grad():
        model(first)
        twice = model(second).clone()
        torch.cuda.synchronize()
        fresh = Model(model.cfg, precision="bf16x3").to(DEV).eval()
        fresh.load_state_dict(synth.make_state_dict(model.cfg, 7))
        once = fresh(second).clone()
    assert torch.equal(twice, once)


def test_query_is_zero_where_the_contraction_waits_for_the_stream_pass():
    """Indexed rows and the one-pass fp16 contraction take their A operand from the stream pass; fp32 runs another kernel."""
    assert side_tiles(4096, indexed=1) == 0
    assert side_tiles(4096, precision=_lib.PREC_BF16X3_IF16) == 0
    assert side_tiles(4096, precision=_lib.PREC_F32) == 0
    assert side_tiles(4096, precision=_lib.PREC_BF16X3_IF16, features=_lib.FEAT_BF16) > 0   # (the fp16 gate is fp32 rows only)
    assert side_tiles(64) == 0
