"""`table_ops.cross_modal_edges`, the one wrapper of `drin_cross_modal_edges` / `_ex`: the bits of
`IndexedBatch.from_clip` - which forms its edges through it - on a float32 and on a bfloat16 table, with the mentions cut into slices
(`MAX_CALL_MENTIONS` = 2 under B = 3: a slice boundary is crossed), and an out-of-range candidate reaches the status words."""
import pytest
import torch

from drin_amd.config import default_config
from drin_amd.model import EntityTable, IndexedBatch, Model
from drin_amd.table_ops import cross_modal_edges, decode_status

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, E, WIDTH = 3, 5, 19, 16
SCALE, EPS = 100.0, 1e-8


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("stored", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_wrapper_has_the_bits_of_from_clip_across_a_slice_boundary_and_reports_a_bad_row(stored, monkeypatch):
    g = torch.Generator().manual_seed(35)
    t_text, t_image = (torch.randn(E, WIDTH, generator=g).to(stored).to(DEV) for _ in range(2))
    m_image, m_text = (torch.randn(B, WIDTH, generator=g).to(DEV) for _ in range(2))
    index = torch.randint(0, E, (B, N), generator=g).to(DEV)
    table = EntityTable(torch.zeros(E, 4, device=DEV), None, None, None, None).set_clip(t_text, t_image)
    monkeypatch.setattr(Model, "MAX_CALL_MENTIONS", 2)
    batch = IndexedBatch.from_clip([None] * 7, table, index, m_image, m_text)           # no model: default config, its own check
    cfg = default_config()                                                               # (what from_clip reads scale and eps from)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    miet, mtei = cross_modal_edges(m_image, m_text, table.clip_text, table.clip_image, index, cfg.clip_logit_scale, cfg.cosine_eps, status, 2)
    assert miet.shape == mtei.shape == (B, N)
    assert torch.equal(bits(miet), bits(batch.miet_similarity)) and torch.equal(bits(mtei), bits(batch.mtei_similarity))
    whole = cross_modal_edges(m_image, m_text, table.clip_text, table.clip_image, index, cfg.clip_logit_scale, cfg.cosine_eps, None)
    assert torch.equal(bits(whole[0]), bits(miet)) and torch.equal(bits(whole[1]), bits(mtei))      # one call: the same bits
    assert status.tolist() == [0, 0, 0, 0]
    # a row outside the table, in the second slice: clamped, scored as the clamped row, reported with its pair of the SLICE's call
    bad = index.clone()
    bad[2, 4] = E + 3
    got = cross_modal_edges(m_image, m_text, table.clip_text, table.clip_image, bad, SCALE, EPS, status, 2)
    ref = cross_modal_edges(m_image, m_text, table.clip_text, table.clip_image, bad.clamp(0, E - 1), SCALE, EPS, None, 2)
    flag, pair, row = decode_status(status.tolist())
    assert (flag, pair, row) == (1, 0 * N + 4, E + 3)                                                # mention 2 is mention 0 of slice 2
    assert torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(bits(got[1]), bits(ref[1]))
    with pytest.raises(IndexError, match=f"row {E + 3} at pair 4 "):
        IndexedBatch.from_clip([None] * 7, table, bad, m_image, m_text)
