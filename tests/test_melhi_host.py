"""CPU checks of the MELHI baseline: the test-side restatement against the reference's goldens (the tiny cases and the
shape cases of melhi_shapes.npz, with what each shape case must reach), torch's tie order, the Module's keys /
initialisation / dataset refusal, and the C ABI's structs and host-side refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from drin_amd import _lib
from drin_amd.melhi import MelhiConfig, Model, orders_and_lengths, torch_order
from tests.melhi_inputs import (CASES, KEYS, SHAPE_CASES, SHAPE_CHECKSUM, SHAPE_FORWARD_ONLY, TINY, geometry, grad_weights,
                                melhi_inputs)
from tests.melhi_restatement import melhi_scores

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TINY_CASES = [n for n, c in CASES.items() if not c.get("full") and "geom" not in c]


def tiny_cfg() -> MelhiConfig:
    return MelhiConfig(num_candidates=TINY["N"], embed_dim=TINY["D"], image_dim=TINY["R"], mention_tokens=TINY["L"],
                       image_regions=TINY["P"])


def case_model(name: str) -> Model:
    g = geometry(name)
    cfg = MelhiConfig(num_candidates=g["N"], embed_dim=g["D"], image_dim=g["R"], mention_tokens=g["L"], image_regions=g["P"])
    torch.manual_seed(CASES[name]["seed"])
    return Model(cfg)


def as_torch(batch, dtype=torch.float64, device="cpu"):
    out = []
    for i, x in enumerate(batch):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if isinstance(x, torch.Tensor):
            x = x.to(device, dtype if x.is_floating_point() else torch.int64)
        out.append(x)
    return out


@pytest.fixture(scope="module")
def tiny_golden():
    return np.load(os.path.join(GOLDEN, "melhi_tiny.npz"))


@pytest.fixture(scope="module")
def shapes_golden():
    return np.load(os.path.join(GOLDEN, "melhi_shapes.npz"))


def restated(name: str, grads: bool = True):
    """(scores, mask, fp64 state dict) of case `name` by the restatement on the CPU; with `grads`, the state dict's .grad hold
    the gradients of sum(scores * grad_weights) (when no score is NaN)."""
    model = case_model(name)
    sd = {k: v.detach().double().requires_grad_(grads) for k, v in model.state_dict().items()}
    assert list(sd) == KEYS
    batch = melhi_inputs(name, {k: v.detach().float().numpy() for k, v in sd.items()})
    t1, t2 = CASES[name].get("thres", (0.3, 0.3))
    scores, mask = melhi_scores(as_torch(batch), sd, t1, t2, return_mask=True)
    if grads and not torch.isnan(scores).any():
        (scores * torch.from_numpy(grad_weights(name, scores.shape)).double()).sum().backward()
    return scores.detach(), mask, sd, batch


@pytest.mark.parametrize("name", TINY_CASES + SHAPE_CASES)
def test_restatement_matches_reference_goldens(name, tiny_golden, shapes_golden):
    golden = shapes_golden if name in SHAPE_CASES else tiny_golden
    scores, mask, sd, _ = restated(name)
    np.testing.assert_allclose([sd[k].detach().sum().item() for k in KEYS], golden[f"{name}/w_sums"], rtol=1e-9, atol=1e-9)
    assert np.array_equal(mask.numpy().astype(np.uint8), golden[f"{name}/mask"])
    got = scores.numpy()
    if name in SHAPE_CHECKSUM:   # sums, L2 norms and leading elements (the melhi_full.npz form)
        assert not np.isnan(got).any()
        assert abs(got.sum() - golden[f"{name}/scores_sum"]) < 2e-6 * got.size
        assert abs(np.linalg.norm(got) - golden[f"{name}/scores_l2"]) < 2e-6 * np.sqrt(got.size)
        assert np.abs(got.flatten()[:32] - golden[f"{name}/scores_head"]).max() < 2e-6
        for k in KEYS:
            g = sd[k].grad.numpy() if sd[k].grad is not None else np.zeros(sd[k].shape)
            scale = max(np.abs(g).max(), 1e-6)
            want_l2 = float(golden[f"{name}/grad_l2/{k}"])
            assert abs(np.linalg.norm(g) - want_l2) <= 2e-5 * max(want_l2, 1e-12), k
            assert np.abs(g.flatten()[:16] - golden[f"{name}/grad_head/{k}"]).max() / scale < 2e-5, k
        return
    want = golden[f"{name}/scores"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max(initial=0.0) < 2e-6
    if name in SHAPE_FORWARD_ONLY:
        assert f"{name}/grad/{KEYS[0]}" not in golden
    if f"{name}/grad/{KEYS[0]}" in golden:
        for k in KEYS:
            ref = golden[f"{name}/grad/{k}"]
            got = sd[k].grad.numpy() if sd[k].grad is not None else np.zeros_like(ref)   # W_hh unused: no recurrence
            err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
            assert err < 2e-5, (k, err)
    else:
        assert name in SHAPE_FORWARD_ONLY or np.isnan(want).any()


def test_shape_cases_reach_their_corners():
    """What each shape case is for holds on its inputs (a case that missed it would pass vacuously)."""
    for name in SHAPE_CASES:
        scores, _, _, batch = restated(name, grads=False)
        rows_nan = torch.isnan(scores).any(-1)
        if name == "max_len_nan":
            assert 0 < rows_nan.sum().item() <= len(rows_nan) // 4, rows_nan.sum().item()
        else:
            assert not rows_nan.any(), name
        L = geometry(name)["L"]
        order, lengths = orders_and_lengths(batch[2], batch[3], torch.from_numpy(batch[1]), L)
        start, end, mlen = batch[2].numpy(), batch[3].numpy(), batch[1].sum(-1)
        if name == "long_lanes":
            assert all(lengths[s].max() >= 256 for s in range(2)), lengths.max(1)
        if name == "short_L":
            assert lengths.max() == 1            # T0 = T1 = 0: no long recurrence on either side
            assert (start > 1).any()             # a real length-1 left context (token 1)
            assert (mlen > end).any()            # a real length-1 right context
        if name == "max_len_nan":
            assert lengths[0].max() == L - 1
        if CASES[name]["B"] >= 64:              # ties in both orders
            for s in range(2):
                assert (np.diff(lengths[s][order[s]]) == 0).sum() > len(order[s]) // 2, (name, s)


def test_golden_cases_cover_the_corners(tiny_golden):
    assert np.isnan(tiny_golden["b16_empty_span/scores"]).any()
    assert tiny_golden["b16_mask_on/mask"].all() and not tiny_golden["b16_mask_off/mask"].any()
    assert 0 < tiny_golden["b64_ties/mask"].sum() < 64
    for name in ("b64_ties", "b300_ties", "b64_top_ties"):   # ties in both orders, and at the longest length
        model = case_model(name)
        batch = melhi_inputs(name, {k: v.detach().numpy() for k, v in model.state_dict().items()})
        order, lengths = orders_and_lengths(batch[2], batch[3], torch.from_numpy(batch[1]), TINY["L"])
        for s in range(2):
            ls = lengths[s][order[s]]
            assert (np.diff(ls) == 0).sum() > len(ls) // 2
        if name == "b64_top_ties":
            assert all((lengths[s] == lengths[s].max()).sum() > 1 for s in range(2))


@pytest.mark.parametrize("B", [4, 64, 300, 1000])
def test_order_rule_reproduces_packing(B):
    """The order the port hands the library is the one pack_sequence(enforce_sorted=False) packs by, ties included."""
    g = torch.Generator().manual_seed(B)
    lengths = torch.randint(1, 5, (B,), generator=g).tolist()
    seqs = [torch.zeros(n, 2) for n in lengths]
    packed = nn.utils.rnn.pack_sequence(seqs, enforce_sorted=False)
    assert torch.equal(packed.sorted_indices, torch_order(lengths))
    if B >= 64:   # the unstable sort is what makes this matter: ties do not come back in index order
        assert not torch.equal(torch_order(lengths), torch.sort(torch.as_tensor(lengths), descending=True, stable=True)[1])


def test_state_dict_keys_and_initialisation():
    full = np.load(os.path.join(GOLDEN, "melhi_full.npz"))
    torch.manual_seed(0)
    sd = Model().state_dict()
    assert list(sd) == KEYS == list(full["state_dict_seed0/keys"])
    np.testing.assert_allclose([v.double().sum().item() for v in sd.values()], full["state_dict_seed0/sums"], rtol=1e-9, atol=1e-7)
    np.testing.assert_array_equal(np.stack([v.flatten()[:8].numpy() for v in sd.values()]), full["state_dict_seed0/heads"])


def test_wikimel_is_refused():
    with pytest.raises(NotImplementedError, match="wikidiverse"):
        MelhiConfig(dataset_name="wikimel")
    cfg = tiny_cfg()
    cfg.dataset_name = "wikimel"
    with pytest.raises(NotImplementedError):
        Model(cfg)


def test_model_refuses_cpu():
    model = Model(tiny_cfg())
    batch = melhi_inputs("b4", {k: v.detach().numpy() for k, v in model.state_dict().items()})
    with pytest.raises(RuntimeError, match="GPU only"):
        model(as_torch(batch, torch.float32))


def test_melhi_ctypes_mirror_the_header(tmp_path):
    header = os.path.join(REPO, "include", "drin_hip.h")
    pairs = [("drin_melhi_config", _lib.DrinMelhiConfigC), ("drin_melhi_batch", _lib.DrinMelhiBatchC),
             ("drin_melhi_params", _lib.DrinMelhiParamsC), ("drin_melhi_param_grads", _lib.DrinMelhiParamGradsC)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert int(got[f"{cname}.{field}"]) == getattr(cls, field).offset, f"{cname}.{field}"
    assert len(_lib.DrinMelhiParamsC._fields_) == 10


def _abi_call(lib, cfg, order, lengths, ws_bytes=None):
    one = C.c_void_p(256)   # never dereferenced: every refusal below happens on the host before a launch
    b = _lib.DrinMelhiBatchC(*[one] * 7)
    p = _lib.DrinMelhiParamsC(*[one] * 10)
    o = np.ascontiguousarray(order, dtype=np.int32)
    n = np.ascontiguousarray(lengths, dtype=np.int32)
    ws = lib.drin_melhi_workspace_bytes(C.byref(cfg), 0) if ws_bytes is None else ws_bytes
    return lib.drin_melhi_forward(C.byref(cfg), C.byref(b), C.byref(p), o.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p),
                                  one, ws, one, None)


def test_melhi_abi_refuses_bad_shapes_and_orders():
    lib = _lib.load()
    cfg = _lib.DrinMelhiConfigC(batch=4, num_candidates=4, embed_dim=16, image_dim=32, mention_tokens=12, image_regions=3,
                                precision=_lib.PREC_BF16X3, cosine_eps=1e-8, thres_tmim=0.3, thres_imie=0.3)
    inf, trn = lib.drin_melhi_workspace_bytes(C.byref(cfg), 0), lib.drin_melhi_workspace_bytes(C.byref(cfg), 1)
    assert 0 < inf < trn
    good_order = [[0, 1, 2, 3], [3, 2, 1, 0]]
    good_len = [[3, 2, 1, 1], [1, 1, 2, 4]]
    bad = [
        ([[0, 1, 2, 2], [3, 2, 1, 0]], good_len, _lib.E_INDEX),        # not a permutation
        ([[0, 1, 2, 7], [3, 2, 1, 0]], good_len, _lib.E_INDEX),        # out of range
        ([[1, 0, 2, 3], [3, 2, 1, 0]], good_len, _lib.E_INDEX),        # not sorted by descending length
        (good_order, [[3, 2, 1, 0], [1, 1, 2, 4]], _lib.E_SHAPE),      # a length of 0
        (good_order, [[12, 2, 1, 1], [1, 1, 2, 4]], _lib.E_SHAPE),     # a left context longer than L - 1
    ]
    for order, lengths, status in bad:
        assert _abi_call(lib, cfg, order, lengths) == status, lib.drin_last_error()
    assert _abi_call(lib, cfg, good_order, good_len, ws_bytes=16) == _lib.E_WORKSPACE
    for field, value, status in (("embed_dim", 18, _lib.E_SHAPE), ("mention_tokens", 1, _lib.E_SHAPE),
                                 ("precision", _lib.PREC_BF16X3_ALL, _lib.E_UNSUPPORTED), ("embed_dim", 1028, _lib.E_UNSUPPORTED)):
        old = getattr(cfg, field)
        setattr(cfg, field, value)
        assert lib.drin_melhi_workspace_bytes(C.byref(cfg), 1) == 0
        assert _abi_call(lib, cfg, good_order, good_len, ws_bytes=1 << 30) == status
        setattr(cfg, field, old)
    assert lib.drin_melhi_forward(C.byref(cfg), None, None, None, None, None, 0, None, None) == _lib.E_NULL


def test_shim_reads_the_wikidiverse_offline_files(tmp_path, monkeypatch):
    import sys
    import types
    from drin_amd import melhi_shim
    B, L, D, R, P, N = 3, TINY["L"], TINY["D"], TINY["R"], TINY["P"], TINY["N"]
    r = np.random.default_rng(0)
    for s in melhi_shim.SPLITS:
        np.save(tmp_path / f"mention-text-feature_{s}.npy", r.standard_normal((B, L, D), dtype=np.float32))
        np.save(tmp_path / f"mention-text-mask_{s}.npy", np.ones((B, L), dtype=np.int64))
        np.save(tmp_path / f"entity-attr-feature_{s}.npy", r.standard_normal((B * N, D), dtype=np.float32))
        np.save(tmp_path / f"start-pos_{s}.npy", np.array([0, 2, 4]))
        np.save(tmp_path / f"end-pos_{s}.npy", np.array([1, 3, 5]))
        np.save(tmp_path / f"answer_{s}.npy", np.array([0, 1, N - 1]))
        np.save(tmp_path / f"mention-image-feature_{s}.npy", r.standard_normal((B, P, R), dtype=np.float32))
        np.save(tmp_path / f"entity-image-feature_{s}.npy", r.standard_normal((B * N, R), dtype=np.float32))
    args = types.SimpleNamespace(dataset_name="wikidiverse", num_candidates_model=N, bert_embed_dim=D, resnet_embed_dim=R,
                                 max_mention_sentence_len=L, resnet_num_region=P, preprocess_dir=str(tmp_path), batch_size=2,
                                 shuffle_train_data=False)
    common = types.ModuleType("common")
    common.args = args
    monkeypatch.setitem(sys.modules, "common", common)
    monkeypatch.setitem(sys.modules, "common.args", args)
    train, valid, test = melhi_shim.create_datasets()
    batch = next(iter(valid))
    assert len(batch) == 9
    assert batch[0].shape == (2, L, D) and batch[4].shape == (2, P, R) and batch[5].shape == (2, N, D) and batch[7].shape == (2, N, R)
    assert batch[2].tolist() == [1, 3] and batch[3].tolist() == [2, 4]        # the CLS shift of baselines/data.py
    assert batch[8].shape == (2, N - 1) and batch[8][1].tolist()[1] == 1
    model = melhi_shim.Model()
    assert list(model.state_dict()) == KEYS
