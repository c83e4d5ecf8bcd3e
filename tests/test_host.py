"""CPU tests of the host logic around the path: loader, loss/metric, training-loop semantics."""
import json
import os

import numpy as np
import pytest
import torch

from drin_amd import synth
from drin_amd.config import DrinConfig, wikimel_config
from drin_amd.data import ShardSampler, create_datasets, write_synthetic_dataset
from drin_amd.metrics import TopkAccuracy, TripletLoss
from drin_amd.model import Model
from drin_amd.train import MELRunner, seed_everything
from oracle import drin_oracle as O
from oracle.cases import TINY
from tests.helpers import OracleModel

TINY_WD = DrinConfig(batch_size=4, **TINY)
TINY_WM = DrinConfig(dataset_name="wikimel", num_candidates_data=6, max_entity_attr_token_len=6, batch_size=4,
                     metrics_topk=(1, 3), acc_correction=(0.0, 0.0, 0.0), **TINY)


def test_config_defaults_follow_reference_args():
    wd, wm = DrinConfig(), wikimel_config()
    assert (wd.num_candidates_model, wm.num_candidates_model) == (11, 101)          # args.py:83,93,101
    assert wd.metrics_topk == (1, 3, 5) and wm.metrics_topk == (1, 5, 10, 20, 50)    # args.py:114,120
    assert wd.batch_size == wm.batch_size == 64 and wd.learning_rate == 1e-3 and wd.triplet_margin == 0.25
    assert abs(wd.acc_correction[0] - 2292 / 13205) < 1e-12
    DrinConfig(gcn_edge_feature="vector").validate()                                 # args.py:30 spelling "scaler" | "vector"
    with pytest.raises(ValueError):
        DrinConfig(gcn_edge_feature="scalar").validate()


def test_state_dict_contract():
    """24 tensors, reference key names and order, 7 875 072 parameters."""
    m = Model(DrinConfig())
    sd = m.state_dict()
    assert list(sd) == [k for k, _ in synth.STATE_DICT_SHAPES(768, 2048, 2)]
    assert [tuple(v.shape) for v in sd.values()] == [s for _, s in synth.STATE_DICT_SHAPES(768, 2048, 2)]
    assert sum(v.numel() for v in sd.values()) == 7_875_072
    # vector edges (model.py:112-116): w_m between w_h and w_u, half-width w_u / w_v
    cfg = DrinConfig(gcn_edge_feature="vector", **TINY)
    sd = Model(cfg).state_dict()
    want = synth.STATE_DICT_SHAPES(64, 128, 2, True)
    assert list(sd) == [k for k, _ in want] and [tuple(v.shape) for v in sd.values()] == [s for _, s in want]
    assert tuple(sd["gcn_layers.0.w_u.weight"].shape) == (32, 64) and "gcn_layers.1.w_m.bias" in sd


def test_model_refuses_to_run_without_gpu_tensors():
    m = Model(TINY_WD)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        m(synth.make_batch(TINY_WD, 2, 1))


@pytest.mark.parametrize("cfg", [TINY_WD, TINY_WM], ids=["wikidiverse", "wikimel"])
def test_loader_tuple_contract(tmp_path, cfg):
    write_synthetic_dataset(cfg, str(tmp_path), sizes=(10, 6, 5), seed=3, num_entities=40)
    train, valid, test = create_datasets(cfg.with_(shuffle_train_data=False), str(tmp_path))
    assert (len(train.dataset), len(valid.dataset), len(test.dataset)) == (10, 6, 5)
    batch = next(iter(train))
    assert len(batch) == 15
    B, N, D, R = 4, cfg.num_candidates_model, cfg.bert_embed_dim, cfg.resnet_embed_dim
    L, P = cfg.max_mention_sentence_len, cfg.resnet_num_region
    wm = cfg.token_level_entities
    T = cfg.max_entity_attr_token_len
    expect = [(B, L, D), (B, L), (B,), (B,), (B, P, R), (B, 3, 1, R), (B, 3),
              (B, N, T, D) if wm else (B, N, D), (B, N, T) if wm else (B,), (B, N, 1, R) if wm else (B, N, R),
              (B, N, 1, 1, R) if wm else (B, N, 1, R), (B, N, 1), (B, N), (B, N), (B, N - 1)]
    assert [tuple(t.shape) for t in batch] == expect
    assert batch[14].dtype == torch.uint8 and batch[2].dtype == torch.int64 and batch[0].dtype == torch.float32
    # +1 CLS shift (data.py:113-114) and the one-hot / all-zero answer rows (data.py:159-161)
    raw_start = np.load(tmp_path / "start-pos_train.npy")[:B]
    assert batch[2].tolist() == (raw_start + 1).tolist()
    ans = np.load(tmp_path / "answer_train.npy")[:B]
    for i, a in enumerate(ans):
        row = batch[14][i].numpy()
        assert row.sum() == (0 if a == N - 1 else 1) and (a == N - 1 or row[a] == 1)
    if wm:  # entity rows gathered through qid2idx (data.py:87-93)
        q2i = json.load(open(tmp_path / "qid2idx.json"))
        qids = np.load(tmp_path / "entity-name-raw_train.npy").reshape(-1, N)
        table = np.load(tmp_path / "entity-attr-feature.npy")
        rows = [q2i[q] for q in qids[1]]
        np.testing.assert_array_equal(batch[7][1].numpy(), table[rows])
    # the oracle accepts the collated tuple as is
    s = O.forward(synth.make_state_dict(cfg, 8), batch)
    assert s.shape == (B, N) and torch.isfinite(s).all()


def test_sharded_loaders_partition_the_split(tmp_path):
    write_synthetic_dataset(TINY_WD, str(tmp_path), sizes=(11, 4, 4), seed=5)
    seen, valid = [], []
    for r in range(2):
        loaders = create_datasets(TINY_WD, str(tmp_path), rank=r, world_size=2)
        seen.append(list(loaders[0].sampler))
        valid.append(list(loaders[1].sampler))
        assert len(loaders[0].sampler) == len(seen[-1]) and len(loaders[1].sampler) == len(valid[-1])
    # train: every mention is drawn, and the shards have ONE length (11 = 6 + 6 with one wrapped-around mention), so that
    # every rank runs the same number of steps - the per-step gradient all-reduce needs that
    assert len(seen[0]) == len(seen[1]) == 6 and set(seen[0] + seen[1]) == set(range(11))
    assert len(seen[0] + seen[1]) - len(set(seen[0] + seen[1])) == 1
    # evaluation: an exact partition - every mention counts once in the metrics
    assert sorted(valid[0] + valid[1]) == list(range(4)) and not set(valid[0]) & set(valid[1])
    odd = [list(ShardSampler(5, r, 2, False, 0)) for r in range(2)]
    assert sorted(odd[0] + odd[1]) == list(range(5)) and len(odd[0]) == 3 and len(odd[1]) == 2


def test_triplet_loss_matches_oracle_and_reference_vectors(golden_dir):
    g = np.load(os.path.join(golden_dir, "triplet.npz"))
    for i in range(3):
        y, yhat = torch.from_numpy(g[f"y{i}"]), torch.from_numpy(g[f"yhat{i}"])
        assert abs(TripletLoss(0.25)(y, yhat).item() - float(g[f"loss{i}"])) <= 1e-6


def test_topk_accuracy_semantics():
    yhat = torch.tensor([[0.9, 0.1, 0.5, 7.0], [0.2, 0.2, 0.1, 7.0], [0.3, 0.6, 0.1, 7.0]])
    y = torch.tensor([[0, 0, 1], [0, 1, 0], [0, 0, 0]], dtype=torch.uint8)
    m = TopkAccuracy(1)
    m.update(yhat, y)
    assert (int(m.correct), int(m.total)) == O.topk_counts(yhat, y, 1) == (1, 3)
    m.update(yhat, y)
    assert abs(float(m.compute()) - 2 / 6) < 1e-7
    m.reset()
    assert int(m.total) == 0


def test_training_loop_semantics(tmp_path):
    """config 1 plumbing on CPU: .npy -> loader -> loop.  Checks the Adam reset every interval
    (train.py:141-144), metric reset per epoch, and that the loss goes down on a learnable toy set."""
    cfg = TINY_WD.with_(num_epoch=4, test_epoch_interval=2, shuffle_train_data=False, learning_rate=1e-3)
    write_synthetic_dataset(cfg, str(tmp_path), sizes=(16, 8, 8), seed=2)
    seed_everything(cfg.seed)
    loaders = create_datasets(cfg, str(tmp_path))
    model = OracleModel(cfg)
    created = []
    orig = torch.optim.Adam

    class SpyAdam(orig):
        def __init__(self, *a, **k):
            created.append(self)
            super().__init__(*a, **k)

    torch.optim.Adam = SpyAdam
    try:
        hist = MELRunner(cfg, model, "cpu").fit(loaders)
    finally:
        torch.optim.Adam = orig
    assert len(created) == 2, "a new optimizer per test_epoch_interval round"
    assert len(hist.train) == 4 and len(hist.valid) == 4 and len(hist.test) == 2
    assert hist.train[-1].loss < hist.train[0].loss
    assert all(0 <= v <= 1 / (1 - cfg.acc_correction[0]) + 1e-6 for v in hist.train[-1].topk)
    # first epoch, first step reproduces the hand-written reference step on the same batch
    seed_everything(cfg.seed)
    ref = OracleModel(cfg)
    batch = next(iter(create_datasets(cfg, str(tmp_path))[0]))
    opt = torch.optim.Adam(ref.parameters(), lr=cfg.learning_rate)
    loss = O.triplet_loss(batch[-1], ref(batch[:-1]), cfg.triplet_margin)
    loss.backward()
    opt.step()
    seed_everything(cfg.seed)
    mine = OracleModel(cfg)
    r = MELRunner(cfg, mine, "cpu")
    opt2 = torch.optim.Adam(mine.parameters(), lr=cfg.learning_rate)
    opt2.zero_grad()
    l2 = r.forward_step(batch, 0)
    l2.backward()
    opt2.step()
    assert abs(l2.item() - loss.item()) < 1e-7
    for (k, a), (_, b) in zip(ref.state_dict().items(), mine.state_dict().items()):
        assert torch.allclose(a, b, atol=1e-7), k


def test_indexed_loader_matches_gathered_loader(tmp_path):
    """Table form: candidate rows + tables reproduce the gathered 15-tuple exactly."""
    from drin_amd.data import create_indexed_datasets, load_entity_table
    from drin_amd.model import IndexedBatch
    cfg = TINY_WM.with_(shuffle_train_data=False)
    write_synthetic_dataset(cfg, str(tmp_path), sizes=(8, 4, 4), seed=6, num_entities=25)
    full = next(iter(create_datasets(cfg, str(tmp_path))[0]))
    idx = next(iter(create_indexed_datasets(cfg, str(tmp_path))[0]))
    assert len(idx) == 11 and idx[7].dtype == torch.int64 and tuple(idx[7].shape) == (4, cfg.num_candidates_model)
    table = load_entity_table(cfg, str(tmp_path))
    rebuilt = IndexedBatch(idx[:7], table, idx[7], idx[8], idx[9]).gathered() + [idx[10]]
    assert len(rebuilt) == 15
    for a, b in zip(full, rebuilt):
        assert torch.equal(a, b)


def test_device_loss_metric_refuses_host_tensors():
    from drin_amd.metrics import DeviceLossMetric
    m = DeviceLossMetric(0.25, (1, 3), "cpu")
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        m(torch.zeros(2, 3, dtype=torch.uint8), torch.zeros(2, 4))


def test_device_split_yields_the_indexed_loader_batches(tmp_path):
    """`DeviceSplit` (a whole split resident on one device) iterates exactly the batches of a DataLoader over
    `IndexedMELData`: order, sharding over ranks, per-epoch shuffling, dtypes and values."""
    from drin_amd.data import create_device_splits, create_indexed_datasets, write_synthetic_dataset
    for shuffle in (False, True):
        cfg = DrinConfig(dataset_name="wikimel", num_candidates_data=6, max_entity_attr_token_len=6, batch_size=5,
                         shuffle_train_data=shuffle, bert_embed_dim=64, gcn_embed_dim=64, resnet_embed_dim=128,
                         max_mention_sentence_len=16, resnet_num_region=4)
        root = tmp_path / f"s{int(shuffle)}"
        root.mkdir()
        write_synthetic_dataset(cfg, str(root), sizes=(13, 4, 4), seed=4, num_entities=30)
        for world, rank in ((1, 0), (2, 1)):
            ref = create_indexed_datasets(cfg, str(root), rank=rank, world_size=world)
            got = create_device_splits(cfg, str(root), "cpu", rank=rank, world_size=world)
            for epoch in (0, 1):
                for la, lb in zip(ref, got):
                    for ld in (la, lb):
                        if hasattr(ld.sampler, "set_epoch"):
                            ld.sampler.set_epoch(epoch)
                    assert len(la) == len(lb)
                    for ba, bb in zip(la, lb):
                        assert len(ba) == len(bb) == 11
                        for x, y in zip(ba, bb):
                            assert x.dtype == y.dtype and torch.equal(x, y)
    # WikiDiverse layout: the per-mention candidate tensors themselves live on the device, batches are the 15-tuples
    from drin_amd.data import create_datasets
    cfg = DrinConfig(num_candidates_data=6, batch_size=5, shuffle_train_data=True, bert_embed_dim=64, gcn_embed_dim=64,
                     resnet_embed_dim=128, max_mention_sentence_len=16, resnet_num_region=4)
    root = tmp_path / "wd"
    root.mkdir()
    write_synthetic_dataset(cfg, str(root), sizes=(13, 4, 4), seed=4)
    for world, rank in ((1, 0), (2, 0)):
        for la, lb in zip(create_datasets(cfg, str(root), rank=rank, world_size=world),
                          create_device_splits(cfg, str(root), "cpu", rank=rank, world_size=world)):
            assert len(la) == len(lb)
            for ba, bb in zip(la, lb):
                assert len(ba) == len(bb) == 15
                for x, y in zip(ba, bb):
                    assert x.dtype == y.dtype and torch.equal(x, y)


def test_shard_sampler_properties():
    """For any split size, world size and epoch: padded shards have ONE length and together cover every index (a rank never
    waits in a per-step collective for a rank that has run out of batches); unpadded shards partition the split exactly."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=200, deadline=None)
    @given(n=st.integers(0, 300), world=st.integers(1, 9), shuffle=st.booleans(), epoch=st.integers(0, 5))
    def check(n, world, shuffle, epoch):
        padded, exact = [], []
        for r in range(world):
            a, b = ShardSampler(n, r, world, shuffle, 0, pad=True), ShardSampler(n, r, world, shuffle, 0)
            a.set_epoch(epoch)
            b.set_epoch(epoch)
            padded.append(list(a))
            exact.append(list(b))
            assert len(a) == len(padded[-1]) and len(b) == len(exact[-1])
        assert len({len(p) for p in padded}) == 1
        assert set(sum(padded, [])) == set(range(n)) and len(sum(padded, [])) - n < world
        assert sorted(sum(exact, [])) == list(range(n))

    check()


def test_step_profiler_follows_the_reference_schedule(tmp_path, monkeypatch):
    """`StepProfiler` = `torch.profiler.schedule(wait=1, warmup=1, active=3, repeat=2)` of `train.py:64-70` over the
    library's profiler: per fit, two cycles of (skip 1, run 1, time 3); an epoch that ends inside a cycle reports what it has."""
    import json
    from drin_amd import _lib
    from drin_amd.train import StepProfiler
    calls = []
    monkeypatch.setattr(_lib, "profile_begin", lambda n: calls.append("begin"))
    monkeypatch.setattr(_lib, "profile_end", lambda: (calls.append("end") or {"gemm": (3.0, 12), "optim": (0.375, 3), "edge": (0.0, 0)}))
    prof = StepProfiler(out_dir=str(tmp_path))
    prof.start()
    opened_at = []
    for step in range(14):
        if prof.open:
            opened_at.append(step)
        prof.step()
    prof.stop()
    assert opened_at == [2, 3, 4, 7, 8, 9] and calls == ["begin", "end", "begin", "end"]
    rep = json.load(open(tmp_path / "drin_profile_1.json"))
    assert rep["steps"] == 3 and rep["kernel_ms_per_step"] == {"gemm": 1.0, "optim": 0.125} and rep["launches_per_step"]["gemm"] == 4
    short = StepProfiler(out_dir=str(tmp_path / "short"))
    short.start()
    for _ in range(3):
        short.step()
    short.stop()                                        # the epoch ended after one timed step
    assert short.reports[0]["steps"] == 1 and not short.open


def test_no_kernel_uses_scratch():
    """no kernel of the gfx950 code objects may spill to scratch memory (`.private_segment_fixed_size` /
    `.vgpr_spill_count` of the AMDGPU metadata notes; round 2 shipped `k_entity_stream<3, 8, tokens, guarded, bf16>` with 26
    spilled VGPRs).  Reads the objects `python -m drin_amd.build` leaves under csrc/build - no GPU."""
    from drin_amd import build, resources
    build.build(verbose=False)
    rows = resources.kernel_resources()
    names = " ".join(k["name"] for k in rows)
    for must in ("k_entity_stream", "k_gemm_bf16x3", "k_gemm_x3_planes", "k_gemm_tn_bf16x3", "k_gemm_f32", "k_pair_layer1", "k_pair_final",
                 "k_cached_pairs", "k_slice_sum", "k_layernorm_gelu_bwd"):
        assert must in names, f"{must} not found in the code objects"
    assert len(rows) >= 90
    bad = [(k["name"], k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0)) for k in rows
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)]
    assert not bad, f"kernels with scratch / spilled VGPRs: {bad}"
    assert all(k.get("vgpr_count", 0) <= 256 for k in rows)


def test_untracked_loads_are_not_touched_before_their_counted_wait():
    """`k_gemm_bf16x3_p4` fetches its fp32 A units by inline-asm `global_load_dwordx4` whose data lands
    behind a hand-counted `s_waitcnt vmcnt(4)`; the compiler believes the registers defined at the asm statement.  The
    generated gfx950 ISA is checked instead of trusted: no instruction between a vector-memory load and the wait that retires
    it may read or write the load's destination registers (layout order + every loop body a second time).  The same walk
    over the other hand-pipelined kernels, and over a synthetic sequence with exactly that slip, which it must flag."""
    from drin_amd import build, resources
    build.build(verbose=False)
    for obj, kernel, min_insns in (("gemm_x3_planes.o", "k_gemm_bf16x3_p4", 1000), ("gemm_x3_planes.o", "k_gemm_x3_planes_p4ILb1ELb0E", 800),
                                   ("gemm_x3_planes.o", "k_gemm_x3_planes_p4ILb0ELb0E", 800),
                                   ("gemm_x3_planes.o", "k_gemm_x3_planes_p4ILb1ELb1E", 600),                     # one fp16 pass on single planes
                                   ("gemm_bf16x3.o", "k_gemm_bf16x3ILi256ELi256ELi2ELi4ELb1E", 1000), ("gemm_tn_bf16x3.o", "k_gemm_tn", 500),
                                   ("fused_kernels.o", "k_entity_stream", 1000), ("entity_cache.o", "k_cached_pairs", 1000)):
        isa = resources.kernel_isa(obj, kernel)
        assert len(isa) >= min_insns, (obj, kernel, len(isa))
        assert any(t.startswith("v_mfma") for _a, t, _b in isa) or "gemm" not in kernel
        hazards = resources.untracked_load_hazards(isa)
        assert not hazards, f"{kernel}: {hazards[:4]}"
    p4 = resources.kernel_isa("gemm_x3_planes.o", "k_gemm_bf16x3_p4")
    loops = [(a, b) for a, _t, b in p4 if b is not None and b <= a]
    mfmas = lambda ab: sum(t.startswith("v_mfma") for a, t, _b in p4 if ab[1] <= a <= ab[0])   # noqa: E731
    main = max(loops, key=mfmas)                                          # the K loop: four phases of counted waits
    body = [t for a, t, _b in p4 if main[1] <= a <= main[0]]
    assert sum(t.startswith("s_waitcnt vmcnt(4)") for t in body) == 4 and sum(t == "s_barrier" for t in body) == 8
    assert sum(t.startswith("global_load_dwordx4") for t in body) == 4 and sum(t.startswith("global_load_lds_dwordx4") for t in body) == 4
    assert sum(t.startswith("v_mfma_f32_16x16x32_bf16") for t in body) == 96
    # the single-plane fp16 instantiation (round 5): the same four counted waits and eight barriers per K-block (64 wide), all DMA,
    # 16 fp16 MFMAs per phase
    f16 = resources.kernel_isa("gemm_x3_planes.o", "k_gemm_x3_planes_p4ILb1ELb1E")
    loops = [(a, b) for a, _t, b in f16 if b is not None and b <= a]
    mfmas16 = lambda ab: sum(t.startswith("v_mfma") for a, t, _b in f16 if ab[1] <= a <= ab[0])   # noqa: E731
    main = max(loops, key=mfmas16)
    body = [t for a, t, _b in f16 if main[1] <= a <= main[0]]
    assert sum(t.startswith("s_waitcnt vmcnt(4)") for t in body) == 4 and sum(t == "s_barrier" for t in body) == 8
    assert sum(t.startswith("global_load_lds_dwordx4") for t in body) == 8 and not any(t.startswith("global_load_dwordx4") for t in body)
    assert sum(t.startswith("v_mfma_f32_16x16x32_f16") for t in body) == 64 and not any(t.startswith("v_mfma_f32_16x16x32_bf16") for t in body)
    fake = [(0, "global_load_dwordx4 v[6:9], v[162:163], off", None), (8, "global_load_lds_dwordx4 v[10:11], off", None),
            (16, "s_waitcnt vmcnt(1)", None), (20, "v_mov_b32_e32 v20, v6", None),          # retired: fine
            (24, "global_load_dwordx4 v[6:9], v[162:163], off", None), (32, "v_mov_b32_e32 v21, v7", None),   # copied too early
            (36, "s_waitcnt vmcnt(0)", None), (40, "v_mov_b32_e32 v21, v7", None)]
    assert len(resources.untracked_load_hazards(fake)) == 1
    # an if / else the compiler lays out as load | s_branch over | mov into the same registers is NOT a hazard (two paths) ...
    ifelse = [(0, "s_cbranch_scc1 5", 16), (4, "global_load_dwordx2 v[4:5], v[2:3], off", None), (12, "s_branch 1", 20),
              (16, "v_mov_b64_e32 v[4:5], v[12:13]", None), (20, "s_waitcnt vmcnt(0)", None), (24, "v_add_u32_e32 v6, v4, v5", None)]
    assert not resources.untracked_load_hazards(ifelse)



def test_design_md_quotes_what_its_tracked_files_say():
    """DESIGN.md quoted best-box numbers while citing tracked files that said otherwise.  Every measured figure there now
    carries a tag naming the file and the field it comes from; the figure and the file must agree to 3 %, and the tag must sit on the
    line that shows the number (tools/check_design_numbers.py).  Also: the checker itself flags a wrong figure and a misplaced tag."""
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_design_numbers", os.path.join(repo, "tools", "check_design_numbers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, problems = mod.check(os.path.join(repo, "DESIGN.md"))
    assert n >= 30 and not problems, problems
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        doc = os.path.join(d, "doc.md")
        ok = "stream 8.269 ms <!--track csv profiles/r5_wikimel_b4096_kernel_stats.csv k_entity_stream AverageNs 8.269-->\n"
        wrong = "stream 7.5 ms <!--track csv profiles/r5_wikimel_b4096_kernel_stats.csv k_entity_stream AverageNs 7.5-->\n"
        apart = "stream is fast <!--track csv profiles/r5_wikimel_b4096_kernel_stats.csv k_entity_stream AverageNs 8.269-->\n"
        missing = "x 1.0 <!--track json profiles/no_such_file.json value 1.0-->\n"
        for text, bad in ((ok, 0), (wrong, 1), (apart, 1), (missing, 1)):
            with open(doc, "w") as f:
                f.write(text)
            assert len(mod.check(doc)[1]) == bad, (text, mod.check(doc))


# ---- round 6: host logic of the index report, the cache-format criterion, the exported contraction gate --------------------------
def _cpu_table(rows=50, scale_row=None, factor=1.0):
    from drin_amd.model import EntityTable
    g = torch.Generator().manual_seed(2)
    img = torch.randn(rows, 1, 64, generator=g)
    if scale_row is not None:
        img[scale_row] *= factor
    return EntityTable(torch.randn(rows, 4, 16, generator=g), torch.ones(rows, 4, dtype=torch.int64), img,
                       torch.randn(rows, 1, 64, generator=g), torch.rand(rows, 1, generator=g)), img


def test_mixed_f16_cache_format_is_used_only_inside_its_scale_criterion():
    """`EntityTable.enable_cache(format="mixed_f16")`: one scan of the image table per table VERSION; a row more than
    MIXED_F16_MAX_ROW_RATIO (8) x the median row's magnitude makes the table fall back to fp32 rows, with a warning saying so;
    `force=True` keeps the fp16 fields (and still says what it found); a table inside the criterion is silent."""
    import warnings
    t, img = _cpu_table()
    t.enable_cache(True, format="mixed_f16")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert t._effective_cache_format() == "mixed_f16"
    img[7] *= 20.0                                                   # in place: the version counter moves, the next build rescans
    with pytest.warns(UserWarning, match="1 of 50 entity image rows.*gets fp32 cache rows"):
        assert t._effective_cache_format() == "f32"
    scans = []
    orig = torch.Tensor.amax
    try:
        torch.Tensor.amax = lambda self, *a, **k: (scans.append(1), orig(self, *a, **k))[1]
        with pytest.warns(UserWarning):
            t._effective_cache_format()                              # same table version: no second pass over the table
    finally:
        torch.Tensor.amax = orig
    assert not scans
    t.enable_cache(True, format="mixed_f16", force=True)
    with pytest.warns(UserWarning, match=r"mixed_f16 \(forced\): 1 of 50"):
        assert t._effective_cache_format() == "mixed_f16"
    img[7] /= 20.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert t._effective_cache_format() == "mixed_f16"
    t.enable_cache(True, format="f32")
    assert t._effective_cache_format() == "f32"
    with pytest.raises(ValueError):
        t.enable_cache(True, format="fp8")


def test_index_report_words_become_an_index_error():
    """`Model.check_indices`: the four status words the kernels leave (`drin_batch.index_status`: flag, pair, value low / high) raise
    IndexError naming row and pair - a negative row too - and are cleared; clean words raise nothing."""
    m = Model(TINY_WD)
    dev = torch.device("cpu")
    words = m._status_words(dev)
    assert words.dtype == torch.int32 and words.tolist() == [0, 0, 0, 0]
    m.check_indices()
    words.copy_(torch.tensor([1, 205, -4, -1], dtype=torch.int32))                # row -4 at pair 205
    with pytest.raises(IndexError, match=r"row -4 at pair 205 .*drin/data.py:87-93"):
        m.check_indices()
    assert words.tolist() == [0, 0, 0, 0]
    words.copy_(torch.tensor([1, 7, 1001, 0], dtype=torch.int32))
    with pytest.raises(IndexError, match="row 1001 at pair 7"):
        m.check_indices()
    words[0] = 1                                                                  # the training paths report the flag alone
    with pytest.raises(IndexError, match="a row of a training batch"):
        m.check_indices()
    m.check_indices()


def test_library_reports_how_it_runs_the_image_contraction():
    """`drin_image_contraction_passes`: the library's own gate for the one-pass fp16 contraction (host-side, no launch)."""
    import ctypes as C
    from drin_amd import _lib
    lib = _lib.load()
    c = _lib.DrinConfigC()
    _lib.check(lib.drin_default_config(C.byref(c)))
    c.batch, c.num_candidates, c.embed_dim, c.image_dim, c.entity_tokens = 4096, 101, 768, 2048, 64
    for prec, feat, indexed, want in ((_lib.PREC_F32, _lib.FEAT_F32, 0, 0), (_lib.PREC_BF16X3, _lib.FEAT_F32, 0, 3),
                                      (_lib.PREC_BF16X3, _lib.FEAT_BF16, 0, 2), (_lib.PREC_BF16X3_IF16, _lib.FEAT_F32, 0, 1),
                                      (_lib.PREC_BF16X3_IF16, _lib.FEAT_F32, 1, 3), (_lib.PREC_BF16X3_IF16, _lib.FEAT_BF16, 0, 2)):
        c.precision, c.feature_dtype = prec, feat
        assert lib.drin_image_contraction_passes(C.byref(c), indexed) == want, (prec, feat, indexed)
    c.precision, c.feature_dtype, c.num_candidates = _lib.PREC_BF16X3_IF16, _lib.FEAT_F32, 11          # short lists: split-bf16
    assert lib.drin_image_contraction_passes(C.byref(c), 0) == 3
    c.num_candidates, c.batch = 101, 64                                                                 # fewer than 128 tiles
    assert lib.drin_image_contraction_passes(C.byref(c), 0) == 3
    assert lib.drin_index_status(None, None) == _lib.E_NULL


def test_library_says_which_configs_train_in_table_form():
    """`drin_indexed_supported` one step either side of every bound of the table form of the layer-by-layer entry points
    (host-side, no launch).  Expected values read off `indexed_supported` in csrc/api.hip."""
    import ctypes as C
    from drin_amd import _lib
    lib = _lib.load()
    OK, NO = _lib.OK, _lib.E_UNSUPPORTED
    base = dict(batch=11, num_candidates=101, embed_dim=128, image_dim=128, entity_objects=1, entity_image_inner=1,
                entity_object_inner=1, vector_edges=0, precision=_lib.PREC_BF16X3, num_entities=64, entity_tokens=0)
    for change, want in (
            (dict(), OK),
            (dict(batch=341, num_candidates=3), NO), (dict(batch=1024, num_candidates=1), OK),      # 1023 / 1024 pairs
            (dict(embed_dim=96), NO), (dict(embed_dim=144), NO), (dict(embed_dim=160), OK),       # D >= 128, a multiple of 32
            (dict(image_dim=96), NO), (dict(image_dim=2048), OK), (dict(image_dim=2080), NO),     # 128 <= R <= 2048
            (dict(image_dim=144), NO),
            (dict(batch=65535), OK), (dict(batch=65536), NO),
            (dict(entity_objects=2), NO),
            (dict(entity_image_inner=0), OK), (dict(entity_image_inner=2), NO),
            (dict(entity_object_inner=0), OK), (dict(entity_object_inner=2), NO),
            (dict(vector_edges=1), NO),
            (dict(precision=_lib.PREC_F32), NO), (dict(precision=_lib.PREC_BF16X3_ALL), OK),
            (dict(precision=_lib.PREC_BF16X3_IF16), NO),
            (dict(num_entities=0), NO), (dict(entity_tokens=8), NO)):
        c = _lib.DrinConfigC()
        _lib.check(lib.drin_default_config(C.byref(c)))
        for k, v in {**base, **change}.items():
            setattr(c, k, v)
        assert lib.drin_indexed_supported(C.byref(c)) == want, change
        if want == NO:
            assert b"drin_indexed_supported: entity_index needs pooled entity text tables" in lib.drin_last_error(), change
    assert lib.drin_indexed_supported(None) == _lib.E_NULL
    c.precision = 2                                                    # not a drin_precision: validate_config speaks first
    assert lib.drin_indexed_supported(C.byref(c)) == NO and b"precision 2" in lib.drin_last_error()
