"""Test-only helpers.  `OracleModel` has the product's parameter tree (so state_dicts interchange) but
computes its forward with the CPU oracle - it exists so that the loader / training loop / data-parallel
plumbing can be exercised on a machine without a GPU.  Never imported by the product."""
import torch

from drin_amd.config import DrinConfig
from drin_amd.model import Model
from oracle import drin_oracle as O


class OracleModel(Model):
    def forward(self, batch):
        p = dict(self.named_parameters())
        cfg: DrinConfig = self.cfg
        return O.forward(p, batch, num_layers=cfg.num_gcn_layers, edge_enabled=cfg.gcn_edge_enabled,
                         dynamic=cfg.gcn_edge_type == "dynamic", vector=cfg.gcn_edge_feature == "vector",
                         vertex_activation=cfg.gcn_vertex_activation, edge_activation=cfg.gcn_edge_activation)


# ---- the every-path check of one configuration (tests/test_gpu_fuzz.py, tests/test_gpu_width_bands.py) ----------------------------
class _relu_spy:
    """Wraps `F.relu` inside the block (the oracle resolves activations by name at call time, `model.py:117-118`).
    Recording: `near` lists every relu INPUT ELEMENT closer to the kink than `thr` - as (call number, flat index, value) - EXACT
    ZEROS EXCLUDED (a masked or zero-padded input is zero on every path, and relu'(0) = 0 is torch's convention the kernels must
    follow: nothing to excuse there).  Replaying with `flip`: the listed elements keep their VALUE but take the derivative of the
    other side of the kink (x > 0: derivative 0; x < 0: derivative 1) - the gradient the case has if the arithmetic of the path
    under test put those pre-activations on the other side."""

    def __init__(self, thr: float, flip=()):
        self.thr, self.near, self.calls = thr, [], 0
        self.flip = {}
        for c, j in flip:
            self.flip.setdefault(c, []).append(j)

    def __enter__(self):
        import torch.nn.functional as F
        self._F, self._orig = F, F.relu

        def spy(x, *a, **k):
            c, self.calls = self.calls, self.calls + 1
            xd = x.detach()
            close = (xd.abs() < self.thr) & (xd != 0)
            if bool(close.any()):
                flat = xd.reshape(-1)
                self.near += [(c, int(j), float(flat[j])) for j in close.reshape(-1).nonzero().flatten().tolist()]
            out = self._orig(x, *a, **k)
            if c in self.flip:
                sel = torch.zeros(x.numel(), dtype=torch.bool)
                sel[torch.tensor(self.flip[c])] = True
                sel = sel.view(x.shape)
                out = torch.where(sel & (xd > 0), xd, out)               # value kept, derivative 0
                out = torch.where(sel & (xd < 0), out + (x - xd), out)   # value 0, derivative 1
            return out
        F.relu = spy
        return self

    def __exit__(self, *exc):
        self._F.relu = self._orig
        return False


def every_path_against_the_oracle(cfg, B, precision, seed, label, weights_seed=None, index_seed=None, table_refusal=None,
                                  cached_refusal=None, same_bits=False):
    """Every path the product offers for `cfg` against the CPU oracle on the same inputs: inference (the folded path where it
    applies, else layer by layer), the training-mode forward, the parameter gradients of the caller's loss against fp64 autograd
    through the oracle (the conditioning yardstick, the bounded relu excuse, WHICH gradients are None), the table form and the
    per-entity cache in both row formats.  `seed` draws the batch and the entity table, `weights_seed` the parameters and
    `index_seed` the candidate rows (both default to `seed`); `label` names the case in every message and in the printed line.
    `table_refusal` / `cached_refusal`: a regular expression - the table form without a cache / the per-entity cache in both row
    formats is then EXPECTED to refuse the call with the library's own error of that text (split-bf16 precision at a width that
    is no multiple of 32) instead of scoring: a route scores inside its bar or says why it does not, nothing else.
    `same_bits`: every inference route (gathered batch, table form, each cache format) is scored a second time and must return
    the same bits.
    Returns what it measured and built: {"inference", "training", "table", "cache": {format: error}, "model", "batch"}."""
    import pytest
    from drin_amd import _lib, synth
    from drin_amd.metrics import TripletLoss
    from drin_amd.model import EntityTable, IndexedBatch
    DEV = "cuda"
    weights_seed = seed if weights_seed is None else weights_seed
    index_seed = seed if index_seed is None else index_seed
    sd = synth.make_state_dict(cfg, weights_seed)
    T = cfg.max_entity_attr_token_len
    batch = synth.make_batch(cfg, B, seed % 100000, min_span=1, max_span=3, min_tokens=min(3, T))
    if cfg.token_level_entities and T >= 3:
        # Python-slice corners of the token mean: an entity with every token (ntok = T) and one with exactly one kept token
        batch[8][0, 0, :] = 1
        batch[8][-1, -1, :] = 0
        batch[8][-1, -1, :3] = 1
    ref_p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.forward(ref_p, batch[:14], **O.config_kwargs(cfg))
    tol = 2e-5 if precision == "bf16x3_all" else 1e-5
    finite = torch.isfinite(ref)
    assert finite.all(), f"case {label}: a degenerate draw - the oracle's scores are not all finite, the comparison would be partly vacuous"
    model = Model(cfg, precision=precision).to(DEV)
    model.load_state_dict(sd)
    dbatch = [t.to(DEV) for t in batch]

    def check(got, what):
        got = got.detach().cpu()
        assert got.shape == ref.shape, what
        assert torch.equal(torch.isnan(got), torch.isnan(ref.detach())), f"case {label} {what}: NaN pattern differs ({cfg})"
        err = (got - ref.detach())[finite].abs().max().item()
        assert err <= tol, f"case {label} {what}: {err:.2e} > {tol} ({cfg}, B={B}, {precision})"
        return err

    model.eval()
    with torch.no_grad():
        first = model(dbatch[:14])
        e_inf = check(first, "inference")
        if same_bits:
            assert torch.equal(first, model(dbatch[:14])), f"case {label} inference: a second run gives other bits"
    model.train()
    out = model(dbatch[:14])
    e_trn = check(out, "training forward")
    # gradients of the caller's loss (train.py:33-34, common/utils.py:26-43)
    if finite.all():
        if cfg.num_candidates_data == 0:      # a lone answer slot: the triplet loss has no column left (utils.py:36-37); any functional does
            w = torch.linspace(-1.0, 1.0, B)[:, None]
            loss, ref_loss = (out * w.to(DEV)).sum(), (ref * w).sum()
        else:
            loss = TripletLoss(cfg.triplet_margin)(dbatch[14], out)
            ref_loss = O.triplet_loss(batch[14], ref, cfg.triplet_margin)
        loss.backward()
        ref_g = torch.autograd.grad(ref_loss, list(ref_p.values()), allow_unused=True)
        # the yardstick is the oracle in fp64; how far the fp32 ORACLE's own gradient is from it measures the conditioning of the
        # case (a sigmoid vertex activation squeezes all scores into a 2e-4 band: the fp32 oracle is then 7e-4 from the fp64
        # one - tools/probes/fuzz_grad_case.py, profiles/r4_fuzz_grad_cases.txt) and scales the bound; a relu vertex meets its
        # kink: a split-bf16 product moves a pre-activation by 1e-6 and one element in ten thousand flips its derivative
        # relu has no derivative at 0: a pre-activation closer to it than the arithmetic resolves (split-bf16 moves a mention-sized
        # pre-activation by up to ~5e-6, exact fp32 by ~1e-7) may sit on either side, and ONE flipped unit of a last-layer MENTION
        # vertex - which all N scores of its mention share - moved a LayerNorm bias gradient by 15 % (seed 349 of a 640-seed sweep:
        # min |z| 4.6e-6, relu vertices 0.147, the same case with gelu 1.1e-5; tools/probes/fuzz_case_diff.py).  What may be
        # excused is BOUNDED: only relu input ELEMENTS within that resolution of the kink count (exact zeros - masked
        # or padded inputs - never do), and a mismatching case passes only if ALL its gradients agree, to the same bound, with the
        # fp64 oracle re-run with the derivative of some subset of exactly those elements flipped; anything else fails.
        thr = 2e-5 if precision == "bf16x3_all" else 1e-6
        w64 = w.double() if cfg.num_candidates_data == 0 else None

        def grads64(flip=()):
            p64 = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
            with _relu_spy(thr, flip) as spy:
                out64 = O.forward(p64, batch[:14], dtype=torch.float64, **O.config_kwargs(cfg))
            loss64 = (out64 * w64).sum() if w64 is not None else O.triplet_loss(batch[14].double(), out64, cfg.triplet_margin)
            return torch.autograd.grad(loss64, list(p64.values()), allow_unused=True), spy.near

        g64, near = grads64()
        assert abs(loss.item() - ref_loss.item()) <= 2e-5
        base = 5e-4 if precision == "bf16x3_all" else 5e-5
        if cfg.gcn_vertex_activation == "relu" and precision == "bf16x3_all":
            base *= 4
        named = list(model.named_parameters())
        conds = {}
        for (k, p), r, r64 in zip(named, ref_g, g64):
            assert k in ref_p
            assert (p.grad is None) == (r is None), f"case {label}: grad of {k} is {'None' if p.grad is None else 'set'}, reference {'None' if r is None else 'set'} ({cfg})"
            if r is not None and r64.norm().item() > 1e-10:
                conds[k] = (r.double() - r64).norm().item() / r64.norm().item()          # the fp32 oracle's own distance

        def mismatches_against(yardstick):
            out_ = []
            for (k, p), r64 in zip(named, yardstick):
                if k not in conds or r64 is None or r64.norm().item() <= 1e-10:
                    continue
                rel = (p.grad.cpu().double() - r64).norm().item() / r64.norm().item()
                # (5 x: the fp32 oracle's distance is ONE sample of the case's conditioning, the library's another; sigmoid vertices
                #  squeeze all scores into a band of 4e-5 .. 2e-4, where a 1 400-seed sweep saw the two samples 3.5 x and 5.5 x apart:
                #  profiles/r5_fuzz_deep_sweep.txt)
                if rel > max(base, (10 if cfg.gcn_vertex_activation == "sigmoid" else 5) * conds[k]):
                    out_.append(f"case {label}: grad of {k} off by {rel:.2e} (fp32 oracle itself: {conds[k]:.2e}) ({cfg}, B={B}, {precision})")
            return out_

        mismatches = mismatches_against(g64)
        if mismatches and near:
            import itertools
            units = [(c, j) for c, j, _v in near]
            if len(units) <= 4:
                subsets = [s_ for n_ in range(1, len(units) + 1) for s_ in itertools.combinations(units, n_)]
            else:                                                      # many elements that close: each alone, then all of them
                subsets = [(u,) for u in units[:15]] + [tuple(units)]
            excused = next((s_ for s_ in subsets if not mismatches_against(grads64(s_)[0])), None)
            assert excused is not None, (f"{mismatches[0]} - and no flip of the {len(units)} relu input(s) within {thr:g} of the kink "
                                         f"({[f'{v:.1e}' for _c, _j, v in near][:6]}) explains it")
            print(f"case {label}: {len(mismatches)} gradient(s) differ from the fp64 oracle's and ALL agree with the fp64 oracle whose relu derivative "
                  f"is flipped at {len(excused)} of the {len(units)} input(s) within {thr:g} of the kink - no gradient is defined there at this "
                  f"precision: {mismatches[0][:140]}")
        else:
            assert not mismatches, mismatches[0]
    # table form + per-entity cache (inference; the library says so when a geometry has no table form)
    model.eval()
    e_tab = e_cache = None
    cache_errs = {}
    if cfg.num_gcn_layers == 2 and cfg.gcn_edge_feature == "scaler" and cfg.num_candidates_data >= 1:
        N, E = cfg.num_candidates_model, 23
        tab = synth.make_batch(cfg.with_(num_candidates_data=E - 1), 1, seed % 1000 + 7)
        table = EntityTable(tab[7][0], tab[8][0] if cfg.token_level_entities else None, tab[9][0], tab[10][0], tab[11][0]).to(DEV)
        cand = torch.randint(0, E, (B, N), generator=torch.Generator().manual_seed(index_seed)).to(DEV)
        ib = IndexedBatch(dbatch[:7], table, cand, dbatch[12], dbatch[13])
        ref_t = O.forward(sd, [t.cpu() for t in ib.gathered()], **O.config_kwargs(cfg))
        fin_t = torch.isfinite(ref_t)
        assert fin_t.all(), f"case {label}: table-form oracle scores not all finite"
        with torch.no_grad():
            for fmt in (None, "f32", "mixed_f16"):
                if fmt == "mixed_f16" and (cfg.gcn_embed_dim % 8 or cfg.resnet_embed_dim % 8):
                    continue
                table.enable_cache(fmt is not None, format=fmt or "f32")
                refusal = table_refusal if fmt is None else cached_refusal
                if refusal is not None:
                    with pytest.raises(_lib.DrinError, match=refusal):
                        model(ib)
                    e_tab, e_cache = ("refused", e_cache) if fmt is None else (e_tab, "refused")
                    if fmt is not None:
                        cache_errs[fmt] = "refused"
                    continue
                got = model(ib).cpu()
                if same_bits:
                    assert torch.equal(got, model(ib).cpu()), f"case {label} table form (cache {fmt}): a second run gives other bits"
                assert torch.equal(torch.isnan(got), torch.isnan(ref_t)), f"case {label} table form ({fmt}): NaN pattern"
                err = (got - ref_t)[fin_t].abs().max().item()
                # (mixed rows at D = 64: the fp16 operands' rounding is averaged over 64 columns only)
                assert err <= ((3e-5 if cfg.gcn_embed_dim < 256 else tol) if fmt == "mixed_f16" else tol), f"case {label} table form (cache {fmt}): {err:.2e} ({cfg}, B={B}, {precision})"
                e_tab, e_cache = (err, e_cache) if fmt is None else (e_tab, err)
                if fmt is not None:
                    cache_errs[fmt] = err
        table.enable_cache(False)
    print(f"case {label}: {cfg.dataset_name} N={cfg.num_candidates_model} D={cfg.gcn_embed_dim} R={cfg.resnet_embed_dim} L={cfg.num_gcn_layers} "
          f"{cfg.gcn_edge_type}/{cfg.gcn_edge_feature} {cfg.gcn_vertex_activation}/{cfg.gcn_edge_activation} mask={cfg.gcn_edge_enabled} "
          f"Km={cfg.object_topk_mention} Ke={cfg.object_topk_entity} T={T} B={B} {precision}: inference {e_inf:.1e} training {e_trn:.1e} "
          f"table {e_tab} cache {e_cache}")
    return {"inference": e_inf, "training": e_trn, "table": e_tab, "cache": cache_errs, "model": model, "batch": dbatch}


# ---- which width form the library takes for a geometry (drin_width_class) -----------------------------------------------------------
def config_c(D, R, cache_format="f32", vertex_activation="gelu", **fields):
    """A default `drin_config` (two layers, dynamic scalar edges) of 3 mentions x 6 candidates at embed_dim D / image_dim R."""
    import ctypes as C
    from drin_amd import _lib
    c = _lib.DrinConfigC()
    _lib.check(_lib.load().drin_default_config(C.byref(c)))
    c.batch, c.num_candidates, c.embed_dim, c.image_dim = 3, 6, D, R
    c.cache_format = _lib.CACHE_FORMATS[cache_format]
    c.vertex_activation = _lib.ACTIVATIONS[vertex_activation]
    for k, v in fields.items():   # (any field by its C name, raw values: an invalid one too)
        setattr(c, k, v)
    return c


def width_class(D, R, family, cache_format="f32", vertex_activation="gelu", **fields):
    """`drin_width_class` for `config_c(...)`: the band's name ("not-built", "tiny", "guarded", "exact"), V for the family
    "ln_backward", or the negative status.  Host-only: no device is touched."""
    import ctypes as C
    from drin_amd import _lib
    got = _lib.load().drin_width_class(C.byref(config_c(D, R, cache_format, vertex_activation, **fields)), _lib.WIDTH_FAMILIES[family])
    return got if got < 0 or family == "ln_backward" else _lib.WIDTH_BANDS[got]


def width_classes(cfg, cache_format="f32"):
    """{family: band} of a `DrinConfig` (its widths, vertex activation, layer count and edge feature), for `cache_format` rows."""
    from drin_amd import _lib
    return {f: width_class(cfg.gcn_embed_dim, cfg.resnet_embed_dim, f, cache_format, cfg.gcn_vertex_activation,
                           num_layers=cfg.num_gcn_layers, vector_edges=1 if cfg.gcn_edge_feature == "vector" else 0)
            for f in _lib.WIDTH_FAMILIES}


# ---- how the library cuts a mention's candidate list into workgroups (drin_workgroups_per_mention) ---------------------------------
def workgroups_per_mention(D, R, B, N, cached, vertex_activation="gelu", **fields):
    """`drin_workgroups_per_mention` of a default `drin_config` of B mentions x N candidates at widths D / R: the chunks of the
    folded path (`cached` false) or of the per-entity-cache path; 0 where the geometry has neither.  Host-only."""
    import ctypes as C
    from drin_amd import _lib
    c = config_c(D, R, vertex_activation=vertex_activation, batch=B, num_candidates=N, **fields)
    return _lib.load().drin_workgroups_per_mention(C.byref(c), 1 if cached else 0)


def workgroups_of(cfg, B, cached, precision="f32", num_entities=0):
    """... of a `DrinConfig` (widths, candidates, token count, vertex activation) at B mentions."""
    from drin_amd import _lib
    prec = {"f32": _lib.PREC_F32, "bf16x3": _lib.PREC_BF16X3, "bf16x3_all": _lib.PREC_BF16X3_ALL}[precision]
    return workgroups_per_mention(cfg.gcn_embed_dim, cfg.resnet_embed_dim, B, cfg.num_candidates_model, cached,
                                  cfg.gcn_vertex_activation, precision=prec, num_entities=num_entities,
                                  entity_tokens=cfg.max_entity_attr_token_len if cfg.token_level_entities else 0)


# ---- callers of single entry points that several GPU test files share (tests/test_gpu_ghmfc_train.py, test_gpu_mention_rows.py,
# test_gpu_step_kernels.py, test_gpu_launch_caps.py): outputs and scratch are filled with NaN or a sentinel before the call ----------
import ctypes as C  # noqa: E402

from drin_amd import _lib, row_ops  # noqa: E402
from tests.step_restatement import cosine_rows64_grads  # noqa: E402

DEV = "cuda"
KERNEL_TOL = 1e-5                                                     # fp32-FMA kernels, DESIGN.md section 16
NAN = float("nan")
ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)                      # noqa: E731  (NaN positions count)


def rel_err(got, ref, what, scale=None):
    ref = ref.double()
    scale = ref.abs().max().item() if scale is None else scale
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} (max |ref| {scale:.3e}) ratio {err / max(scale, 1e-300):.2e}")
    return err / max(scale, 1e-300)


def ln_bwd(x, res, mean, rstd, gamma, dy, sums=True):
    lib = _lib.load()
    rows, E = x.shape
    dh = torch.full_like(x, float("nan"))
    dgamma, dbeta = (torch.full((E,), float("nan"), device=DEV) for _ in range(2)) if sums else (None, None)
    floats = lib.drin_layernorm_res_bwd_scratch_floats(rows, E)
    scratch = torch.full((floats,), float("nan"), device=DEV) if sums else None
    _lib.check(lib.drin_layernorm_res_bwd(ptr(x), ptr(res), ptr(mean), ptr(rstd), ptr(gamma), ptr(dy), ptr(dh), ptr(dgamma), ptr(dbeta),
                                          ptr(scratch), floats if sums else 0, rows, E, stream()))
    return dh, dgamma, dbeta


def mention_rows_fwd(raw, enc, start, end, representation):
    """(edge_row, vertex_row, idx [2, B, D] int32) of drin_mention_rows_fwd; raw fp32 or bf16.  Outputs are prefilled with a
    sentinel: a row the kernel skipped shows."""
    B, L, D = raw.shape
    edge, vert = torch.full((B, D), 7.0, device=DEV), torch.full((B, D), 7.0, device=DEV)
    idx = torch.full((2, B, D), -5, dtype=torch.int32, device=DEV)
    dtype = _lib.FEAT_BF16 if raw.dtype == torch.bfloat16 else _lib.FEAT_F32
    _lib.check(_lib.load().drin_mention_rows_fwd(ptr(raw), dtype, ptr(enc), ptr(start), ptr(end), representation, ptr(edge), ptr(vert),
                                                 ptr(idx), B, L, D, stream()))
    return edge, vert, idx


def mention_rows_bwd(g_edge, g_vert, start, end, idx, representation, has_encoded, shape, want_raw=True, want_enc=True):
    """(d_raw, d_enc) of drin_mention_rows_bwd, prefilled with NaN: an element the kernel did not write shows."""
    B, L, D = shape
    d_raw = torch.full(shape, float("nan"), device=DEV) if want_raw else None
    d_enc = torch.full(shape, float("nan"), device=DEV) if want_enc else None
    _lib.check(_lib.load().drin_mention_rows_bwd(ptr(g_edge), ptr(g_vert), ptr(start), ptr(end), ptr(idx), representation, has_encoded,
                                                 ptr(d_raw), ptr(d_enc), B, L, D, stream()))
    return d_raw, d_enc


def lowest_argmax(x):
    """[B, D]: the lowest position that attains the max over dim 1; the lowest NaN position where the column holds one."""
    L = x.shape[1]
    pos = torch.arange(L, device=x.device)[None, :, None].expand_as(x)
    nan = torch.isnan(x)
    hit = torch.where(nan.any(1, keepdim=True), nan, x == x.nan_to_num(float("-inf")).max(1, keepdim=True)[0])
    return torch.where(hit, pos, L).min(1)[0]


def cos_case(B, N, D, seed):
    """x [B, D], y [B, N, D] = a x + noise (cosines of 0.3 ... 0.8, none near 0), dout [B, N] with exact zeros in it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g)
    a = 0.3 + torch.rand(B, N, 1, generator=g)
    y = a * x[:, None, :] + torch.randn(B, N, D, generator=g)
    dout = torch.randn(B, N, generator=g)
    dout.view(-1)[1::3] = 0.0
    return x, y, dout


def cos_fwd(x, y, eps):
    B, N, D = y.shape
    out = torch.full((B, N), NAN, device=DEV)
    _lib.check(_lib.load().drin_cosine_rows_fwd(ptr(x), ptr(y), ptr(out), B, N, D, eps, stream()))
    return out


def cos_bwd(x, y, dout, eps, scratch_floats=None):
    B, N, D = y.shape
    floats = 3 * B * N if scratch_floats is None else scratch_floats
    dx, dy = torch.full_like(x, NAN), torch.full_like(y, NAN)
    scratch = torch.full((max(floats, 1),), NAN, device=DEV)
    status = _lib.load().drin_cosine_rows_bwd(ptr(x), ptr(y), ptr(dout), ptr(dx), ptr(dy), ptr(scratch), floats, B, N, D, eps, stream())
    return status, dx, dy


def rows_ratio(got, ref, what):
    """max over rows of max|got - ref| / max|ref| of that row; a row whose reference is all zero must be exactly zero."""
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]).to(got.device)
    assert not torch.isnan(got).any(), what
    scale = ref.abs().amax(1)
    err = (got.double() - ref).abs().amax(1)
    zero = scale == 0
    assert torch.count_nonzero(got[zero]).item() == 0, what
    ratio = (err[~zero] / scale[~zero]).max().item() if (~zero).any() else 0.0
    print(f"{what}: worst row ratio {ratio:.2e} over {int((~zero).sum())} rows (row maxima {scale[~zero].min().item() if (~zero).any() else 0:.2e} ... "
          f"{scale.max().item():.2e}), {int(zero.sum())} all-zero rows")
    return ratio


def check_cosine(x, y, dout, eps, tag):
    out64, dx64, dy64 = cosine_rows64_grads(x, y, dout, eps)
    xd, yd, gd = x.to(DEV), y.to(DEV), dout.to(DEV)
    B, N, D = y.shape
    out = cos_fwd(xd, yd, eps)
    assert not torch.isnan(out).any()
    ferr = (out.double().cpu() - out64).abs().max().item()
    print(f"{tag}: forward max err {ferr:.2e} of max |ref| {out64.abs().max().item():.2e}")
    assert ferr <= KERNEL_TOL * out64.abs().max().item() or (out64 == 0).all() and ferr == 0.0
    status, dx, dy = cos_bwd(xd, yd, gd, eps)
    _lib.check(status)
    assert rows_ratio(dx, dx64, tag + " dx") <= KERNEL_TOL
    assert rows_ratio(dy, dy64, tag + " dy") <= KERNEL_TOL
    dead = (gd == 0).reshape(-1)
    assert dead.any() or B * N == 1
    assert torch.count_nonzero(dy.reshape(B * N, D)[dead]).item() == 0   # dout = 0: exactly-zero dy rows
    _, dx2, dy2 = cos_bwd(xd, yd, gd, eps)
    assert torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(dy), bits(dy2)) and torch.equal(bits(out), bits(cos_fwd(xd, yd, eps)))
    # the autograd edge GHMFC trains through: the same bits
    xl, yl = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
    o = row_ops.cosine_rows(xl, yl, eps)
    o.backward(gd)
    assert torch.equal(bits(o.detach()), bits(out)) and torch.equal(bits(xl.grad), bits(dx)) and torch.equal(bits(yl.grad), bits(dy))
    # one float of scratch short: refused, nothing written
    status, ndx, ndy = cos_bwd(xd, yd, gd, eps, scratch_floats=3 * B * N - 1)
    torch.cuda.synchronize()
    assert status == _lib.E_WORKSPACE and torch.isnan(ndx).all() and torch.isnan(ndy).all()
    return out, dx, dy
