// Host program over drin_amd/csrc/arena.h and layout.h: every region of the layer-by-layer workspace (Layout) and of the backward
// pass's temporaries (BackwardScratch) starts on a 256-byte boundary, regions that are live together are disjoint and end inside
// the total, BackwardScratch's total is Layout::bwd_scratch_floats, and each of its regions holds what drin_backward_ex indexes.
// The sizes below are the test's own statement of what the kernels index, not the layout's.
// Built and run by tests/test_workspace_host.py (no GPU, no HIP runtime).  Exit status 0 = all cases hold.
#include <cstdio>
#include <vector>

#include "arena.h"
#include "layout.h"

using namespace drin;

static std::vector<Region> regions;
static void reg(const char* name, size_t offset, size_t floats) { regions.push_back({name, offset, floats}); }
static const char* bad(size_t total) { return first_bad_region(regions.data(), (int)regions.size(), total); }

static void describe(const drin_config& c, const char* what) {
  std::printf("%s: layers %d B %d N %d D %d R %d vector %d dynamic %d precision %d edge act %d: ", what, c.num_layers, c.batch, c.num_candidates,
              c.embed_dim, c.image_dim, c.vector_edges, c.dynamic_edges, c.precision, c.edge_activation);
}

static int check(const drin_config& c) {
  const size_t B = c.batch, M = B * c.num_candidates, D = c.embed_dim, R = c.image_dim, EW = c.vector_edges ? D : 1;
  const int nl = c.num_layers;
  const bool keep_z = (c.edge_activation == DRIN_ACT_GELU || c.edge_activation == DRIN_ACT_SILU) && c.dynamic_edges;
  // what both layouts hold from the first launch to the last: pooled inputs, split-K scratch, weight planes
  auto shared = [&](const Layout& L) {
    regions.clear();
    reg("edges_scalar", L.edges_scalar, c.vector_edges ? 4 * M : 0);
    reg("span_mean", L.span_mean, B * D), reg("mimg_pool", L.mimg_pool, B * R);
    reg("mobj_pool", L.mobj_pool, c.mention_object_inner > 1 ? B * c.mention_objects * R : 0);
    reg("eobj_pool", L.eobj_pool, c.entity_object_inner > 1 ? M * c.entity_objects * R : 0);
    reg("eimg_pool", L.eimg_pool, c.entity_image_inner > 1 ? M * R : 0), reg("xet_pool", L.xet_pool, c.entity_tokens > 0 ? M * D : 0);
    reg("splitk", L.splitk, L.splitk_floats);
    if (L.weight_planes) {
      for (int k = 0; k < 4; ++k) reg("wp_enc", L.wp_enc[k], (k & 1) ? D * R : D * D);
      for (int l = 0; l < nl; ++l) reg("wp_h", L.wp_h[l], D * D), reg("wp_u", L.wp_u[l], D * D), reg("wp_v", L.wp_v[l], D * D);
    }
  };
  auto layer = [&](const Layout& L, int l) {   // what layer l reads and writes
    reg("edges", L.edges[l], 4 * M * EW), reg("vm", L.vm[l], 2 * B * D), reg("ve", L.ve[l], 2 * M * D);
    reg("masked", L.masked[l], 4 * M * EW), reg("pre", L.pre[l], c.vector_edges ? 4 * M * D : 0);
    reg("agg_m", L.agg_m[l], 2 * B * D), reg("agg_e", L.agg_e[l], 2 * M * D), reg("fu", L.fu[l], 2 * B * D);
  };

  // training: every layer's intermediates are kept, everything is live together
  Layout T;
  T.build(c, true);
  shared(T);
  for (int l = 0; l < nl; ++l) {
    layer(T, l);
    reg("edge_z", T.edge_z[l], keep_z ? 4 * M * EW : 0);
    reg("h_m", T.h_m[l], 2 * B * D), reg("h_e", T.h_e[l], 2 * M * D), reg("fv", T.fv[l], 2 * M * D);
    reg("ln_stat_m", T.ln_stat_m[l], 4 * B), reg("ln_stat_e", T.ln_stat_e[l], 4 * M);
  }
  reg("edges", T.edges[nl], 4 * M * EW), reg("vm", T.vm[nl], 2 * B * D), reg("ve", T.ve[nl], 2 * M * D);
  reg("wt", T.wt, (2 * (size_t)nl + 1) * D * D);
  // the LayerNorm backward's block rows and shared level-1 rows, then one level-1 area [3][16][D] per layer
  reg("ln_part", T.ln_part, ((size_t)1024 + 16 + 16 * (nl > 0 ? nl : 1)) * 3 * D);
  reg("tn_part", T.tn_part, T.tn_part_floats), reg("small_part", T.small_part, T.small_part_floats);
  reg("colsum_part", T.colsum_part, T.colsum_part_floats);
  reg("bwd_scratch", T.bwd_scratch, T.bwd_scratch_floats);
  if (const char* r = bad(T.total_floats)) return describe(c, "training layout"), std::printf("region %s\n", r), 1;
  for (int l = 0; l < nl; ++l)
    if (ln_bwd_level1(D, l) + 3 * 16 * D > ((size_t)1024 + 16 + 16 * (nl > 0 ? nl : 1)) * 3 * D || ln_bwd_level1(D, l) < ((size_t)1024 + 16) * 3 * D)
      return describe(c, "training layout"), std::printf("level-1 area of layer %d leaves ln_part\n", l), 1;

  // the backward pass's temporaries: nl + 1 generations of vertex gradients, two of edge gradients, per-layer dfu / dfv
  BackwardScratch S;
  S.build(c);
  if (S.total_floats != T.bwd_scratch_floats)
    return describe(c, "backward scratch"), std::printf("total %zu, Layout::bwd_scratch_floats %zu\n", S.total_floats, T.bwd_scratch_floats), 1;
  regions.clear();
  for (int l = 0; l <= nl; ++l) reg("g_vm", S.g_vm[l], 2 * B * D), reg("g_ve", S.g_ve[l], 2 * M * D);
  reg("g_e[0]", S.g_e[0], 4 * M * EW), reg("g_e[1]", S.g_e[1], 4 * M * EW), reg("dpre", S.dpre, 4 * M * EW);
  reg("dA_m", S.dA_m, 2 * B * D), reg("dA_e", S.dA_e, 2 * M * D), reg("cos_scratch", S.cos_scratch, 3 * M);
  // layers below the last have a live edge update: dfu / dfv of each are operands of the grouped weight-gradient launch at the end
  // of the pass; the last layer's (and a zero-layer pass's) are never written and share slot 0
  for (int l = 0; l < (nl > 1 ? nl - 1 : 1); ++l) reg("dfu_of", S.dfu_of[l], 2 * B * D), reg("dfv_of", S.dfv_of[l], 2 * M * D);
  if (const char* r = bad(S.total_floats)) return describe(c, "backward scratch"), std::printf("region %s\n", r), 1;
  if (nl > 1 && (S.dfu_of[nl - 1] != S.dfu_of[0] || S.dfv_of[nl - 1] != S.dfv_of[0]))
    return describe(c, "backward scratch"), std::printf("the last layer's dfu / dfv do not share slot 0\n"), 1;

  // inference: layers re-use their scratch and ping-pong the vertex and edge buffers - live together is one layer at a time
  Layout I;
  I.build(c, false);
  if (I.bwd_scratch_floats != 0 || I.tn_part_floats != 0) return describe(c, "inference layout"), std::printf("holds training scratch\n"), 1;
  for (int l = 0; l < nl || l == 0; ++l) {
    shared(I);
    if (l < nl) {
      layer(I, l);
      reg("edges'", I.edges[l + 1], 4 * M * EW), reg("vm'", I.vm[l + 1], 2 * B * D), reg("ve'", I.ve[l + 1], 2 * M * D);
      // pre-LayerNorm rows are normalised in place; W_v's output is consumed before agg_e is written again
      if (I.h_m[l] != I.vm[l + 1] || I.h_e[l] != I.ve[l + 1] || I.fv[l] != I.agg_e[l])
        return describe(c, "inference layout"), std::printf("layer %d: h / fv do not alias the buffers they are documented to\n", l), 1;
    } else {
      reg("edges", I.edges[0], 4 * M * EW), reg("vm", I.vm[0], 2 * B * D), reg("ve", I.ve[0], 2 * M * D);
    }
    if (const char* r = bad(I.total_floats)) return describe(c, "inference layout"), std::printf("layer %d region %s\n", l, r), 1;
  }
  return 0;
}

int main() {
  // the arena itself: offsets in order, rounded to 64 floats, empty regions take nothing
  {
    Arena A;
    if (A.take(1) != 0 || A.take(0) != 64 || A.take(64) != 64 || A.take(65) != 128 || A.total != 256 || Arena::rounded(0) != 0 ||
        Arena::rounded(63) != 64)
      return std::printf("Arena::take does not round to 64 floats\n"), 1;
    float base[4];
    if (Arena::at(base, 3) != base + 3) return std::printf("Arena::at\n"), 1;
  }
  int cases = 0;
  for (int nl = 0; nl <= 8; ++nl)
    for (int B : {1, 2, 255, 256, 257, 300, 1024, 2049, 4096})
      for (int N : {1, 11, 101})
        for (int dims = 0; dims < 2; ++dims)
          for (int vec = 0; vec < 2; ++vec)
            for (int dyn = 0; dyn < 2; ++dyn)
              for (int prec : {(int)DRIN_PREC_F32, (int)DRIN_PREC_BF16X3, (int)DRIN_PREC_BF16X3_ALL})
                for (int act : {(int)DRIN_ACT_DEFAULT, (int)DRIN_ACT_GELU}) {
                  drin_config c = {};
                  c.batch = B, c.num_candidates = N, c.embed_dim = dims ? 768 : 64, c.image_dim = dims ? 2048 : 128;
                  c.mention_tokens = 8, c.image_regions = 4, c.mention_objects = 3, c.entity_objects = 1, c.mention_object_inner = dims ? 2 : 1;
                  c.entity_object_inner = c.entity_image_inner = dims ? 0 : 2, c.entity_tokens = dims ? 0 : 4;
                  c.num_layers = nl, c.dynamic_edges = dyn, c.vector_edges = vec, c.precision = prec, c.edge_activation = act;
                  if (check(c)) return 1;
                  ++cases;   // (training and inference layouts of each)
                }
  std::printf("workspace: %d cases hold\n", cases);
  return 0;
}
