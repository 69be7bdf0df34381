// Stand-alone host program around noisereduce_amd/csrc/route.hpp (tests/test_route_plan_host.py builds and drives it; no GPU,
// no HIP).  One caps / shape tuple per line on stdin, or one tuple as command-line arguments:
//   variant stationary smooth_mask prop_decrease iir_b nf nt n_movemean ktot fused_ok t_sm2_ok geom reg_sel ftab3 optab regtab
//   norm64 force_unfused force_nofast force_f64_decide force_noseam force_nolean force_split fast_integer force_exact
//   exact_materialised rowgate_mode tile_order ws_budget | F FS n T nh in_dtype out_dtype units field noise_rows
// geom: 0 default 1024, 1 register (reg_sel 0 / 1 / 2 = n_fft 512 / 256 / 2048), 2 other power of two, 3 mixed radix,
// 4 chirp-z, 5 long frames.  Per tuple one line: every field of plan_S, of plan_T, and workspace_S's three numbers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../noisereduce_amd/csrc/route.hpp"

using namespace sg::route;
using sg::host::OnePassGeom;

// the one-pass geometries as api.hip lays them out (hop, NF, NH, tile_words, xw, max_nf, max_nt, F, lds, extra); lds plays no part
static const OnePassGeom OP1024{256, 16, 16, 288, 9, 8, 16, 513, 0, 3};
static const OnePassGeom OP512{128, 32, 29, 320, 5, 8, 24, 257, 0, 0}, OP512S{128, 32, 32, 320, 5, 8, 24, 257, 0, 3};
static const OnePassGeom OP256{64, 64, 61, 384, 3, 8, 40, 129, 0, 0}, OP256S{64, 64, 64, 384, 3, 8, 40, 129, 0, 3};
static const OnePassGeom OP2048{512, 8, 8, 272, 17, 24, 8, 1025, 0, 3};

static void facts(const BatchFacts& f) {
  printf(" %d %d %d %d %d %d %d %d", f.keeps, f.has_P, f.has_raw, f.fused, f.fast, f.k16_only, f.rg, (int)f.range);
}

static int one(const std::vector<std::string>& a) {
  if (a.size() != 39) { fprintf(stderr, "route_plan_host: 39 values per tuple, got %zu\n", a.size()); return 2; }
  size_t i = 0;
  auto I = [&] { return atoll(a[i++].c_str()); };
  auto D = [&] { return atof(a[i++].c_str()); };
  RouteCaps c;
  c.variant = (int)I(); c.stationary = I(); c.smooth_mask = I(); c.prop_decrease = D(); c.iir_b = D();
  c.nf = (int)I(); c.nt = (int)I(); c.n_movemean = (int)I(); c.ktot = I(); c.fused_ok = I(); c.t_sm2_ok = I();
  const int geom = (int)I(), sel = (int)I();
  c.geom = (GeomClass)geom;
  if (c.geom == GeomClass::DEFAULT) c.op = c.op_seam = &OP1024;
  if (c.geom == GeomClass::REG) {
    c.op = sel == 0 ? &OP512 : (sel == 1 ? &OP256 : &OP2048);
    c.op_seam = sel == 0 ? &OP512S : (sel == 1 ? &OP256S : &OP2048);
    c.reg_abut = sel == 2;
    c.reg_frames = c.op->NF;
  }
  c.ftab3 = I(); c.optab = I(); c.regtab = I(); c.norm64 = I();
  c.force_unfused = I(); c.force_nofast = I(); c.force_f64_decide = I(); c.force_noseam = I(); c.force_nolean = I();
  c.force_split = I(); c.fast_integer = I(); c.force_exact = I(); c.exact_materialised = I();
  c.rowgate_mode = (int)I(); c.tile_order = (int)I(); c.ws_budget = I();
  RouteShape s;
  s.F = (int)I(); s.FS = (int)I(); s.n = (int)I(); s.T = I(); s.nh = I(); s.in_dtype = (int)I(); s.out_dtype = (int)I();
  s.units = I(); s.field = I(); s.noise_rows = I();
  const SPlan p = plan_S(c, s);
  printf("%d %d %d %d %d %d %d %d %d %d %d %d", (int)p.pipe, (int)p.decide, (int)p.ns, p.smooth_stage, p.k16_to_mask, (int)p.apply,
         p.seam, p.exact_tiled, p.lean, p.f32_copy, p.fast, p.reg);
  facts(p.facts);
  const TPlan t = plan_T(c, s);
  printf(" %d %d %d %d %d %d %d %d %d %d", t.rowgate, t.bits_path, t.to_raw, t.row_fused, (int)t.thresh, (int)t.ns, t.smooths,
         (int)t.apply, t.fast, t.reg);
  facts(t.facts);
  const Workspace w = workspace_S(c, p, s, s.units);
  printf(" %lld %lld %lld\n", (long long)w.ub, (long long)w.unit, (long long)w.exchange);
  return 0;
}

static std::vector<std::string> split(const char* line) {
  std::vector<std::string> v;
  std::string cur;
  for (const char* q = line;; ++q) {
    if (*q == ' ' || *q == '\n' || *q == '\0') {
      if (!cur.empty()) v.push_back(cur);
      cur.clear();
      if (*q == '\0') break;
    } else {
      cur += *q;
    }
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc > 1) return one(std::vector<std::string>(argv + 1, argv + argc));
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    const std::vector<std::string> a = split(line);
    if (a.empty()) continue;
    if (int rc = one(a)) return rc;
  }
  return 0;
}
