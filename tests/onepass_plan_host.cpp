// Stand-alone driver of noisereduce_amd/csrc/onepass_plan.hpp for tests/test_onepass_plan_host.py: the functions the kernel
// runs, on the host.
//   plan  <28 numbers: the fields of OpPlanIn in declaration order> <first ticket> <count>
//         line 1: the plan's ranges; then one line per ticket
//   magic <divisor> <first dividend> <count>       one quotient per line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../noisereduce_amd/csrc/onepass_plan.hpp"

using namespace sg::fast;

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "magic")) {
    const uint32_t d = (uint32_t)strtoull(argv[2], nullptr, 10);
    const uint64_t n0 = strtoull(argv[3], nullptr, 10), cnt = strtoull(argv[4], nullptr, 10);
    const OpMagic g = op_magic(d);
    for (uint64_t n = n0; n < n0 + cnt && n <= 0xffffffffull; ++n) printf("%u\n", op_magic_div((uint32_t)n, g.m, g.s));
    return 0;
  }
  if (argc != 2 + 28 + 2 || strcmp(argv[1], "plan")) {
    fprintf(stderr, "usage: see the head of %s\n", __FILE__);
    return 2;
  }
  long long a[28];
  for (int i = 0; i < 28; ++i) a[i] = strtoll(argv[2 + i], nullptr, 10);
  OpPlanIn I{};
  int i = 0;
  I.x = (uint64_t)a[i++]; I.out = (uint64_t)a[i++];
  I.in_dtype = (int32_t)a[i++]; I.out_dtype = (int32_t)a[i++]; I.normalize = (int32_t)a[i++];
  I.stride = a[i++]; I.lo = a[i++]; I.hi = a[i++]; I.cs = a[i++]; I.pad = a[i++]; I.Lp = a[i++]; I.c0 = a[i++]; I.unit0 = a[i++];
  I.n_chunks = (int32_t)a[i++];
  I.ostride = a[i++]; I.p0 = a[i++]; I.p1 = a[i++]; I.g_step = a[i++]; I.g0 = a[i++]; I.g_lo = a[i++]; I.g_hi = a[i++];
  I.padL = (int32_t)a[i++];
  I.T = a[i++]; I.Lout = a[i++]; I.h_begin = a[i++]; I.h_end = a[i++];
  I.n_tiles = (int32_t)a[i++]; I.scan_q = (int32_t)a[i++];
  const OpPlan P = op_plan_build(I);
  const uint64_t t0 = strtoull(argv[2 + 28], nullptr, 10), cnt = strtoull(argv[2 + 29], nullptr, 10);
  printf("%u %u %d %d %d %d %" PRIu64 " %" PRIu64 "\n", P.k0, P.k1, P.bv0, P.bv1, P.tf0, P.tf1, P.src, P.dst);
  for (uint64_t t = t0; t < t0 + cnt; ++t) {
    const OpTile tl = op_plan_tile(P, (uint32_t)t);
    const OpScan sc = op_plan_scan(P, tl);
    printf("%u %d %u %u %d %d %d %" PRId64 " %" PRId64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %" PRId64 "\n", tl.u, tl.jt, tl.row,
           tl.k, (int)tl.interior, (int)op_plan_blk_vec(P, tl), (int)op_plan_tile_fast(P, tl), op_plan_src_off(P, tl),
           op_plan_dst_off(P, tl), op_plan_xbits_off(P, tl, 288), op_plan_part2_off(P, tl), sc.c0, sc.c1, (int)sc.has, sc.off);
  }
  return 0;
}
