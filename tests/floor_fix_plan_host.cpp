// Stand-alone host program around floor_fix_plan (noisereduce_amd/csrc/onepass_plan.hpp): the ticket layout of the one-launch
// floor fix-up.  tests/test_floor_fix_plan_host.py builds and runs it.
//   floor_fix_plan_host UNITS T TILES   ->   "blocks n_max grid ok", then per ticket of the launch "role unit index"
//   (role 0: maxima block `index` of `unit`; role 1: tile ticket `index`, unit -1), decoded as k_floor_fix decodes it.
#include <cstdio>
#include <cstdlib>

#include "../noisereduce_amd/csrc/onepass_plan.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const long long units = atoll(argv[1]), T = atoll(argv[2]), tiles = atoll(argv[3]);
  const sg::fast::FloorFixPlan p = sg::fast::floor_fix_plan(units, T, tiles);
  printf("%u %u %u %d\n", p.blocks, p.n_max, p.grid, p.ok ? 1 : 0);
  if (!p.ok || p.grid > (1u << 22)) return 0;
  for (unsigned tk = 0; tk < p.grid; ++tk) {
    if (tk < p.n_max) {
      const unsigned u = tk / p.blocks;
      printf("0 %u %u\n", u, tk - u * p.blocks);
    } else {
      printf("1 -1 %u\n", tk - p.n_max);
    }
  }
  return 0;
}
