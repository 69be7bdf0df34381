// Stand-alone host program around noisereduce_amd/csrc/stream_plan.hpp (tests/test_stream_plan_host.py builds and drives it; no
// GPU, no HIP).  Commands on stdin, one per line; every command answers with lines that end in a line "end":
//   bank n_fft W H nt lookahead channels kind exact n_slots max_block M has_thr
//        a bank of that geometry (kind: SG_STREAM_*; M: filters of its filterbank, 0 = none; has_thr: every slot's flag);
//        answers "layout" + RC RB RF max_frames, the bytes of every buffer in StLayout's order, tabs, ws, state_bytes(), RB_ring
//        and bits_alloc
//   thr slot flag | reset slot            a slot's threshold flag / a slot emptied (its flag stays)
//   counters n | payload n                st_counters_at / 8 * st_payload_words of the bank's geometry
//   step mode in_dtype out_dtype n_recs   mode 0 push, 1 spectrum, 2 features, 3 both tables given
//        then for mode 1 / 3:  dtype has_spec has_recs has_mask       for mode 2 / 3:  dtype has_feat has_recs has_mask power take_log eps scale
//        then per record:      slot flush n_samples in_offset in_stride out_offset out_stride
//                              [spec_offset mask_offset stride]  [feat_offset feat_stride mask_offset mask_stride]
//        answers "err code message" -- or "plan" with mrows sframes and the four stage ranges, one "unit" line per StUnit (every
//        member in declaration order), one "third" line per StSpec / StFeatUnit, one "tile" line per tile, one "slot" line per
//        record (the slot's state afterwards) -- and commits that state, as st_push does.
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "../noisereduce_amd/csrc/stream_plan.hpp"

using namespace sg;

int main() {
  StGeo g{};
  int64_t max_block = 0;
  int M = 0;
  std::vector<StSlot> slots;
  char buf[1 << 16];
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string cmd;
    if (!(in >> cmd)) continue;
    auto I = [&] { long long v = 0; in >> v; return (int64_t)v; };
    auto D = [&] { std::string s; in >> s; return atof(s.c_str()); };
    if (cmd == "bank") {
      const int64_t n_fft = I(), W = I(), H = I(), nt = I(), L = I(), C = I(), kind = I(), exact = I(), n_slots = I();
      max_block = I();
      M = (int)I();
      const bool has_thr = I() != 0;
      const int64_t F = n_fft / 2 + 1;
      g = st_make_geo(n_fft, F, (F + 15) / 16 * 16, W, H, nt, L, C, (int)kind, exact != 0);
      slots.assign((size_t)n_slots, StSlot());
      for (auto& s : slots) s.has_thr = has_thr;
      const StLayout y = st_layout(g, n_slots, max_block);
      printf("layout %lld %lld %lld %lld", (long long)y.RC, (long long)y.RB, (long long)y.RF, (long long)y.max_frames);
      for (int64_t v : {y.ring, y.carry, y.fst, y.fa, y.mk, y.rmax, y.bits, y.nst, y.thr, y.T2, y.stage, y.slot_list, y.tabs, y.ws,
                        y.state_bytes(), y.RB_ring, y.bits_alloc})
        printf(" %lld", (long long)v);
      printf("\n");
    } else if (cmd == "thr") {
      const int64_t s = I();
      slots.at((size_t)s).has_thr = I() != 0;
    } else if (cmd == "reset") {
      StSlot& S = slots.at((size_t)I());
      const bool t = S.has_thr;
      S = StSlot();
      S.has_thr = t;
    } else if (cmd == "counters") {
      const StCounters k = st_counters_at(g, I());
      printf("counters %lld %lld %lld %lld\n", (long long)k.td, (long long)k.ts, (long long)k.ta, (long long)k.E);
    } else if (cmd == "payload") {
      printf("payload %lld\n", (long long)(8 * st_payload_words(g, I())));
    } else if (cmd == "step") {
      const int mode = (int)I(), in_dtype = (int)I(), out_dtype = (int)I();
      const int32_t n = (int32_t)I();
      int dummy = 0;   // stands for a device buffer: the planner never reads through it
      StSpecOut so{};
      StFeatOut fo{};
      bool so_recs = false, fo_recs = false;
      if (mode == 1 || mode == 3) {
        so.dtype = (int)I();
        so.spec = I() ? &dummy : nullptr;
        so_recs = I() != 0;
        so.mask = I() ? &dummy : nullptr;
      }
      if (mode == 2 || mode == 3) {
        fo.dtype = (int)I();
        fo.feat = I() ? &dummy : nullptr;
        fo_recs = I() != 0;
        fo.mask = I() ? &dummy : nullptr;
        fo.power = (int32_t)I();
        fo.take_log = (int32_t)I();
        fo.eps = D();
        fo.scale = D();
      }
      std::vector<sg_stream_rec> recs((size_t)n);
      std::vector<sg_stream_spec_rec> srecs((size_t)n);
      std::vector<sg_stream_feat_rec> frecs((size_t)n);
      for (int32_t i = 0; i < n; ++i) {
        sg_stream_rec& r = recs[i];
        r.slot = (int32_t)I(); r.flush = (int32_t)I(); r.n_samples = I();
        r.in_offset = I(); r.in_stride = I(); r.out_offset = I(); r.out_stride = I();
        if (mode == 1 || mode == 3) { srecs[i].spec_offset = I(); srecs[i].mask_offset = I(); srecs[i].stride = I(); }
        if (mode == 2 || mode == 3) {
          frecs[i].feat_offset = I(); frecs[i].feat_stride = I(); frecs[i].mask_offset = I(); frecs[i].mask_stride = I();
        }
      }
      if (!in) { fprintf(stderr, "stream_plan_host: short step line\n"); return 2; }
      so.recs = so_recs ? srecs.data() : nullptr;
      fo.recs = fo_recs ? frecs.data() : nullptr;
      const StSpecOut* sp = (mode == 1 || mode == 3) ? &so : nullptr;
      const StFeatOut* fp = (mode == 2 || mode == 3) ? &fo : nullptr;
      std::string err;
      const int rc = st_check_step(g, max_block, M, slots, in_dtype, out_dtype, recs.data(), n, sp, fp, &err);
      if (rc) {
        printf("err %d %s\n", rc, err.c_str());
      } else {
        const StStep P = st_plan_step(g, slots, recs.data(), n, sp, fp);
        printf("plan %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)P.mrows, (long long)P.sframes, (long long)P.t_dec,
               (long long)P.n_dec, (long long)P.t_fs, (long long)P.n_fs, (long long)P.t_ap, (long long)P.n_ap, (long long)P.t_fin,
               (long long)P.n_fin);
        for (const StUnit& U : P.units) {
          printf("unit");
          for (int64_t v : {U.in_off, U.out_off, U.n0, U.n1, U.td0, U.td1, U.ts0, U.ts1, U.ta0, U.ta1, U.Tend, U.Lout, U.E0, U.E1,
                            U.cov0, U.r0, U.r1, U.mrow, U.srow, (int64_t)U.state, (int64_t)U.slot, (int64_t)U.par, (int64_t)U.flush})
            printf(" %lld", (long long)v);
          printf("\n");
        }
        for (const StSpec& s : P.specs) printf("third %lld %lld\n", (long long)s.spec_off, (long long)s.mask_off);
        for (const StFeatUnit& s : P.feats) printf("third %lld %lld\n", (long long)s.feat_off, (long long)s.mask_off);
        for (const Tile& t : P.tl.tiles) printf("tile %d %d %lld %lld\n", t.idx, t.kind, (long long)t.a, (long long)t.b);
        for (int32_t i = 0; i < n; ++i) {
          const StSlot& S = P.after[i];
          printf("slot %d %lld %d %d\n", recs[i].slot, (long long)S.n, S.par, S.has_thr ? 1 : 0);
          slots[(size_t)recs[i].slot] = S;
        }
      }
    } else {
      fprintf(stderr, "stream_plan_host: unknown command %s\n", cmd.c_str());
      return 2;
    }
    printf("end\n");
    fflush(stdout);   // (the driver waits for this line before it sends the next command)
  }
  return 0;
}
