// Stand-alone host program around noisereduce_amd/csrc/stream_plan.hpp for the box bank (TorchGate's non-stationary gate,
// DESIGN section 13h): tests/test_stream_tg_host.py builds and runs it; no GPU, no HIP.
//   stream_tg_plan_host n_fft W H nt K channels exact n_slots max_block seed
// prints "geo L Lb RC" and "layout RC RB RF max_frames fst fa mk state_bytes", then plays `n_slots` streams through random
// block splits (0-length blocks, blocks of max_block, single samples; several slots per step; a flush with or without a
// last block; a second stream on the flushed slot) and replays on the host which row of which ring every launch of the
// step touches, in the kernels' order:
//   k_sb_decide   writes A row t at t % RF for t in (td0, td1], then for every t in (ts0, ts1] reads the A rows of
//                 [t - Lb, t - Lb + K) cut to [0, td1] and writes sigmoid row t at t % RB
//   k_st_fsmooth  reads the sigmoid rows [r0, r1)
// A read that does not find its own frame at its ring position is a row the ring has already given away: "miss", exit 1.
// It also holds what the kernel's comment promises: a push decides t only when its window is complete (t - Lb + K - 1 <=
// td1), a flush decides every frame up to the stream's last.  Ends with "ok <reads checked> <steps>".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../noisereduce_amd/csrc/stream_plan.hpp"

using namespace sg;

int main(int argc, char** argv) {
  if (argc != 11) { fprintf(stderr, "usage: stream_tg_plan_host n_fft W H nt K channels exact n_slots max_block seed\n"); return 2; }
  const int64_t n_fft = atoll(argv[1]), W = atoll(argv[2]), H = atoll(argv[3]), nt = atoll(argv[4]), K = atoll(argv[5]),
                C = atoll(argv[6]), exact = atoll(argv[7]), n_slots = atoll(argv[8]), max_block = atoll(argv[9]);
  std::mt19937_64 rng((uint64_t)atoll(argv[10]));
  const int64_t F = n_fft / 2 + 1;
  const StGeo g = st_make_geo_box(n_fft, F, (F + 15) / 16 * 16, W, H, nt, K, C, exact != 0);
  const StLayout y = st_layout(g, n_slots, max_block);
  printf("geo %lld %lld %lld\n", (long long)g.L, (long long)g.Lb, (long long)g.RC);
  printf("layout %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)y.RC, (long long)y.RB, (long long)y.RF,
         (long long)y.max_frames, (long long)y.fst, (long long)y.fa, (long long)y.mk, (long long)y.state_bytes());
  if (!g.ns || !g.box || g.L + g.Lb + 1 != K) { printf("miss: geometry\n"); return 1; }

  std::vector<StSlot> slots((size_t)n_slots);
  for (auto& s : slots) s.has_thr = true;
  // which frame (of which of the slot's streams) every ring position of every unit holds (-1: none yet)
  const int64_t nu = n_slots * C;
  std::vector<std::vector<int64_t>> fa((size_t)nu, std::vector<int64_t>((size_t)y.RF, -1));
  std::vector<std::vector<int64_t>> mk((size_t)nu, std::vector<int64_t>((size_t)y.RB, -1));
  std::vector<int64_t> target((size_t)n_slots), streams_done((size_t)n_slots, 0);
  auto new_target = [&](size_t s) { target[s] = W + (int64_t)(rng() % (uint64_t)((K + 2 * nt + 12) * H + 2 * max_block)); };
  for (size_t s = 0; s < slots.size(); ++s) new_target(s);
  long long reads = 0, steps = 0;
  while (true) {
    std::vector<sg_stream_rec> recs;
    bool open = false;
    for (int32_t s = 0; s < (int32_t)n_slots; ++s) {
      if (streams_done[(size_t)s] >= 2) continue;
      open = true;
      if (rng() % 4 == 0) continue;   // (not every stream is part of every step)
      const int64_t left = target[(size_t)s] - slots[(size_t)s].n;
      int64_t n;
      switch (rng() % 5) {
        case 0: n = 0; break;
        case 1: n = 1; break;
        case 2: n = max_block; break;
        default: n = (int64_t)(rng() % (uint64_t)(max_block + 1));
      }
      sg_stream_rec r{};
      r.slot = s;
      r.n_samples = n < left ? n : left;
      r.flush = (r.n_samples == left && rng() % 2) ? 1 : 0;   // (else the flush comes later, without a last block)
      if (left == 0) r.flush = 1;
      r.in_stride = r.n_samples;
      recs.push_back(r);
    }
    if (!open) break;
    std::string err;
    const int rc = st_check_step(g, max_block, 0, slots, SG_F32, SG_F32, recs.data(), (int32_t)recs.size(), nullptr, nullptr, &err);
    if (rc) { printf("miss: st_check_step refuses: %s\n", err.c_str()); return 1; }
    const StStep P = st_plan_step(g, slots, recs.data(), (int32_t)recs.size(), nullptr, nullptr);
    ++steps;
    for (const StUnit& U : P.units) {
      std::vector<int64_t>& A = fa[(size_t)U.state];
      std::vector<int64_t>& S = mk[(size_t)U.state];
      // (a row is named by its stream as well: a second stream on a slot must not find the first one's row t as its own)
      const int64_t gen = streams_done[(size_t)U.slot] << 40;
      if (U.td1 - U.td0 > y.max_frames || U.ts1 - U.ts0 > y.max_frames + g.L) {
        printf("miss: a step of %lld / %lld frames (max_frames %lld)\n", (long long)(U.td1 - U.td0), (long long)(U.ts1 - U.ts0),
               (long long)y.max_frames);
        return 1;
      }
      if (U.flush && (U.td1 != U.Tend - 1 || U.ts1 != U.td1 || U.ta1 != U.td1)) { printf("miss: a flush leaves frames undecided\n"); return 1; }
      for (int64_t t = U.td0 + 1; t <= U.td1; ++t) A[(size_t)(t % y.RF)] = gen + t;
      for (int64_t t = U.ts0 + 1; t <= U.ts1; ++t) {
        if (!U.flush && t - g.Lb + K - 1 > U.td1) { printf("miss: frame %lld decided before its window is in\n", (long long)t); return 1; }
        const int64_t ja = t - g.Lb < 0 ? 0 : t - g.Lb;
        const int64_t jb = t - g.Lb + K > U.td1 + 1 ? U.td1 + 1 : t - g.Lb + K;
        if (t < ja || t >= jb) { printf("miss: frame %lld outside its own window\n", (long long)t); return 1; }
        for (int64_t q = ja; q < jb; ++q, ++reads)
          if (A[(size_t)(q % y.RF)] != gen + q) {
            printf("miss: unit %d frame %lld reads A row %lld, the ring holds %lld there (RF %lld)\n", U.state, (long long)t,
                   (long long)q, (long long)A[(size_t)(q % y.RF)], (long long)y.RF);
            return 1;
          }
        S[(size_t)(t % y.RB)] = gen + t;
      }
      for (int64_t r = U.r0; r < U.r1; ++r, ++reads)
        if (S[(size_t)(r % y.RB)] != gen + r) {
          printf("miss: unit %d smooths sigmoid row %lld, the ring holds %lld there (RB %lld)\n", U.state, (long long)r,
                 (long long)S[(size_t)(r % y.RB)], (long long)y.RB);
          return 1;
        }
    }
    for (size_t i = 0; i < recs.size(); ++i) {
      const size_t s = (size_t)recs[i].slot;
      slots[s] = P.after[i];
      if (recs[i].flush) {
        if (slots[s].n != 0) { printf("miss: a flushed slot is not empty\n"); return 1; }
        ++streams_done[s];
        new_target(s);
      }
    }
  }
  printf("ok %lld %lld\n", reads, steps);
  return 0;
}
