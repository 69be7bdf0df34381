// The tables the table-driven paths upload and their kernels read, and the host arithmetic that fills them: plain C++17, no
// HIP, so that a planner (stream_plan.hpp) and a stand-alone host program around it see them.  tile_core.hpp includes this
// header; the layouts are the kernels' (do not reorder a member).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace sg {

// tile i of a stage: {unit / row / noise source, first, end}; kind is 0 except in the stream's finish stage
struct Tile {
  int32_t idx, kind;
  int64_t a, b;
};

inline int64_t tile_fdiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline int64_t tile_cdiv(int64_t a, int64_t b) { return -tile_fdiv(-a, b); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// all tile lists of a call, back to back: a stage is the tiles pushed between its begin_stage() and the next one
struct TileList {
  std::vector<Tile> tiles;
  int64_t size() const { return (int64_t)tiles.size(); }
  int64_t begin_stage() const { return size(); }
  int64_t count_since(int64_t first) const { return size() - first; }
  void push(int64_t idx, int64_t a, int64_t b, int kind = 0) { tiles.push_back(Tile{(int32_t)idx, kind, a, b}); }
  // [lo, hi) in pieces of `step`; the last piece ends at hi, or runs its full step where clamp is false (band blocks)
  void push_ranges(int64_t idx, int64_t lo, int64_t hi, int64_t step, bool clamp = true, int kind = 0) {
    for (int64_t a = lo; a < hi; a += step) push(idx, a, clamp ? std::min(hi, a + step) : a + step, kind);
  }
};

// ---- a stream step's tables (stream.hip's kernels; stream_plan.hpp fills them) ------------------------------------------
struct StUnit {
  int64_t in_off, out_off;   // element of in holding the block's first sample / of out receiving sample E0
  int64_t n0, n1;            // samples received before / after this step
  int64_t td0, td1;          // last decided (transformed) frame before / after (-1: none)
  int64_t ts0, ts1;          // non-stationary: last frame with a raw mask row before / after (td - lookahead; td at a flush)
  int64_t ta0, ta1;          // last applied frame before / after
  int64_t Tend;              // frames of the whole stream when flushing, else "unbounded"
  int64_t Lout;              // flush: valid samples of the inverse transform (zero tail beyond)
  int64_t E0, E1;            // emitted before / after
  int64_t cov0;              // end of the samples the applied frames of earlier steps reach (carry valid below it)
  int64_t r0, r1;            // mask rows the applied frames read
  int64_t mrow, srow;        // first row of this unit in the smoothed-row / segment scratch
  int32_t state;             // slot * channels + channel
  int32_t slot;
  int32_t par;               // carry buffer to read (the other one is written)
  int32_t flush;
};
enum { ST_OLA = 0, ST_APPEND = 1, ST_CLEAR = 2 };   // Tile::kind of the finish stage
// a unit's part of a spectrum step: the element of spec / smask holding bin 0 of its first newly applied frame (ta0 + 1);
// the frames follow as consecutive rows of F bins
struct StSpec {
  int64_t spec_off, mask_off;
};

// a unit's part of a feature step: the element of feat holding filter 0 / of fmask holding bin 0 of its first newly applied
// frame; the frames follow as consecutive rows of M filters / F bins
struct StFeatUnit {
  int64_t feat_off, mask_off;
};

}  // namespace sg
