// libmi355gate.so -- options, the per-stage profiler and the debug taps of include/mi355gate_debug.h.
// Host code only: what needs a kernel, or state of the gate's stages, asks api.hip (handle.hpp).
#include <cstring>

#include "handle.hpp"
#include "limits.hpp"

using namespace sg;
using namespace sg::host;

extern "C" int sg_set_option(sg_handle* h, int32_t option, int64_t value) {
  if (!h) return SG_E_INVALID;
  switch (option) {
    case SG_OPT_FORCE_UNFUSED: h->force_unfused = value != 0; return SG_OK;
    case SG_OPT_FORCE_NOFAST: h->force_nofast = value != 0; return SG_OK;
    case SG_OPT_FORCE_F64_DECIDE: h->force_f64_decide = value != 0; return SG_OK;
    case SG_OPT_FORCE_NOSEAM: h->force_noseam = value != 0; return SG_OK;
    case SG_OPT_FORCE_NOLEAN: h->force_nolean = value != 0; return SG_OK;
    case SG_OPT_FORCE_SPLIT: h->force_split = value != 0; return SG_OK;
    case SG_OPT_FAST_INTEGER: h->fast_integer = value != 0; return SG_OK;
    case SG_OPT_FORCE_EXACT: h->force_exact = value != 0; return SG_OK;
    case SG_OPT_FORCE_NOROWGATE:
      if (value < 0 || value > 2) FAIL(h, SG_E_INVALID, "SG_OPT_FORCE_NOROWGATE: 0 (auto), 1 (never) or 2 (always)");
      h->rowgate_mode = (int)value;
      return SG_OK;
    case SG_OPT_ROWGATE_TAP: h->rg_tap = value != 0; return SG_OK;
    case SG_OPT_ROWGATE_SHAPE:
      if (value != 8 && value != 16) FAIL(h, SG_E_INVALID, "SG_OPT_ROWGATE_SHAPE: 8 or 16 waves");
      h->rg_shape = (int)value;
      return SG_OK;
    case SG_OPT_INJECT_HANDOFF_FAULT: h->inject_fault = (unsigned)value & 127u; return SG_OK;
    case SG_OPT_TILE_ORDER:
      if (value < 0 || value > 2) FAIL(h, SG_E_INVALID, "SG_OPT_TILE_ORDER: 0 (persistent workgroups), 1 (block index) or 2 (one ticket per workgroup)");
      h->tile_order = (int)value;
      return SG_OK;
    case SG_OPT_EXACT_MATERIALISED: h->exact_materialised = value != 0; return SG_OK;
    case SG_OPT_STATS_THREE_LAUNCH: h->stats_three = value != 0; return SG_OK;
    case SG_OPT_FLOOR_TWO_LAUNCH: h->floor_two = value != 0; return SG_OK;
    case SG_OPT_FLOOR_TEST:
      if (value < 0 || value > 2) FAIL(h, SG_E_INVALID, "SG_OPT_FLOOR_TEST: 0 (predicted), 1 (a priori) or 2 (in the gate kernel)");
      h->floor_test = (int)value;
      return SG_OK;
  }
  FAIL(h, SG_E_INVALID, "sg_set_option: unknown option %d", option);
}

extern "C" int sg_get_option(const sg_handle* h, int32_t option, int64_t* value) {
  if (!h || !value) return SG_E_INVALID;
  switch (option) {
    case SG_OPT_FORCE_UNFUSED: *value = h->force_unfused; return SG_OK;
    case SG_OPT_FORCE_NOFAST: *value = h->force_nofast; return SG_OK;
    case SG_OPT_FORCE_F64_DECIDE: *value = h->force_f64_decide; return SG_OK;
    case SG_OPT_FORCE_NOSEAM: *value = h->force_noseam; return SG_OK;
    case SG_OPT_FORCE_NOLEAN: *value = h->force_nolean; return SG_OK;
    case SG_OPT_FORCE_SPLIT: *value = h->force_split; return SG_OK;
    case SG_OPT_FAST_INTEGER: *value = h->fast_integer; return SG_OK;
    case SG_OPT_FORCE_EXACT: *value = h->force_exact; return SG_OK;
    case SG_OPT_FORCE_NOROWGATE: *value = h->rowgate_mode; return SG_OK;
    case SG_OPT_ROWGATE_TAP: *value = h->rg_tap; return SG_OK;
    case SG_OPT_ROWGATE_SHAPE: *value = h->rg_shape; return SG_OK;
    case SG_OPT_INJECT_HANDOFF_FAULT: *value = h->inject_fault; return SG_OK;
    case SG_OPT_TILE_ORDER: *value = h->tile_order; return SG_OK;
    case SG_OPT_EXACT_MATERIALISED: *value = h->exact_materialised; return SG_OK;
    case SG_OPT_STATS_THREE_LAUNCH: *value = h->stats_three; return SG_OK;
    case SG_OPT_FLOOR_TWO_LAUNCH: *value = h->floor_two; return SG_OK;
    case SG_OPT_FLOOR_TEST: *value = h->floor_test; return SG_OK;
  }
  return SG_E_INVALID;   // (no message: the handle is const here)
}

extern "C" int sg_profile_enable(sg_handle* h, int32_t on) {
  if (!h) return SG_E_INVALID;
  h->prof_on = on != 0;
  return SG_OK;
}

extern "C" int sg_profile_select(sg_handle* h, int64_t stage_mask) {
  if (!h) return SG_E_INVALID;
  h->prof_mask = stage_mask == 0 ? ~0ull : (uint64_t)stage_mask;
  return SG_OK;
}

extern "C" int sg_profile_read(sg_handle* h, double* ms, int64_t* counts, int32_t n_stages, int32_t reset) {
  if (!h) return SG_E_INVALID;
  if (n_stages != SG_N_STAGES && n_stages != SG_N_STAGES_ALL)
    FAIL(h, SG_E_INVALID, "sg_profile_read: n_stages must be %d (or %d)", SG_N_STAGES, SG_N_STAGES_ALL);
  for (auto& r : h->prof_live) {
    HIPCHK(h, hipEventSynchronize(r.b));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, r.a, r.b));
    h->prof_ms[r.stage] += (double)t;
    h->prof_cnt[r.stage] += 1;
    h->prof_pool.push_back(r.a);
    h->prof_pool.push_back(r.b);
  }
  h->prof_live.clear();
  for (int i = 0; i < SG_N_STAGES_ALL; ++i) {
    if (ms && i < n_stages) ms[i] = h->prof_ms[i];
    if (counts && i < n_stages) counts[i] = h->prof_cnt[i];
    if (reset) { h->prof_ms[i] = 0; h->prof_cnt[i] = 0; }
  }
  return SG_OK;
}

extern "C" const char* sg_stage_name(int32_t stage) {
  static const char* names[SG_N_STAGES_ALL] = {"k_channel_mean", "k_stft<double> (power)", "k_colmax", "k_colstats",
                                           "k_decide", "k_mag_fast* / k_stft<float> (magnitude)",
                                           "k_box_mask / k_iir_sigmoid / k_boxcar_sigmoid (non-stationary mask, other paths)",
                                           "mask smoothing (k_smooth_bits2 / k_smooth_tiled / k_smooth_f+k_smooth_t)",
                                           "k_apply_istft", "k_ola",
                                           "noise statistics (all kernels)", "k_unit_absmax+k_prep_thresh",
                                           "k_stft_bits<max> (floor pre-pass)", "k_stft_bits<decide>",
                                           "k_apply_fast (fft+mask+ifft+ola)",
                                           "k_decide_fast (f32 stft + exact f64 refine)",
                                           "k_gate_onepass (fft+decide+smooth+mask+ifft+ola)",
                                           "k_row_gate (fft+row stats+decide+smooth+mask+ifft+ola)",
                                           "k_iir_chain_par (tile carries; serial: k_iir_part / k_iir_comb + k_iir_chain)",
                                           "k_iir_mask<nt> (recurrence+sigmoid+smoothing)",
                                           "k_rg_noise_power (clips: noise transform)",
                                           "k_rg_noise_final (clips: thresholds)",
                                           "k_rg_decide (clips: transform + bits / magnitudes)",
                                           "k_rg_iir (clips: recurrence + sigmoid)",
                                           "k_rg_fsmooth (clips: frequency smoothing)",
                                           "k_rg_apply (clips: time smoothing + mask + inverse transform)",
                                           "k_rg_ola (clips: overlap-add)",
                                           "k_st_export (stream state -> payload)",
                                           "k_st_import (payload -> stream state)"};
  return (stage >= 0 && stage < SG_N_STAGES_ALL) ? names[stage] : "?";
}

extern "C" int sg_debug_dims(const sg_handle* h, int64_t dims[3]) {
  if (!h || !dims) return SG_E_INVALID;
  dims[0] = h->last.units; dims[1] = h->last.T; dims[2] = h->FS;
  return SG_OK;
}

extern "C" int sg_debug_range(const sg_handle* h, int64_t range[2]) {
  if (!h || !range) return SG_E_INVALID;
  range[0] = h->last.db; range[1] = h->last.de;
  return SG_OK;
}

extern "C" int sg_debug_counter(sg_handle* h, int32_t which, int64_t* value, void* stream) {
  if (!h || !value) return SG_E_INVALID;
  if (which == 1 || which == 2) {   // host counters: one-pass gate calls with the in-kernel (1) / a-priori (2) floor test
    *value = which == 1 ? h->n_floor_lazy : h->n_floor_apriori;
    return SG_OK;
  }
  if (which == 17) {   // SG_SMOOTH_* of the last smoothing launch | cell bytes << 8 | tile frames << 16 (host bookkeeping)
    *value = h->smooth_route;
    return SG_OK;
  }
  if (which == 18) {   // SG_SPEC_* of the last sg_gate_spectrum call | flags | sub-batches << 16 (host bookkeeping)
    *value = h->spec_route;
    return SG_OK;
  }
  if (which == 19) {   // SG_STATS_* form of the last noise statistics of fewer than 16 units (host bookkeeping)
    *value = h->stats_route;
    return SG_OK;
  }
  if (which == 20) {   // SG_FLOOR_* form of the last one-pass gate call's floor fix-up (host bookkeeping)
    *value = h->floor_route;
    return SG_OK;
  }
  if (which == 3) {   // launch epoch of the last gate call in which a chunk's floor test fired / flag was set (0: never)
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    *value = h->err_host ? (int64_t)h->err_host[1] : 0;
    return SG_OK;
  }
  if (which == 8) {   // the OP_TRACE development build keeps its buffer next to the gate (api.hip); the product library goes on to the error block
    int rc = SG_OK;
    if (onepass_dev_counter(h, which, value, (hipStream_t)stream, &rc)) return rc;
  }
  if (which >= 4 && which <= 15) {   // word `which` of the host-mapped error block (diagnosis builds of the persistent gate wrote them; 0 now)
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    *value = h->err_host ? (int64_t)h->err_host[which] : 0;
    return SG_OK;
  }
  if (which != 0) FAIL(h, SG_E_INVALID, "sg_debug_counter: unknown counter %d", which);
  *value = 0;
  if (!h->rg_count.p) return SG_OK;
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  unsigned v = 0;
  HIPCHK(h, hipMemcpy(&v, h->rg_count.p, sizeof(v), hipMemcpyDeviceToHost));
  *value = (int64_t)v;
  return SG_OK;
}

extern "C" int sg_debug_fetch(sg_handle* h, int32_t what, void* host, int64_t bytes, void* stream) {
  if (!h) return SG_E_INVALID;
  if (what == 5) {   // the gate's compare constants of the last noise statistics: T2 double[F], then the 64 words of the alim block
    if (!host || !h->t2_ready) FAIL(h, SG_E_STATE, "sg_debug_fetch: no compare constants from noise statistics");
    if ((size_t)bytes != (size_t)h->F * 8 + 256) FAIL(h, SG_E_INVALID, "sg_debug_fetch: need %zu bytes, got %lld", (size_t)h->F * 8 + 256, (long long)bytes);
    HIPCHK(h, hipMemcpyAsync(host, h->T2.p, (size_t)h->F * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(h, hipMemcpyAsync((char*)host + (size_t)h->F * 8, h->alim.p, 256, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    return SG_OK;
  }
  if (!host || h->last.units == 0) FAIL(h, SG_E_STATE, "sg_debug_fetch: nothing processed yet");
  size_t cells = (size_t)h->last.units * h->last.T * h->FS;
  const void* src;
  size_t need;
  switch (what) {
    case 0:
      if (h->last.fused) FAIL(h, SG_E_STATE, "fused path keeps the raw mask as bits: fetch field 3");
      if (!h->last.has_raw)
        FAIL(h, SG_E_STATE, "the one-kernel non-stationary mask does not materialise the raw mask: set SG_OPT_FORCE_UNFUSED");
      src = h->raw.p; need = cells * 4; break;
    case 3:
      if (!h->last.fused) FAIL(h, SG_E_STATE, "bit field only exists on the fused path");
      src = h->bits.p; need = (size_t)h->last.units * h->last.T * ((h->F + 63) / 64) * 8; break;
    case 1:
      if (h->last.fast && h->last.fused)
        FAIL(h, SG_E_STATE, "fast path keeps the smoothed mask as uint16 counts in the apply kernel's lane order");
      if (h->last.fused && h->last.k16_only) {
        // the apply kernel read the K counts directly: expand them now (api.hip)
        if (int rc = expand_k16_mask(h, cells, (hipStream_t)stream)) return rc;
      }
      src = h->M.p; need = cells * 4; break;
    case 2:
      if (!h->last.has_P) FAIL(h, SG_E_STATE, "power field only exists for stationary gates");
      src = h->P.p; need = cells * 8; break;
    case 4:
      if (!h->last.rg || !h->rg_tap) FAIL(h, SG_E_STATE, "row-gate power tile: set SG_OPT_ROWGATE_TAP and run TorchGate.forward");
      src = h->M.p; need = (size_t)h->last.units * 64 * fast::RG_PP * 4; break;
    default: FAIL(h, SG_E_INVALID, "sg_debug_fetch: unknown field %d", what);
  }
  if ((size_t)bytes != need) FAIL(h, SG_E_INVALID, "sg_debug_fetch: need %zu bytes, got %lld", need, (long long)bytes);
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  { int rc = handoff_verdict(h); if (rc) return rc; }
  if (what == 3 && h->last.xbits) {
    // one-pass path: the bits live tile-blocked in the exchange buffer [unit][tile][16][9]; rearrange into
    // the natural [unit][T][wpr] layout (frames outside sg_debug_range stay zero)
    const int wpr = (h->F + 63) / 64;
    const int TW = h->last.tiles.words ? h->last.tiles.words : fast::OP_TILE_WORDS, XW = h->last.tiles.xw;
    const size_t words = (size_t)h->last.units * h->last.tiles.ntt * TW;
    std::vector<unsigned long long> tmp(words);
    HIPCHK(h, hipMemcpy(tmp.data(), h->xbits.p, words * 8, hipMemcpyDeviceToHost));
    unsigned long long* dst = (unsigned long long*)host;
    std::memset(dst, 0, need);
    for (int64_t u = 0; u < h->last.units; ++u)
      for (int64_t j = 0; j < h->last.tiles.ntt; ++j)
        for (int i = 0; i < h->last.tiles.rows; ++i) {
          const int64_t t = h->last.tiles.f0 + (j - 1) * h->last.tiles.step + i;
          if (t < 0 || t >= h->last.T) continue;
          for (int w = 0; w < wpr; ++w)
          {
            const unsigned long long* gr = &tmp[((size_t)u * h->last.tiles.ntt + j) * TW + (i * XW + w) * 2];
            dst[(u * h->last.T + t) * wpr + w] = (gr[0] & 0xffffffffull) | (gr[1] << 32);
          }
        }
    return SG_OK;
  }
  HIPCHK(h, hipMemcpy(host, src, need, hipMemcpyDeviceToHost));
  return SG_OK;
}

extern "C" int sg_debug_clip_thresholds(sg_handle* h, double* host, int32_t n_noise, int32_t n_bins, void* stream) {
  if (!h || !host || n_bins != h->F) return SG_E_INVALID;
  return sg::rg_thresholds(h->rg, host, n_noise, n_bins, (hipStream_t)stream, &h->err);
}

extern "C" int sg_debug_clip_batches(const sg_handle* h, int64_t* value) {
  if (!h || !value) return SG_E_INVALID;
  *value = sg::rg_last_batches(h->rg);
  return SG_OK;
}

extern "C" int sg_debug_rows_batches(const sg_handle* h, int64_t* value) {
  if (!h || !value) return SG_E_INVALID;
  *value = sg::rw_last_batches(h->rw);
  return SG_OK;
}

extern "C" int sg_debug_backward_route(const sg_handle* h, int64_t* value) {
  if (!h || !value) return SG_E_INVALID;
  *value = h->dbg_bwd_route;
  return SG_OK;
}
