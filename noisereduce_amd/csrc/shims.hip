// libmi355gate.so -- the C entry points that check their arguments and forward to a table-driven unit:
// ragged batches (ragged.hip), padded batches of different-length rows (rows.hip), banks of live streams (stream.hip).
// Host code only: no kernels.
#include "handle.hpp"
#include "stream.hpp"

using namespace sg;
using namespace sg::host;

static bool rg_variant_ok(sg_handle* h) {
  if (h->p.variant != SG_VARIANT_S) { h->err = "sg_process_clips is a variant-S entry point"; return false; }
  return true;
}

extern "C" int sg_clips_workspace_bytes(const sg_handle* h, const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips,
                                        int64_t n_clips, int64_t* bytes) {
  if (!h || !bytes || n_clips < 0 || (n_clips > 0 && !clips) || n_noise < 0 || (n_noise > 0 && !noise)) return SG_E_INVALID;
  sg_handle* hm = const_cast<sg_handle*>(h);
  if (!rg_variant_ok(hm)) return SG_E_INVALID;
  return sg::rg_workspace_bytes(rg_ctx(hm), noise, n_noise, clips, n_clips, bytes, &hm->err);
}

extern "C" int sg_process_clips(sg_handle* h, const void* x_dev, int in_dtype, const void* noise_dev, int noise_dtype,
                                const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips,
                                void* out_dev, int out_dtype, int64_t max_workspace_bytes, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!rg_variant_ok(h)) return SG_E_INVALID;
  if (n_clips < 0 || (n_clips > 0 && (!clips || !x_dev || !out_dev)) || !dtype_ok(in_dtype) || !dtype_ok(out_dtype) ||
      n_noise < 0 || (n_noise > 0 && !noise) || (h->p.stationary && n_noise > 0 && !dtype_ok(noise_dtype) && noise_dev))
    FAIL(h, SG_E_INVALID, "sg_process_clips: bad argument");
  if (n_clips == 0) return SG_OK;
  return sg::rg_process(&h->rg, rg_ctx(h), x_dev, in_dtype, noise_dev, noise_dtype, noise, n_noise, clips, n_clips, out_dev,
                        out_dtype, max_workspace_bytes, (hipStream_t)stream, &h->err);
}

// ---- padded batches of different-length rows: thin wrappers over rows.hip ---------------------------------------------
static int64_t rw_budget(const sg_handle* h) { return h->p.max_workspace_bytes > 0 ? h->p.max_workspace_bytes : 0; }

extern "C" int sg_process_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                               const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                               const int64_t* xn_lengths, void* out_dev, int out_dtype, int64_t out_stride,
                               float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_process_rows")) return rc;
  if (!x_dev || !out_dev || (dtype != SG_F32 && dtype != SG_F64) || (out_dtype != SG_F32 && out_dtype != SG_F64) || B < 1 ||
      x_stride < L || out_stride < 0)
    FAIL(h, SG_E_INVALID, "sg_process_rows: bad argument");
  if (int rc = t_min_lengths(h, B, L, xn_dev, Bn, Ln)) return rc;
  return sg::rw_process(&h->rw, rg_ctx(h), h->p.n_movemean, x_dev, dtype, B, L, x_stride, lengths, xn_dev, Bn, Ln, xn_stride,
                        xn_lengths, out_dev, out_dtype, out_stride, mask_out_dev, rw_budget(h), (hipStream_t)stream, &h->err);
}

extern "C" int sg_process_rows_backward(sg_handle* h, const void* grad_out_dev, int dtype, int64_t B, int64_t L,
                                        int64_t go_stride, const int64_t* lengths, const float* mask_dev, void* grad_x_dev,
                                        int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_process_rows_backward")) return rc;
  if (!grad_out_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64) || gx_stride < L ||
      L < 2 * (int64_t)h->W)
    FAIL(h, SG_E_INVALID, "sg_process_rows_backward: bad argument");
  h->dbg_bwd_route = SG_BWD_ROWS;
  return sg::rw_backward(&h->rw, rg_ctx(h), grad_out_dev, dtype, B, L, go_stride, lengths, mask_dev, grad_x_dev, gx_stride,
                         rw_budget(h), (hipStream_t)stream, &h->err);
}

// TorchGate.gated_stft(lengths=): the rows pipeline with the masked spectrum stored instead of inverted (rows.hpp)
extern "C" int sg_gate_spectrum_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                     const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                                     const int64_t* xn_lengths, void* spec_dev, float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_gate_spectrum_rows")) return rc;
  if (!x_dev || !spec_dev || (dtype != SG_F32 && dtype != SG_F64) || B < 1 || x_stride < L)
    FAIL(h, SG_E_INVALID, "sg_gate_spectrum_rows: bad argument");
  if (int rc = t_min_lengths(h, B, L, xn_dev, Bn, Ln)) return rc;
  return sg::rw_spectrum(&h->rw, rg_ctx(h), h->p.n_movemean, x_dev, dtype, B, L, x_stride, lengths, xn_dev, Bn, Ln, xn_stride,
                         xn_lengths, spec_dev, mask_out_dev, rw_budget(h), (hipStream_t)stream, &h->err);
}

extern "C" int sg_gate_spectrum_rows_backward(sg_handle* h, const void* grad_spec_dev, int dtype, int64_t B, int64_t L,
                                              const int64_t* lengths, const float* mask_dev, void* grad_x_dev,
                                              int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_gate_spectrum_rows_backward")) return rc;
  if (!grad_spec_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64) || gx_stride < L ||
      L < 2 * (int64_t)h->W)
    FAIL(h, SG_E_INVALID, "sg_gate_spectrum_rows_backward: bad argument");
  return sg::rw_spectrum_backward(&h->rw, rg_ctx(h), grad_spec_dev, dtype, B, L, lengths, mask_dev, grad_x_dev, gx_stride,
                                  rw_budget(h), (hipStream_t)stream, &h->err);
}

// TorchGate.gated_filterbank(lengths=): the rows pipeline with the features of the masked frame stored instead of the
// frame (rows.hpp; the bank is sg_set_filterbank's)
extern "C" int sg_gate_features_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                     const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                                     const int64_t* xn_lengths, int32_t power, int32_t take_log, double eps,
                                     void* feat_dev, float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_gate_features_rows")) return rc;
  if (!x_dev || !feat_dev || (dtype != SG_F32 && dtype != SG_F64) || B < 1 || x_stride < L)
    FAIL(h, SG_E_INVALID, "sg_gate_features_rows: bad argument");
  if (int rc = features_args_ok(h, "sg_gate_features_rows", power, eps)) return rc;
  if (int rc = t_min_lengths(h, B, L, xn_dev, Bn, Ln)) return rc;
  return sg::rw_features(&h->rw, rg_ctx(h), h->p.n_movemean, feat_bank(h), x_dev, dtype, B, L, x_stride, lengths, xn_dev, Bn,
                         Ln, xn_stride, xn_lengths, power, take_log != 0, eps, feat_dev, mask_out_dev, rw_budget(h),
                         (hipStream_t)stream, &h->err);
}

extern "C" int sg_gate_features_rows_backward(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L,
                                              int64_t x_stride, const int64_t* lengths, const void* grad_feat_dev,
                                              const float* mask_dev, int32_t power, int32_t take_log, double eps,
                                              void* grad_x_dev, int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_gate_features_rows_backward")) return rc;
  if (!x_dev || !grad_feat_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64) || x_stride < L ||
      gx_stride < L)
    FAIL(h, SG_E_INVALID, "sg_gate_features_rows_backward: bad argument");
  if (int rc = features_args_ok(h, "sg_gate_features_rows_backward", power, eps)) return rc;
  if (L < 2 * (int64_t)h->W) FAIL(h, SG_E_INVALID, "x must be bigger than %d", 2 * h->W);
  return sg::rw_features_backward(&h->rw, rg_ctx(h), feat_bank(h), x_dev, dtype, B, L, x_stride, lengths, grad_feat_dev,
                                  mask_dev, power, take_log != 0, eps, grad_x_dev, gx_stride, rw_budget(h),
                                  (hipStream_t)stream, &h->err);
}

// ---- banks of live streams: thin wrappers over stream.hip --------------------------------------------------------------
struct sg_stream_bank {
  sg_handle* h;
  sg::StBank* b;
};

// the one create call behind the four entry points; `who` names the caller in the variant message
// A handle of variant T streams its non-stationary gate alone (a box bank): kind
// SG_STREAM_NONSTATIONARY, the moving mean's n_movemean frames deciding the lookahead.  0: the handle is of variant S.
static int stream_box_check(sg_handle* h, const sg_stream_desc& d, const char* who) {
  if (h->p.stationary)
    FAIL(h, SG_E_INVALID, "%s: a variant-T handle streams its non-stationary gate only (this one is stationary: its noise "
         "statistics need the whole recording or xn)", who);
  if (d.kind != SG_STREAM_NONSTATIONARY)
    FAIL(h, SG_E_INVALID, "%s: a variant-T handle takes kind SG_STREAM_NONSTATIONARY only (got kind %d)", who, d.kind);
  if (h->W & 1)
    FAIL(h, SG_E_INVALID, "%s: a variant-T handle streams with an even win_length only (got %d: the stream's frames would "
         "not be the samples torch.stft windows)", who, h->W);
  if (h->p.n_movemean < 1 || h->p.n_movemean > SG_STREAM_MAX_LOOKAHEAD)
    FAIL(h, SG_E_INVALID, "%s: n_movemean must be 1 .. %d on a variant-T handle (got %d)", who, SG_STREAM_MAX_LOOKAHEAD,
         h->p.n_movemean);
  if (d.lookahead_frames != 0)
    FAIL(h, SG_E_INVALID, "%s: lookahead_frames must be 0 on a variant-T handle (n_movemean = %d decides it: %d frames)", who,
         h->p.n_movemean, h->p.n_movemean - 1 - (h->p.n_movemean - 1) / 2);
  return SG_OK;
}

// (a variant-T handle makes its box bank through sg_stream_create_ex alone: the three older entry points answer it as before)
static int stream_create(sg_handle* h, const sg_stream_desc& d, const char* who, sg_stream_bank** out, bool ex = false) {
  const bool box = h->p.variant != SG_VARIANT_S;
  if (box && !ex) FAIL(h, SG_E_INVALID, "%s is a variant-S entry point", who);
  if (box) {
    int rc = stream_box_check(h, d, who);
    if (rc) return rc;
  }
  sg::StBank* b = nullptr;
  const sg::StAdaptive ad{d.forget, d.learn_frames};
  const bool ns = d.kind == SG_STREAM_NONSTATIONARY;
  int rc = sg::st_create(&b, rg_ctx(h), d.n_slots, d.channels, d.max_block, ns, ns ? d.lookahead_frames : 0,
                         d.kind == SG_STREAM_ADAPTIVE ? &ad : nullptr, d.exact != 0, &h->err, box ? h->p.n_movemean : 0);
  if (rc) return rc;
  *out = new sg_stream_bank{h, b};
  return SG_OK;
}

// the one size call behind the three entry points
static int64_t stream_state_bytes(const sg_handle* h, bool ns, int64_t n_slots, int64_t channels, int64_t max_block, int64_t L,
                                  bool adaptive, bool exact, int32_t box_k = 0) {
  return sg::st_state_bytes(rg_ctx(const_cast<sg_handle*>(h)), ns, n_slots, channels, max_block, L, adaptive, exact, box_k);
}

extern "C" int sg_stream_create_ex(sg_handle* h, const sg_stream_desc* desc, sg_stream_bank** out) {
  if (!h || !out) return SG_E_INVALID;
  if (!desc) FAIL(h, SG_E_INVALID, "sg_stream_create_ex: desc is null");
  if (desc->kind != SG_STREAM_FIXED && desc->kind != SG_STREAM_NONSTATIONARY && desc->kind != SG_STREAM_ADAPTIVE)
    FAIL(h, SG_E_INVALID, "sg_stream_create_ex: unknown kind %d", desc->kind);
  return stream_create(h, *desc, "sg_stream_create_ex", out, true);
}

extern "C" int sg_stream_state_bytes_ex(const sg_handle* h, const sg_stream_desc* d, int64_t* bytes) {
  if (!h || !d || !bytes || d->n_slots < 1 || d->channels < 1 || d->max_block < 1) return SG_E_INVALID;
  const bool ns = d->kind == SG_STREAM_NONSTATIONARY, ad = d->kind == SG_STREAM_ADAPTIVE;
  if (h->p.variant != SG_VARIANT_S) {   // (the box bank: the one a variant-T handle creates)
    if (int rc = stream_box_check(const_cast<sg_handle*>(h), *d, "sg_stream_state_bytes_ex")) return rc;
    *bytes = stream_state_bytes(h, true, d->n_slots, d->channels, d->max_block, 0, false, d->exact != 0, h->p.n_movemean);
    return SG_OK;
  }
  if ((!ns && !ad && d->kind != SG_STREAM_FIXED) || (ns && d->lookahead_frames < 0) || ns == (h->p.stationary != 0))
    return SG_E_INVALID;
  *bytes = stream_state_bytes(h, ns, d->n_slots, d->channels, d->max_block, ns ? d->lookahead_frames : 0, ad, d->exact != 0);
  return SG_OK;
}

extern "C" int sg_stream_create(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block, sg_stream_bank** out) {
  if (!h || !out) return SG_E_INVALID;
  sg_stream_desc d{};
  d.n_slots = n_slots; d.channels = channels; d.max_block = max_block; d.kind = SG_STREAM_FIXED;
  return stream_create(h, d, "sg_stream_create", out);
}

extern "C" int sg_stream_create_nonstationary(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                              int32_t lookahead_frames, sg_stream_bank** out) {
  if (!h || !out) return SG_E_INVALID;
  sg_stream_desc d{};
  d.n_slots = n_slots; d.channels = channels; d.max_block = max_block; d.kind = SG_STREAM_NONSTATIONARY;
  d.lookahead_frames = lookahead_frames;
  return stream_create(h, d, "sg_stream_create_nonstationary", out);
}

extern "C" int sg_stream_state_bytes(const sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                     int32_t lookahead_frames, int64_t* bytes) {
  if (!h || !bytes || n_slots < 1 || channels < 1 || max_block < 1 || lookahead_frames < 0) return SG_E_INVALID;
  *bytes = stream_state_bytes(h, !h->p.stationary, n_slots, channels, max_block, h->p.stationary ? 0 : lookahead_frames, false, false);
  return SG_OK;
}

extern "C" int sg_stream_create_adaptive(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block, double forget,
                                         int64_t learn_frames, sg_stream_bank** out) {
  if (!h || !out) return SG_E_INVALID;
  sg_stream_desc d{};
  d.n_slots = n_slots; d.channels = channels; d.max_block = max_block; d.kind = SG_STREAM_ADAPTIVE;
  d.forget = forget; d.learn_frames = learn_frames;
  return stream_create(h, d, "sg_stream_create_adaptive", out);
}

extern "C" int sg_stream_state_bytes_adaptive(const sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                              int64_t* bytes) {
  if (!h || !bytes || n_slots < 1 || channels < 1 || max_block < 1 || !h->p.stationary) return SG_E_INVALID;
  *bytes = stream_state_bytes(h, false, n_slots, channels, max_block, 0, true, false);
  return SG_OK;
}

extern "C" int sg_stream_noise_profile(sg_stream_bank* b, int32_t slot, double* thresh_host, int32_t n_bins, void* stream) {
  if (!b) return SG_E_INVALID;
  sg_handle* h = b->h;
  if (!thresh_host) FAIL(h, SG_E_INVALID, "sg_stream_noise_profile: thresh_host is null");
  if (n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_stream_noise_profile: n_bins must be %d", h->F);
  return sg::st_noise_profile(b->b, slot, thresh_host, (hipStream_t)stream, &h->err);
}

extern "C" int sg_stream_bank_emitted(const sg_stream_bank* b, int64_t n, int64_t* emitted) {
  if (!b || !emitted || n < 0) return SG_E_INVALID;
  *emitted = sg::st_bank_emitted(b->b, n);
  return SG_OK;
}

extern "C" int sg_stream_destroy(sg_stream_bank* b) {
  if (!b) return SG_OK;
  sg::st_destroy(b->b);
  delete b;
  return SG_OK;
}

extern "C" int sg_stream_set_threshold(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, const double* thresh_host,
                                       int32_t n_bins, void* stream) {
  if (!b) return SG_E_INVALID;
  sg_handle* h = b->h;
  if (n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_stream_set_threshold: n_bins must be %d", h->F);
  if (!thresh_host && !h->has_thresh) FAIL(h, SG_E_STATE, "no noise threshold set");
  return sg::st_set_threshold(b->b, slots, n_slots, thresh_host ? nullptr : (const double*)h->thresh.p, thresh_host,
                              (hipStream_t)stream, &h->err);
}

extern "C" int sg_stream_push(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                              const sg_stream_rec* recs, int32_t n_recs, void* stream) {
  if (!b) return SG_E_INVALID;
  sg_handle* h = b->h;
  // (the sample codes an exact bank takes beyond float32 / float64 are st_push's to check: it knows the bank)
  if (n_recs < 0 || (n_recs > 0 && !recs) || !dtype_ok(in_dtype) || !dtype_ok(out_dtype))
    FAIL(h, SG_E_INVALID, "sg_stream_push: bad argument (float32 / float64 buffers)");
  return sg::st_push(b->b, in_dev, in_dtype, out_dev, out_dtype, recs, n_recs, (hipStream_t)stream, &h->err);
}

extern "C" int sg_stream_push_spectrum(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                                       void* spec_dev, int spec_dtype, void* mask_dev, const sg_stream_rec* recs,
                                       const sg_stream_spec_rec* spec_recs, int32_t n_recs, void* stream) {
  if (!b) return SG_E_INVALID;
  sg_handle* h = b->h;
  if (n_recs < 0 || (n_recs > 0 && !recs) || !dtype_ok(in_dtype) || !dtype_ok(out_dtype))
    FAIL(h, SG_E_INVALID, "sg_stream_push_spectrum: bad argument (float32 / float64 buffers)");
  const sg::StSpecOut so{spec_dev, spec_dtype, mask_dev, spec_recs};
  return sg::st_push(b->b, in_dev, in_dtype, out_dev, out_dtype, recs, n_recs, (hipStream_t)stream, &h->err, &so);
}

// the stream bank's own filterbank (sg_set_filterbank above is a variant-T entry point: t_entry refuses this handle)
extern "C" int sg_stream_set_filterbank(sg_stream_bank* b, const float* fb_host, int32_t n_filters) {
  if (!b) return SG_E_INVALID;
  return sg::st_set_filterbank(b->b, fb_host, n_filters, &b->h->err);
}

extern "C" int sg_stream_push_features(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                                       void* feat_dev, int feat_dtype, void* mask_dev, int32_t power, int32_t take_log,
                                       double eps, double scale, const sg_stream_rec* recs,
                                       const sg_stream_feat_rec* feat_recs, int32_t n_recs, void* stream) {
  if (!b) return SG_E_INVALID;
  sg_handle* h = b->h;
  if (n_recs < 0 || (n_recs > 0 && !recs) || !dtype_ok(in_dtype) || !dtype_ok(out_dtype))
    FAIL(h, SG_E_INVALID, "sg_stream_push_features: bad argument (float32 / float64 buffers)");
  const sg::StFeatOut fo{feat_dev, feat_dtype, mask_dev, feat_recs, power, take_log, eps, scale};
  return sg::st_push(b->b, in_dev, in_dtype, out_dev, out_dtype, recs, n_recs, (hipStream_t)stream, &h->err, nullptr, &fo);
}

extern "C" int sg_stream_bank_frames(const sg_stream_bank* b, int64_t n, int64_t* frames) {
  if (!b || !frames || n < 0) return SG_E_INVALID;
  *frames = sg::st_bank_frames(b->b, n);
  return SG_OK;
}

extern "C" int sg_stream_reset(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, void* stream) {
  if (!b) return SG_E_INVALID;
  return sg::st_reset(b->b, slots, n_slots, (hipStream_t)stream, &b->h->err);
}

extern "C" int sg_stream_emitted(const sg_handle* h, int64_t n, int64_t* emitted) {
  if (!h || !emitted || n < 0) return SG_E_INVALID;
  *emitted = sg::st_emitted(h->W, h->H, h->p.smooth_mask ? h->p.n_grad_time : 0, n);
  return SG_OK;
}

extern "C" int sg_stream_counters(const sg_stream_bank* b, int32_t slot, int64_t* n, int64_t* emitted) {
  if (!b || !n || !emitted) return SG_E_INVALID;
  return sg::st_counters(b->b, slot, n, emitted, &b->h->err);
}

// the handle's part of a stream state's signature (the bank's part is stream.hip's)
static sg_stream_head stream_signature(const sg_handle* h) {
  sg_stream_head s{};
  s.n_fft = h->p.n_fft; s.win_length = h->W; s.hop_length = h->H;
  s.n_grad_freq = h->p.n_grad_freq; s.n_grad_time = h->p.n_grad_time; s.smooth_mask = h->p.smooth_mask ? 1 : 0;
  s.prop_decrease = h->p.prop_decrease; s.n_std_thresh = h->p.n_std_thresh; s.top_db = h->p.top_db;
  s.iir_b = h->p.iir_b; s.nonstat_thresh = h->p.nonstat_thresh; s.nonstat_slope = h->p.nonstat_slope;
  return s;
}

extern "C" int sg_stream_export_bytes(const sg_stream_bank* b, int32_t slot, int64_t* bytes) {
  if (!b || !bytes) return SG_E_INVALID;
  return sg::st_export_bytes(b->b, slot, bytes, &b->h->err);
}

extern "C" int sg_stream_head_bytes(const sg_stream_head* head, int64_t* bytes) {
  if (!head || !bytes) return SG_E_INVALID;
  return sg::st_head_bytes(*head, bytes);
}

extern "C" int sg_stream_export(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, void* blob_dev, const int64_t* offsets,
                                sg_stream_head* heads_out, void* stream) {
  if (!b) return SG_E_INVALID;
  return sg::st_export(b->b, slots, n_slots, blob_dev, offsets, stream_signature(b->h), heads_out, (hipStream_t)stream, &b->h->err);
}

extern "C" int sg_stream_import(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, const void* blob_dev,
                                const int64_t* offsets, const sg_stream_head* heads_in, void* stream) {
  if (!b) return SG_E_INVALID;
  return sg::st_import(b->b, slots, n_slots, blob_dev, offsets, stream_signature(b->h), heads_in, (hipStream_t)stream, &b->h->err);
}
