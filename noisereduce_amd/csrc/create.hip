// libmi355gate.so -- the life of a handle: sg_create builds the tables of its geometry on the host and uploads them,
// sg_destroy releases them; the buffers, the cached dynamic-LDS limit and the profiler scope every host unit uses.
// Host code only: no kernels.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "handle.hpp"
#include "launch.hpp"
#include "fft_wave.hpp"   // cx
#include "limits.hpp"

using namespace sg;
using namespace sg::host;

namespace {
thread_local std::string g_create_error;

// Optional roctx ranges around every stage's enqueue (SG_ROCTX=1 in the environment at sg_create): the stages show
// up by name in `rocprofv3 --marker-trace` next to the kernel trace.  libroctx64 is looked up at run time: the library
// does not depend on it.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    // rocprofv3 listens to the rocprofiler-sdk flavour; libroctx64 is the roctracer one (older tools)
    void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(lib, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
const Roctx& roctx() {
  static const Roctx r;
  return r;
}
}  // namespace

namespace sg {
namespace host {

static hipEvent_t prof_event(sg_handle* h) {
  if (!h->prof_pool.empty()) {
    hipEvent_t e = h->prof_pool.back();
    h->prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
ProfScope::ProfScope(sg_handle* h_, int stage, hipStream_t st_) : h(h_), st(st_) {
  if (h->roctx_on && roctx().push) {
    roctx().push(sg_stage_name(h->prof_override >= 0 ? h->prof_override : stage));
    ranged = true;
  }
  if (!h->prof_on) return;
  const int booked = h->prof_override >= 0 ? h->prof_override : stage;
  if (!((h->prof_mask >> booked) & 1ull)) return;
  sg_handle::ProfRec r{h->prof_override >= 0 ? h->prof_override : stage, prof_event(h), prof_event(h)};
  (void)hipEventRecord(r.a, st);
  h->prof_live.push_back(r);
  idx = (int)h->prof_live.size() - 1;
}
ProfScope::~ProfScope() {
  if (idx >= 0) (void)hipEventRecord(h->prof_live[idx].b, st);
  if (ranged) roctx().pop();
}
void* rg_prof_begin(void* ctx, int stage, hipStream_t st) { return new ProfScope((sg_handle*)ctx, stage, st); }
void rg_prof_end(void* tok) { delete (ProfScope*)tok; }

// (launch.hpp) the one hipFuncSetAttribute(MaxDynamicSharedMemorySize) of the library
hipError_t set_lds(const void* kern, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = done[{dev, kern}];
  if (have >= bytes) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

int ensure(sg_handle* h, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes) return SG_OK;
  if (b.p) {
    HIPCHK(h, hipDeviceSynchronize());  // buffer may still be in use by enqueued work
    HIPCHK(h, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
  }
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    FAIL(h, SG_E_NOMEM, "workspace allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
  }
  b.bytes = bytes;
  return SG_OK;
}

int ensure_zeroed(sg_handle* h, DevBuf& b, size_t bytes, hipStream_t st, bool* fresh) {
  // freshness from the SIZE, not the pointer: the allocator may hand the freed address straight back
  const bool grow = b.bytes < bytes;
  int rc = ensure(h, b, bytes);
  if (rc) return rc;
  if (fresh) *fresh = grow;
  if (grow) HIPCHK(h, hipMemsetAsync(b.p, 0, b.bytes, st));
  return SG_OK;
}

int upload(sg_handle* h, DevBuf& b, const void* src, size_t bytes) {
  int rc = ensure(h, b, bytes);
  if (rc) return rc;
  HIPCHK(h, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return SG_OK;
}

}  // namespace host
}  // namespace sg

// ------------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------------
extern "C" int sg_version(void) { return SG_VERSION; }

extern "C" const char* sg_last_error(const sg_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static std::vector<double> triangle(int m) {
  // base.py:7-29 one axis: [1..m, m+1, m..1] / (m+1)
  std::vector<double> v(2 * m + 1);
  for (int i = 0; i <= 2 * m; ++i) v[i] = (double)(i <= m ? i + 1 : 2 * m + 1 - i) / (double)(m + 1);
  return v;
}

// Host radix-2 transform in long double (tables only)
static void host_fft(std::vector<long double>& br, std::vector<long double>& bi) {
  typedef long double ld;
  const ld PI = 3.14159265358979323846264338327950288L;
  const int M = (int)br.size();
  for (int i = 1, j = 0; i < M; ++i) {
    int bit = M >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(br[i], br[j]);
      std::swap(bi[i], bi[j]);
    }
  }
  for (int len = 2; len <= M; len <<= 1) {
    for (int k = 0; k < len / 2; ++k) {
      const ld a = -2.0L * PI * (ld)k / (ld)len;
      const ld wr = cosl(a), wi = sinl(a);
      for (int i = k; i < M; i += len) {
        const int j = i + len / 2;
        const ld xr = br[j] * wr - bi[j] * wi, xi = br[j] * wi + bi[j] * wr;
        br[j] = br[i] - xr;
        bi[j] = bi[i] - xi;
        br[i] += xr;
        bi[i] += xi;
      }
    }
  }
}

// Tables of the chirp-z kernels (czt.hpp) for a frame length n that is not a power of two:
// chirp conj(b[j]) = exp(-i pi j^2 / n) (j^2 reduced mod 2n in integers), B = FFT_M(b wrapped) / M
// (host radix-2 transform in long double), master twiddles w_{2M}^k of the M-point device core.
static int build_czt(sg_handle* h) {
  typedef long double ld;
  const ld PI = 3.14159265358979323846264338327950288L;
  const int n = h->n;
  int M = 64;
  while (M < 2 * n - 1) M *= 2;
  h->czt_M = M;
  std::vector<ld> br(M, 0.0L), bi(M, 0.0L), cr(n), ci(n);
  for (int j = 0; j < n; ++j) {
    const int64_t q = ((int64_t)j * j) % (2 * (int64_t)n);
    const ld a = PI * (ld)q / (ld)n;
    cr[j] = cosl(a);
    ci[j] = -sinl(a);
    br[j] = cr[j];
    bi[j] = -ci[j];
    if (j) {
      br[M - j] = br[j];
      bi[M - j] = bi[j];
    }
  }
  host_fft(br, bi);
  std::vector<cx<double>> tw64(M), ch64(n), bh64(M);
  std::vector<cx<float>> tw32(M), ch32(n), bh32(M);
  for (int k = 0; k < M; ++k) {
    const ld a = -PI * (ld)k / (ld)M;
    tw64[k] = {(double)cosl(a), (double)sinl(a)};
    tw32[k] = {(float)cosl(a), (float)sinl(a)};
    bh64[k] = {(double)(br[k] / (ld)M), (double)(bi[k] / (ld)M)};
    bh32[k] = {(float)(br[k] / (ld)M), (float)(bi[k] / (ld)M)};
  }
  for (int j = 0; j < n; ++j) {
    ch64[j] = {(double)cr[j], (double)ci[j]};
    ch32[j] = {(float)cr[j], (float)ci[j]};
  }
  int rc = upload(h, h->czt_tw64, tw64.data(), tw64.size() * sizeof(cx<double>));
  if (!rc) rc = upload(h, h->czt_ch64, ch64.data(), ch64.size() * sizeof(cx<double>));
  if (!rc) rc = upload(h, h->czt_bh64, bh64.data(), bh64.size() * sizeof(cx<double>));
  if (!rc) rc = upload(h, h->czt_tw32, tw32.data(), tw32.size() * sizeof(cx<float>));
  if (!rc) rc = upload(h, h->czt_ch32, ch32.data(), ch32.size() * sizeof(cx<float>));
  if (!rc) rc = upload(h, h->czt_bh32, bh32.data(), bh32.size() * sizeof(cx<float>));
  return rc;
}

// Tables of the long-frame kernels (big.hpp): w_M^j, the master twiddles of the M2-point row transform and, for a
// frame length that is not a power of two, the chirp exp(-i pi j^2 / n) and B = FFT_M(b wrapped) / M in the PERMUTED
// order pos(k) = (k & 15) * M2 + (k >> 4) the four-step transform leaves its output in.
static int build_big(sg_handle* h, bool pow2) {
  typedef long double ld;
  const ld PI = 3.14159265358979323846264338327950288L;
  const int n = h->n;
  int M = n;
  if (!pow2) {
    M = 16384;
    while (M < 2 * n - 1) M *= 2;
  }
  const int M2 = M / 16;
  h->big_M = M;
  h->big_czt = pow2 ? 0 : 1;
  std::vector<cx<double>> twM(M), tw2(M2);
  for (int j = 0; j < M; ++j) {
    const ld a = -2.0L * PI * (ld)j / (ld)M;
    twM[j] = {(double)cosl(a), (double)sinl(a)};
  }
  for (int k = 0; k < M2; ++k) {
    const ld a = -PI * (ld)k / (ld)M2;
    tw2[k] = {(double)cosl(a), (double)sinl(a)};
  }
  int rc = upload(h, h->big_twM, twM.data(), twM.size() * sizeof(cx<double>));
  if (!rc) rc = upload(h, h->big_tw2, tw2.data(), tw2.size() * sizeof(cx<double>));
  if (rc || pow2) return rc;
  std::vector<ld> br(M, 0.0L), bi(M, 0.0L);
  std::vector<cx<double>> ch(n), bh(M);
  for (int j = 0; j < n; ++j) {
    const int64_t q = ((int64_t)j * j) % (2 * (int64_t)n);
    const ld a = PI * (ld)q / (ld)n;
    ch[j] = {(double)cosl(a), (double)-sinl(a)};
    br[j] = cosl(a);
    bi[j] = sinl(a);
    if (j) {
      br[M - j] = br[j];
      bi[M - j] = bi[j];
    }
  }
  host_fft(br, bi);
  for (int k = 0; k < M; ++k)
    bh[(size_t)(k & 15) * M2 + (k >> 4)] = {(double)(br[k] / (ld)M), (double)(bi[k] / (ld)M)};
  rc = upload(h, h->big_ch, ch.data(), ch.size() * sizeof(cx<double>));
  if (!rc) rc = upload(h, h->big_bh, bh.data(), bh.size() * sizeof(cx<double>));
  return rc;
}

extern "C" int sg_create(const sg_params* p, const double* window_host, sg_handle** out) {
  if (!p || !out) {
    g_create_error = "sg_create: null argument";
    return SG_E_INVALID;
  }
  auto bad = [&](int code, const std::string& m) {
    g_create_error = m;
    return code;
  };
  int n = p->n_fft;
  // powers of two 64..8192 run on the Stockham kernels; every other length 4..4096 on the chirp-z
  // kernels (czt.hpp); longer frames -- powers of two up to 65536, any other length up to 32768 -- on the
  // four-step transform through HBM (big.hpp)
  const bool pow2 = n >= 64 && (n & (n - 1)) == 0;
  const bool bigf = (pow2 && n > 8192) || (!pow2 && n > 4096);
  if (n < 4 || (pow2 && n > 65536) || (!pow2 && n > 32768))
    return bad(SG_E_UNSUPPORTED,
               fmt("n_fft=%d unsupported: must be in [4, 32768], or a power of two up to 65536", n));
  if (p->win_length < 2 || p->win_length > n)
    return bad(SG_E_INVALID, fmt("win_length=%d must be in [2, n_fft=%d]", p->win_length, n));
  if (p->hop_length < 1 || p->hop_length > p->win_length)
    return bad(SG_E_INVALID, fmt("hop_length=%d must be in [1, win_length]", p->hop_length));
  if (p->variant != SG_VARIANT_S && p->variant != SG_VARIANT_T) return bad(SG_E_INVALID, "bad variant");
  if (p->smooth_mask && (p->n_grad_freq < 1 || p->n_grad_time < 1))
    return bad(SG_E_INVALID, "n_grad_freq / n_grad_time must be >= 1");
  if (p->variant == SG_VARIANT_S && (p->padding < 0 || p->chunk_size < 1))
    return bad(SG_E_INVALID, "chunk_size must be >= 1 and padding >= 0");
  if (!p->stationary && p->variant == SG_VARIANT_T && p->n_movemean < 1)
    return bad(SG_E_INVALID, "n_movemean must be >= 1");

  sg_handle* h = new sg_handle();
  h->p = *p;
  {
    const char* e = getenv("SG_ROCTX");
    h->roctx_on = e && e[0] == '1';
  }
  h->n = n;
  h->N = n / 2;
  h->W = p->win_length;
  h->H = p->hop_length;
  h->F = n / 2 + 1;
  h->FS = (h->F + 15) / 16 * 16;
  const int W = h->W;
  std::vector<double> w(W);
  if (window_host) {
    for (int k = 0; k < W; ++k) w[k] = window_host[k];
  } else {
    for (int k = 0; k < W; ++k) w[k] = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)W);
  }
  h->sum_w = 0.0;
  for (int k = 0; k < W; ++k) h->sum_w += w[k];
  for (int k = 0; k < W; ++k) h->sum_abs_w += std::fabs(w[k]);
  {
    int64_t a = p->smooth_mask ? (int64_t)(p->n_grad_freq + 1) * (p->n_grad_freq + 1) : 1;
    int64_t b = p->smooth_mask ? (int64_t)(p->n_grad_time + 1) * (p->n_grad_time + 1) : 1;
    h->ktot = a * b;
    // fused (bit-mask) path: variant-S stationary gate whose integer smoothing sums fit uint16
    // frame lengths 2 N, N a product of 2, 3, 5, 7, 11, 13: the mixed-radix kernels (mixed.hpp) -- and with them the fused
    // (bit-mask) path -- instead of chirp-z
    h->mr_ok = !pow2 && !bigf && n % 2 == 0 && n >= 8 && mr_make_plan(n / 2, &h->mr) && getenv("SG_NO_MIXED_RADIX") == nullptr;
    h->fused_ok = p->variant == SG_VARIANT_S && p->stationary && h->ktot <= 65535 && (pow2 || h->mr_ok) && n <= 4096 &&
                  (!p->smooth_mask || p->n_grad_time <= 96);
    // the integer smoothing kernel holds (tt + 2 nt) rows of all F bins in LDS: 64-frame tiles, lower ones for long rows
    // and wide time smoothing; returns the bytes of the tile it settled on
    auto fit_sm2_tile = [&](int tt_max) {
      const int wpr = (h->F + 63) / 64;
      const bool small = (p->n_grad_freq + 1) * (p->n_grad_freq + 1) <= 255;
      size_t lds = 0;
      for (h->sm2_tt = tt_max; h->sm2_tt >= 16; h->sm2_tt >>= 1) {
        const int rows = h->sm2_tt + 2 * p->n_grad_time;
        lds = smooth2_cf_bytes(rows + 2, h->F, small ? 1 : 2) + (size_t)rows * (wpr + 2) * 8 + 8192;
        if (lds <= 150 * 1024) break;
      }
      return lds;
    };
    if (h->fused_ok && p->smooth_mask) {
      if (fit_sm2_tile(smooth2_tt_max(h->F)) > 150 * 1024 || p->n_grad_freq > 30) h->fused_ok = false;
    }
    // variant T's bit-mask route (sg_process_batch) smooths with the same kernel and used to launch it with 64-frame tiles
    // whatever the filter: from n_grad_time = 82 on (n_fft = 1024) the tile exceeds the LDS and the call failed.  The same
    // search, from the 64 frames it always ran with; a filter no tile fits keeps the float smoothing kernels.
    if (p->variant == SG_VARIANT_T && p->stationary && p->smooth_mask && p->n_grad_freq <= 30 && h->ktot <= 65535 &&
        p->n_grad_time <= 96)
      h->t_sm2_ok = fit_sm2_tile(SM2_TT) <= 150 * 1024;
  }
  // window embedded in an n_fft frame: scipy zero-pads the windowed frame at the END
  // (scipy/_spectral_py.py:2202) and extends the signal by W//2; torch centres the window
  // inside n_fft and pads the signal by n_fft//2.
  std::vector<double> wfull(n, 0.0);
  int left = (p->variant == SG_VARIANT_S) ? 0 : (n - W) / 2;
  for (int k = 0; k < W; ++k) wfull[left + k] = w[k];
  h->padL = (p->variant == SG_VARIANT_S) ? W / 2 : n / 2;
  h->mag_scale = (p->variant == SG_VARIANT_S) ? 1.0 / h->sum_w : 1.0;

  std::vector<cx<double>> tw64(h->N);
  std::vector<cx<float>> tw32(h->N);
  for (int k = 0; k < h->N; ++k) {
    long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
    tw64[k] = {(double)cosl(a), (double)sinl(a)};
    tw32[k] = {(float)cosl(a), (float)sinl(a)};
  }
  std::vector<float> wa32(n), ws32(n), wsq32(n);
  for (int k = 0; k < n; ++k) {
    wa32[k] = (float)wfull[k];
    // synthesis window incl. the inverse-transform normalisation: the half-size complex core leaves
    // a factor n/2, the chirp-z inverse a factor n
    ws32[k] = (float)(wfull[k] / ((pow2 || h->mr_ok) ? (double)h->N : (double)n));
    wsq32[k] = (float)(wfull[k] * wfull[k]);
  }
  int rc = SG_OK;
  if (!rc) rc = upload(h, h->tw64, tw64.data(), tw64.size() * sizeof(cx<double>));
  if (!rc && h->mr_ok) {
    std::vector<double> pt((size_t)std::max(1, h->mr.ptotal) * 2, 0.0);
    mr_pass_tables(h->mr, pt.data());
    std::vector<float> pt32(pt.begin(), pt.end());
    rc = upload(h, h->mr_pt64, pt.data(), pt.size() * sizeof(double));
    if (!rc) rc = upload(h, h->mr_pt32, pt32.data(), pt32.size() * sizeof(float));
  }
  {
    // db_fast: centre c_i = 1 + (i + 1/2) / 128 of the i-th mantissa slice; the logarithm is that of the ROUNDED
    // reciprocal, so that log2(m) = -log2(t_i) + log2(1 + (m t_i - 1)) holds exactly
    std::vector<double> lt(256);
    for (int i = 0; i < 128; ++i) {
      const double ti = (double)(1.0L / (1.0L + ((long double)i + 0.5L) / 128.0L));
      lt[2 * i] = ti;
      lt[2 * i + 1] = (double)(-log2l((long double)ti));
    }
    if (!rc) rc = upload(h, h->logtab, lt.data(), lt.size() * sizeof(double));
  }
  if (!rc) rc = upload(h, h->tw32, tw32.data(), tw32.size() * sizeof(cx<float>));
  if (!rc) rc = upload(h, h->wfull64, wfull.data(), wfull.size() * sizeof(double));
  if (!rc) rc = upload(h, h->wa32, wa32.data(), wa32.size() * sizeof(float));
  if (!rc) rc = upload(h, h->ws32, ws32.data(), ws32.size() * sizeof(float));
  if (!rc) rc = upload(h, h->wsq32, wsq32.data(), wsq32.size() * sizeof(float));
  if (!rc && bigf) rc = build_big(h, pow2);
  else if (!rc && !pow2) rc = build_czt(h);
  if (!rc && p->smooth_mask) {
    auto vf = triangle(p->n_grad_freq), vt = triangle(p->n_grad_time);
    double sf = 0, stt = 0;
    for (double x : vf) sf += x;
    for (double x : vt) stt += x;
    std::vector<float> kf(vf.size()), kt(vt.size());
    for (size_t i = 0; i < vf.size(); ++i) kf[i] = (float)(vf[i] / sf);
    for (size_t i = 0; i < vt.size(); ++i) kt[i] = (float)(vt[i] / stt);
    if (!rc) rc = upload(h, h->kf, kf.data(), kf.size() * sizeof(float));
    if (!rc) rc = upload(h, h->kt, kt.data(), kt.size() * sizeof(float));
  }
  // 1 / window envelope per hop phase of the geometries with hop = n_fft / 4 (sum over the 4 frames that overlap a hop)
  auto upload_invn = [&](int hop) {
    std::vector<float> invn(hop);
    for (int s2 = 0; s2 < hop; ++s2) {
      double acc = 0.0;
      for (int q = 0; q < 4; ++q) acc += wfull[hop * q + s2] * wfull[hop * q + s2];
      invn[s2] = (float)(acc > 1e-10 ? 1.0 / acc : 1.0);
    }
    return upload(h, h->invn, invn.data(), invn.size() * sizeof(float));
  };
  // w_512^j: the 512-point register transform of n_fft = 1024 / 512 / 256 (fastpath.hpp)
  auto upload_tw512 = [&]() {
    std::vector<cx<float>> t512(512);
    for (int j = 0; j < 512; ++j) {
      long double a = -2.0L * 3.14159265358979323846264338327950288L * (long double)j / 512.0L;
      t512[j] = {(float)cosl(a), (float)sinl(a)};
    }
    return upload(h, h->tw512, t512.data(), t512.size() * sizeof(cx<float>));
  };
  if (!rc && n == 1024 && W == 1024 && h->H == 256) {
    std::vector<double> norm64(256);
    for (int s2 = 0; s2 < 256; ++s2) {
      double acc = 0.0;
      for (int q = 0; q < 4; ++q) acc += wfull[256 * q + s2] * wfull[256 * q + s2];   // frames t-3 .. t in scipy's order
      norm64[s2] = acc;
    }
    rc = upload_tw512();
    if (!rc) rc = upload_invn(256);
    if (!rc) rc = upload(h, h->norm64, norm64.data(), norm64.size() * sizeof(double));
    h->fast_ok = true;
  }
  for (const RegGeom* r : {&REG512, &REG256, &REG2048})
    if (!rc && n == r->n_fft && W == r->n_fft && h->H == r->hop) {
      if (r->tw == &sg_handle::tw512) rc = upload_tw512();   // (2048 reads tw32)
      if (!rc) rc = upload_invn(r->hop);
      h->reg = r;
    }
  if (!rc && p->smooth_mask && 8 + 2 * p->n_grad_freq <= 18) {
    // counts of 8 adjacent bins f..f+7 from the 18-bit window b[f-nf .. f-nf+17]: two 9-bit tables
    const int nf = p->n_grad_freq;
    std::vector<unsigned long long> tab(1024, 0ull);
    for (int half = 0; half < 2; ++half)
      for (int v = 0; v < 512; ++v) {
        unsigned long long packed = 0;
        for (int e = 0; e < 8; ++e) {
          int cnt = 0;
          for (int b = 0; b < 9; ++b)
            if ((v >> b) & 1) {
              int a = (half * 9 + b) - nf - e;  // tap offset of window bit relative to bin f+e
              if (a >= -nf && a <= nf) cnt += nf + 1 - (a < 0 ? -a : a);
            }
          packed |= (unsigned long long)cnt << (8 * e);
        }
        tab[half * 512 + v] = packed;
      }
    rc = upload(h, h->ftab, tab.data(), tab.size() * sizeof(unsigned long long));
  }
  if (!rc && h->fast_ok && p->smooth_mask && p->n_grad_freq <= 8 && p->n_grad_time <= fast::OP_MAX_NT) {
    // per-lane operands of the one-pass kernel's MFMA smoothing (onepass.hpp), v_mfma_i32_16x16x32_i8 layout:
    // lane l = (q = l / 16, j = l % 16) supplies bytes e = 0..7 = k slots 8 q + e of row/column j
    const int nf = p->n_grad_freq, nt = p->n_grad_time;
    std::vector<unsigned long long> mc(192, 0ull), ex(256, 0ull);
    auto wt = [&](int r, int i) {  // time weight of tile row r (frame r - nt) for output frame i
      const int d = r - i - nt, ad = d < 0 ? -d : d;
      return ad <= nt ? nt + 1 - ad : 0;
    };
    auto trow = [&](int m) { return m < nt ? m : 16 + m; };  // neighbour-list index -> tile row
    for (int l = 0; l < 64; ++l) {
      const int q = l / 16, j = l % 16;
      for (int e = 0; e < 8; ++e) {
        const int a = 8 * q + e - 8 - j, aa = a < 0 ? -a : a;
        mc[l] |= (unsigned long long)(aa <= nf ? nf + 1 - aa : 0) << (8 * e);
        int w1;
        if (e < 4) w1 = wt(nt + 4 * q + e, j);
        else { const int m = 4 * q + e - 4; w1 = m < 2 * nt ? wt(trow(m), j) : 0; }
        mc[64 + l] |= (unsigned long long)w1 << (8 * e);
        if (e < 4) { const int m = 16 + 4 * q + e; mc[128 + l] |= (unsigned long long)(m < 2 * nt ? wt(trow(m), j) : 0) << (8 * e); }
      }
    }
    for (int v = 0; v < 256; ++v)
      for (int e = 0; e < 8; ++e) ex[v] |= (unsigned long long)((v >> e) & 1) << (8 * e);
    rc = upload(h, h->ftab3, mc.data(), mc.size() * 8);
    if (!rc) rc = upload(h, h->xexp, ex.data(), ex.size() * 8);
    // the one-pass kernel reads all of its constant tables through ONE base pointer (onepass.hpp: OP_TAB_*)
    if (!rc) rc = ensure(h, h->optab, fast::OP_TAB_BYTES);
    if (!rc) {
      struct { const DevBuf* b; int off; size_t bytes; } parts[] = {
          {&h->wa32, fast::OP_TAB_WIN, 4096}, {&h->wsq32, fast::OP_TAB_WSQ, 4096}, {&h->invn, fast::OP_TAB_INVN, 1024},
          {&h->tw512, fast::OP_TAB_TW512, 4096}, {&h->tw32, fast::OP_TAB_TW1024, 4096}, {&h->wfull64, fast::OP_TAB_WIN64, 8192},
          {&h->tw64, fast::OP_TAB_TW64, 8192}, {&h->ftab3, fast::OP_TAB_MCONST, 1536}, {&h->xexp, fast::OP_TAB_EXP8, 2048}};
      for (const auto& pt : parts) {
        if (!pt.b->p || pt.b->bytes < pt.bytes) { h->err = "one-pass table arena: a source table is missing"; rc = SG_E_STATE; break; }
        if (hipMemcpy((char*)h->optab.p + pt.off, pt.b->p, pt.bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
          h->err = "one-pass table arena: hipMemcpy failed"; rc = SG_E_HIP; break;
        }
      }
    }
  }
  const RegGeom* rg = h->reg;
  if (!rc && rg && p->smooth_mask && p->n_grad_freq <= rg->op.max_nf && p->n_grad_time <= rg->op.max_nt) {
    // operands of the one-pass gate's MFMA smoothing (onepass512.hpp, onepass256.hpp, onepass2048.hpp), v_mfma_i32_16x16x32_i8
    // layout: lane l = (q = l / 16, j = l % 16) supplies bytes e = 0..7 = k slots 8 q + e of row / column j
    const int nf = p->n_grad_freq, nt = p->n_grad_time;
    auto wt = [&](int d) { const int ad = d < 0 ? -d : d; return ad <= nt ? nt + 1 - ad : 0; };
    auto wf = [&](int d) { const int ad = d < 0 ? -d : d; return ad <= nf ? nf + 1 - ad : 0; };
    const bool two = rg == &REG2048;
    const int ex = 64 * (two ? 3 : 1 + rg->tab_kb);   // the byte expansion follows the operands
    std::vector<unsigned long long> tb(ex + 256, 0ull);
    for (int l = 0; l < 64; ++l) {
      const int q = l / 16, j = l % 16;
      for (int e = 0; e < 8; ++e) {
        const int k = 8 * q + e;
        // k slot 8 q + e: row 4 q + e of the first block (e < 4) / 16 + 4 q + (e - 4) of the second; output frame j at row nt + j
        const int r1 = e < 4 ? 4 * q + e : 16 + 4 * q + (e - 4);
        if (two) {
          // 2048: TWO band matrices (bins 16 b - 24 + k and 16 b + 8 + k against output bin 16 b + j), one k-block of time weights
          tb[l] |= (unsigned long long)wf(k - 24 - j) << (8 * e);
          tb[64 + l] |= (unsigned long long)wf(k + 8 - j) << (8 * e);
          tb[128 + l] |= (unsigned long long)wt(r1 - nt - j) << (8 * e);
        } else {
          // 512 / 256: one band matrix, tab_kb k-blocks of time weights
          tb[l] |= (unsigned long long)wf(k - 8 - j) << (8 * e);
          for (int b = 0; b < rg->tab_kb; ++b) tb[64 * (1 + b) + l] |= (unsigned long long)wt(32 * b + r1 - nt - j) << (8 * e);
        }
      }
    }
    for (int v = 0; v < 256; ++v)
      for (int e = 0; e < 8; ++e) tb[ex + v] |= (unsigned long long)((v >> e) & 1) << (8 * e);
    rc = upload(h, h->regtab, tb.data(), tb.size() * 8);
  }
  if (!rc) rc = ensure(h, h->thresh, (size_t)h->FS * sizeof(double));
  if (rc) {
    g_create_error = h->err;
    sg_destroy(h);
    return rc;
  }
  *out = h;
  return SG_OK;
}

extern "C" int sg_destroy(sg_handle* h) {
  if (!h) return SG_OK;
  (void)hipDeviceSynchronize();
  for (auto& r : h->prof_live) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : h->prof_pool) (void)hipEventDestroy(e);
  if (h->err_host) (void)hipHostFree(h->err_host);
  sg::rg_free(h->rg);
  sg::rw_free(h->rw);
  delete h;   // every DevBuf member frees its allocation
  return SG_OK;
}

extern "C" int sg_n_frames(const sg_handle* h, int64_t L, int64_t* n_frames) {
  if (!h || !n_frames) return SG_E_INVALID;
  *n_frames = frames_for(h, L);
  return SG_OK;
}
extern "C" int sg_output_length(const sg_handle* h, int64_t L, int64_t* out_len) {
  if (!h || !out_len) return SG_E_INVALID;
  *out_len = outlen_for(h, L);
  return SG_OK;
}
