// channelizer.hip — the polyphase channelizer (sdrhip_channelizer.h): one antenna row to M uniform channels decimated by D.
// No reference node stands behind it; the header has the definition and the fast form. One kernel form serves every M: a
// workgroup of CH_THREADS lanes takes a tile of T consecutive output times,
//   1  all lanes: element (tt, r) of the tile, r fastest — the branch sum u[r] = sum_p h[p M + r] x[t - p M - r] as a float fma
//      chain over global reads (taps and input are contiguous in r; the row is re-read P times per output time, from L1 / L2) —
//      written into image tt at the digit-reversed position of (r - t) mod M: the circular shift by the absolute time costs
//      an index, and inverse_dit's input order another;
//   2  all lanes: the backward decimation-in-time passes of fftgen.hpp over the T images at once — its butterflies (dft_small,
//      gmulc) and its plan's roots, a pass's lane loop running over (image, butterfly) so that a workgroup is busy on an 8-point
//      transform as well;
//   3  all lanes: the spectra transposed — row i gets the tile's T values of channel sel[i], contiguous; the images are one
//      element apart from a multiple of M in LDS so that the lanes of a row do not meet on a bank.
// Every block also rolls its share of the tail (the last n_taps - 1 samples, as complex float) into the handle's other tail
// buffer: the blocks of a launch read the old one. The input is read at [0, n) and the tail at [0, n_taps - 1) only: the first
// output time of a call is not before its first sample, the last not behind its last, and terms at l >= n_taps are skipped.
#include "sdrhip_internal.hpp"
#include "sdrhip_channelizer.h"
#include "entry.hpp"
#include "fftgen.hpp"

#include <algorithm>
#include <cmath>

using namespace sdrhip;

namespace {

constexpr int CH_THREADS = fftgen::GT, CH_TMAX = 256;
constexpr int CH_M_MIN = 2, CH_M_MAX = 4096, CH_BRANCH_MAX = 64;
constexpr int CH_ELEMS_SMALL = 4096, CH_ELEMS_LARGE = 8192, CH_M_SMALL = 512;   // complex elements of LDS a workgroup's images take
static_assert(CH_TMAX <= CH_THREADS, "the first T lanes make the tile's time table");

struct ChArgs {
  fftgen::GenDev<float2> fft;
  const void *in;          // [n] of the input type
  const float2 *hist;      // [HH] the tail before the call, oldest first
  float2 *hist_new;        // [HH] the tail behind it
  const float *taps;       // [n_taps]
  const int *invperm;      // [M] natural index -> position in inverse_dit's input
  const int *sel;          // [n_sel]
  float2 *out;
  long out_stride;
  int n, HH, M, D, n_taps, T, ld, n_out, n_sel, tiles;
  int lead;                // the call-relative index of the first output's last sample, 0 <= lead < D
  int tmod0;               // that sample's absolute time mod M
};

__device__ __forceinline__ float2 ch_sample(const short2 *p, int i) { const short2 v = p[i]; return make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ float2 ch_sample(const float2 *p, int i) { return p[i]; }

// one backward DIT pass of radix R over nimg images ld apart: pass_dit's arithmetic, the lane loop over (image, butterfly)
template <int R>
__device__ __forceinline__ void ch_pass(float2 *x, const fftgen::GenDev<float2> &p, int s, int nimg, int ld, int tid) {
  const int n = s * R, tw = p.L / n, per = p.L / R, total = nimg * per;
  for (int i = tid; i < total; i += CH_THREADS) {
    const int im = i / per, b = i - im * per;
    const int blk = b / s, j = b - blk * s, base = im * ld + blk * n + j;
    float2 v[R];
    v[0] = x[base];
#pragma unroll
    for (int k = 1; k < R; k++) v[k] = s > 1 ? fftgen::gmulc(x[base + k * s], p.W[j * tw * k]) : x[base + k * s];
    fftgen::dft_small<float2, R, 1>(v, p);
#pragma unroll
    for (int m = 0; m < R; m++) x[base + m * s] = v[m];
  }
}

template <class I>
__device__ __forceinline__ void ch_body(const ChArgs &a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float2 *img = reinterpret_cast<float2 *>(smem_raw);
  __shared__ int tmod_s[CH_TMAX], rel_s[CH_TMAX];
  const int tid = (int)threadIdx.x, tile = (int)blockIdx.x, M = a.M;
  const I *in = static_cast<const I *>(a.in);

  if (tile < a.tiles) {
    const int j0 = tile * a.T, Tc = min(a.T, a.n_out - j0);
    if (tid < Tc) {
      const long long jd = (long long)(j0 + tid) * a.D;   // below n <= 2^30
      tmod_s[tid] = (int)(((long long)a.tmod0 + jd) % M);
      rel_s[tid] = a.lead + (int)jd;
    }
    __syncthreads();
    // phase 1
    for (int e = tid; e < Tc * M; e += CH_THREADS) {
      const int tt = e / M, r = e - tt * M;
      int rel = rel_s[tt] - r;
      float re = 0.f, im = 0.f;
#pragma unroll 4
      for (int l = r; l < a.n_taps; l += M, rel -= M) {
        // (the clamps never bind — see the head of the file; they keep a wrong count from becoming a wild read)
        const float2 v = rel >= 0 ? ch_sample(in, min(rel, a.n - 1)) : a.hist[max(a.HH + rel, 0)];
        const float hv = a.taps[l];
        re = __builtin_fmaf(hv, v.x, re);
        im = __builtin_fmaf(hv, v.y, im);
      }
      int jw = r - tmod_s[tt];
      jw += jw < 0 ? M : 0;
      img[tt * a.ld + a.invperm[jw]] = make_float2(re, im);
    }
    __syncthreads();
    // phase 2
    int s = 1;
    for (int pass = a.fft.npass - 1; pass >= 0; pass--) {
      const int r = a.fft.radix[pass];
#define SDRHIP_CH_CALL(R_) ch_pass<R_>(img, a.fft, s, Tc, a.ld, tid)
      SDRHIP_GEN_RADIX_SWITCH(r, SDRHIP_CH_CALL)
#undef SDRHIP_CH_CALL
      __syncthreads();
      s *= r;
    }
    // phase 3
    for (int e = tid; e < a.n_sel * Tc; e += CH_THREADS) {
      const int i = e / Tc, tt = e - i * Tc;
      a.out[(long)i * a.out_stride + j0 + tt] = img[tt * a.ld + a.sel[i]];
    }
  }
  // the tail behind the call: the last HH samples of (tail, in[0 ... n))
  for (int k = (int)blockIdx.x * CH_THREADS + tid; k < a.HH; k += (int)gridDim.x * CH_THREADS) {
    const int q = a.n + k;   // n < 2^30, HH < 2^18
    a.hist_new[k] = q < a.HH ? a.hist[q] : ch_sample(in, q - a.HH);
  }
}

__global__ __launch_bounds__(CH_THREADS) void channelizer_cs16_kernel(const ChArgs a) { ch_body<short2>(a); }
__global__ __launch_bounds__(CH_THREADS) void channelizer_cf32_kernel(const ChArgs a) { ch_body<float2>(a); }

bool dtype_ok(int d) { return d == SDRHIP_CHAN_CS16 || d == SDRHIP_CHAN_CF32; }

// taps rounded once to float32; false where one is not finite as a float
bool round_taps(const double *taps, int n, std::vector<float> &out, int *bad) {
  out.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    out[i] = (float)taps[i];
    if (!std::isfinite(out[i])) { *bad = i; return false; }
  }
  return true;
}

}  // namespace

struct sdrhip_channelizer {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_CHAN_CS16, M = 2, D = 1, n_taps = 1, T = 1, ld = 3, n_sel = 2;
  size_t max_in = 0;
  uint64_t consumed = 0;
  int cur = 0;                     // which tail buffer holds the state
  fftgen::GenPlan<float2> plan;
  DevBuf<float> taps;
  DevBuf<int> invperm, sel;
  DevBuf<float2> hist[2];          // [n_taps - 1] each (at least one element)
  Staging stage;
  size_t in_elem() const { return dtype == SDRHIP_CHAN_CS16 ? 4 : 8; }
  int HH() const { return n_taps - 1; }
  size_t lds_bytes() const { return (size_t)T * (size_t)ld * sizeof(float2); }
  size_t out_count(size_t n) const { return (size_t)((consumed + n) / (uint64_t)D - consumed / (uint64_t)D); }
  size_t out_count_max(size_t n) const { return ceil_div(n, (size_t)D); }   // whatever N is

  void select_all() {
    std::vector<int> s((size_t)M);
    for (int k = 0; k < M; k++) s[k] = k;
    put_sync(ctx, sel.p, s.data(), s.size() * sizeof(int));
    n_sel = M;
  }
  void fresh_state() {
    SDRHIP_CHECK_HIP(hipMemsetAsync(hist[0].p, 0, hist[0].n * sizeof(float2), ctx->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    cur = 0; consumed = 0;
  }
  // n >= 1; the state moves on only behind a launch that was accepted
  void launch(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) {
    ctx->use();
    ChArgs a;
    a.fft = plan.dev;
    a.in = in_dev; a.hist = hist[cur].p; a.hist_new = hist[cur ^ 1].p;
    a.taps = taps.p; a.invperm = invperm.p; a.sel = sel.p;
    a.out = static_cast<float2 *>(out_dev); a.out_stride = (long)out_stride;
    a.n = (int)n; a.HH = HH(); a.M = M; a.D = D; a.n_taps = n_taps; a.T = T; a.ld = ld; a.n_out = (int)n_out; a.n_sel = n_sel;
    a.tiles = (int)ceil_div(n_out, (size_t)T);
    a.lead = (int)((uint64_t)D - 1 - consumed % (uint64_t)D);
    a.tmod0 = (int)((consumed + (uint64_t)a.lead) % (uint64_t)M);
    const dim3 grid((unsigned)std::max(a.tiles, 1)), block(CH_THREADS);
    const size_t lds = lds_bytes();
    (void)hipGetLastError();
    if (dtype == SDRHIP_CHAN_CS16) hipLaunchKernelGGL(channelizer_cs16_kernel, grid, block, lds, ctx->stream, a);
    else hipLaunchKernelGGL(channelizer_cf32_kernel, grid, block, lds, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
    consumed += n;
    cur ^= 1;
  }
};

extern "C" {

int sdrhip_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                              sdrhip_channelizer **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(dtype_ok(dtype), SDRHIP_E_INVALID, "bad dtype %d", dtype);
    SDRHIP_REQUIRE(M >= CH_M_MIN && M <= CH_M_MAX, SDRHIP_E_SIZE, "M %d outside [%d,%d] (one transform lives in one workgroup's LDS)", M,
                   CH_M_MIN, CH_M_MAX);
    std::vector<int> radix;
    int bad = 1;
    SDRHIP_REQUIRE(fftgen::GenPlan<float2>::factor(M, radix, &bad), SDRHIP_E_INVALID,
                   "M %d has the prime factor %d: the device transforms sizes made of 2, 3, 5, 7, 11 and 13", M, bad);
    SDRHIP_REQUIRE(D >= 1 && D <= M, SDRHIP_E_INVALID, "D %d outside [1,M = %d]", D, M);
    SDRHIP_REQUIRE(n_taps >= 1 && n_taps <= CH_BRANCH_MAX * M, SDRHIP_E_SIZE, "n_taps %d outside [1,%d M = %d]", n_taps, CH_BRANCH_MAX,
                   CH_BRANCH_MAX * M);
    require_max_in(max_in);
    std::vector<float> h32;
    SDRHIP_REQUIRE(round_taps(taps, n_taps, h32, &bad), SDRHIP_E_INVALID, "tap %d is not finite as a float", bad);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_channelizer *h) {
      h->dtype = dtype; h->M = M; h->D = D; h->n_taps = n_taps; h->max_in = max_in;
      h->T = std::min(CH_TMAX, (M <= CH_M_SMALL ? CH_ELEMS_SMALL : CH_ELEMS_LARGE) / M);
      h->ld = M + 1;
      h->plan.build(ctx, M, CH_M_MAX);
      std::vector<int> inv((size_t)M);
      for (int pos = 0; pos < M; pos++) inv[(size_t)h->plan.perm[pos]] = pos;
      h->invperm.alloc((size_t)M);
      h->invperm.upload(inv.data(), inv.size(), ctx->stream);
      h->taps.alloc((size_t)n_taps);
      h->taps.upload(h32.data(), h32.size(), ctx->stream);
      h->sel.alloc((size_t)M);
      h->select_all();
      for (auto &b : h->hist) { b.alloc((size_t)std::max(h->HH(), 1)); b.zero(ctx->stream); }
      allow_lds_max(dtype == SDRHIP_CHAN_CS16 ? channelizer_cs16_kernel : channelizer_cf32_kernel, h->lds_bytes());
      h->fresh_state();
    });
  });
}

int sdrhip_channelizer_out_count(sdrhip_channelizer *h, size_t n, size_t *n_out) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && n_out, SDRHIP_E_INVALID, "NULL argument");
    *n_out = h->out_count(n);
  });
}

int sdrhip_channelizer_process_dev(sdrhip_channelizer *h, const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_channelizer_process_dev");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    const size_t no = h->out_count(n);
    const Strides s = call_strides("n", n, 0, no, out_stride, STRIDE_OUT);
    require_disjoint(in_dev, n, n, h->in_elem(), out_dev, s.out, no, sizeof(float2), 1, (size_t)h->n_sel);
    h->launch(in_dev, n, out_dev, s.out, no);
    if (n_out) *n_out = no;
  });
}

int sdrhip_channelizer_process(sdrhip_channelizer *h, const void *in_host, size_t n, void *out_host, size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_channelizer_process");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_host, out_host)) return;
    const size_t no = h->out_count(n), rows = (size_t)h->n_sel, eb = h->in_elem(), ob = sizeof(float2);
    const Strides s = call_strides("n", n, 0, no, out_stride, STRIDE_OUT);
    // (the staged rows follow the selection: a set_channels can raise them)
    const size_t out_cap_b = rows * h->out_count_max(h->max_in) * ob;
    if (h->stage.out.p && h->stage.out.n < out_cap_b) h->stage.out.alloc(out_cap_b);
    run_staged(h->ctx, h->stage, h->max_in * eb, out_cap_b, {in_host, n * eb, n * eb, 1}, {out_host, s.out * ob, no * ob, rows},
               [&](void *in, void *out) {
                 h->launch(in, n, out, no, no);
                 return no * ob;
               });
    if (n_out) *n_out = no;
  });
}

int sdrhip_channelizer_set_channels(sdrhip_channelizer *h, const int *idx, int n_sel) {
  return guarded([&] {
    use_handle(h);
    if (!idx) { h->select_all(); return; }
    SDRHIP_REQUIRE(n_sel >= 1 && n_sel <= h->M, SDRHIP_E_INVALID, "n_sel %d outside [1,M = %d]", n_sel, h->M);
    std::vector<char> seen((size_t)h->M, 0);
    for (int i = 0; i < n_sel; i++) {
      SDRHIP_REQUIRE(idx[i] >= 0 && idx[i] < h->M, SDRHIP_E_INVALID, "channel %d (row %d) outside [0,%d)", idx[i], i, h->M);
      SDRHIP_REQUIRE(!seen[(size_t)idx[i]], SDRHIP_E_INVALID, "channel %d is selected twice (row %d)", idx[i], i);
      seen[(size_t)idx[i]] = 1;
    }
    put_sync(h->ctx, h->sel.p, idx, (size_t)n_sel * sizeof(int));
    h->n_sel = n_sel;
  });
}

int sdrhip_channelizer_set_taps(sdrhip_channelizer *h, const double *taps) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && taps, SDRHIP_E_INVALID, "NULL argument");
    h->ctx->use();
    std::vector<float> h32;
    int bad = 0;
    SDRHIP_REQUIRE(round_taps(taps, h->n_taps, h32, &bad), SDRHIP_E_INVALID, "tap %d is not finite as a float", bad);
    put_sync(h->ctx, h->taps.p, h32.data(), h32.size() * sizeof(float));
  });
}

int sdrhip_channelizer_reset(sdrhip_channelizer *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}

int sdrhip_channelizer_get_state(sdrhip_channelizer *h, uint64_t *consumed, float *tail, size_t tail_len) {
  return guarded([&] {
    use_handle(h);
    SDRHIP_REQUIRE(!tail || tail_len >= (size_t)h->HH(), SDRHIP_E_SIZE, "tail_len %zu < n_taps - 1 = %d", tail_len, h->HH());
    if (tail && h->HH() > 0) get_sync(h->ctx, tail, h->hist[h->cur].p, (size_t)h->HH() * sizeof(float2));
    if (consumed) *consumed = h->consumed;
  });
}

int sdrhip_channelizer_plan_info(sdrhip_channelizer *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    if (tile_times) *tile_times = h->T;
    if (branch_taps) *branch_taps = (int)ceil_div((size_t)h->n_taps, (size_t)h->M);
    if (lds_bytes) *lds_bytes = (int)h->lds_bytes();
    if (rows) *rows = h->n_sel;
  });
}

int sdrhip_channelizer_kernel_names(sdrhip_channelizer *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->dtype == SDRHIP_CHAN_CS16 ? "channelizer_cs16_kernel" : "channelizer_cf32_kernel"; });
  });
}

int sdrhip_channelizer_destroy(sdrhip_channelizer *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
