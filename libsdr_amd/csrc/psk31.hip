// psk31.hip — the BPSK31 bank (sdrhip_psk31.h): `channels` reference BPSK31<int16_t> / BPSK31<float> demodulators
// (src/psk31.hh:16-291), one launch per call. The node is sequential per row from its first operation to its last: the carrier
// phase that rotates a sample comes from the loop filter the last sub-sample fed, and whether a trip consumes a sample or takes
// a sub-sample depends on mu. So one lane runs a row's whole recursion, state in registers, and the rows are spread as widely
// as they go: a workgroup of PSK_THREADS lanes takes PSK_G rows, ONE WAVE PER ROW, so no two rows share a wave and the two
// paths of the loop never serialise against each other; a 1024-row bank is 256 groups. PSK_T samples at a time:
//   1  all lanes: load the rows' samples (coalesced along the rows) into the LDS tile;
//   2  lane 0 of wave k walks row k's samples: every trip consumes a sample (fill) or emits a sub-sample.
// In LDS besides the tile: the interpolation table (an argument of create), each row's history of 64 phases and its line of 8
// rotated samples, kept as the reference keeps it (a ring written twice, so the 8 taps read 8 consecutive entries).
//
// Numerics (the contract in sdrhip_psk31.h): every float product is rounded on its own — psk_mul passes it through an empty asm
// statement, so no multiply-add can be formed from it whatever the build's contraction mode (agc.hip); psk_dmul does the same
// for the doubles of psk_sincos. Division: hipcc's default, correctly rounded. Denormals are kept (no flush flag).
// What bounds the kernel is the single lane's instruction stream: a double-precision sincos (about 45 dependent operations) per
// input sample, and 16 products and two loop filters per sub-sample; nothing else in the wave hides it.
#include "sdrhip_internal.hpp"
#include "sdrhip_psk31.h"
#include "entry.hpp"

#include <cmath>
#include <cstring>

using namespace sdrhip;

namespace {

constexpr int PSK_G = 4, PSK_T = 256, PSK_WAVE = 64, PSK_THREADS = PSK_G * PSK_WAVE;
constexpr int PSK_CHANNELS_MAX = 65535, PSK_ROWS = 129, PSK_TAPS = 8, PSK_TABLE = PSK_ROWS * PSK_TAPS;
// a row's state in device memory, in floats: P F mu omega | hist_idx last (int bits) | c0 c1 c2 - | p0 p1 p2 | line[8] | hist[64]
constexpr int ST_P = 0, ST_F = 1, ST_MU = 2, ST_OMEGA = 3, ST_HIDX = 4, ST_LAST = 5, ST_C = 6, ST_PP = 10, ST_LINE = 16, ST_HIST = 32, PSK_STATE = 96;
static_assert(PSK_T == PSK_THREADS, "phase 1: lane t takes sample t of every row of the tile");

constexpr double PSK_TWO_PI = 2.0 * M_PI, PSK_TWO_OVER_PI = 2.0 / M_PI, PSK_PIO2 = M_PI / 2.0;

struct PskArgs {
  const void *in; uint8_t *out; uint32_t *counts;
  long in_stride, out_stride;
  int N, C;
  unsigned cap;        // the bits a row may write
  int budget;          // the sub-samples a call can take (the bound behind the capacity): the walk ends there whatever the state
  const float *table;  // [129][8]
  const float2 *par;   // Fmin, Fmax
  float *st;           // [C][PSK_STATE]
  float alpha, beta, min_omega, max_omega;
};

// (the empty asm makes the product a value of its own: it costs no instruction and keeps it out of any fused multiply-add)
__device__ __forceinline__ float psk_mul(float a, float b) { float p = a * b; asm("" : "+v"(p)); return p; }
__device__ __forceinline__ double psk_dmul(double a, double b) { double p = a * b; asm("" : "+v"(p)); return p; }

__device__ __forceinline__ float psk_wrap(float P) {
#pragma unroll
  for (int j = 0; j < 2; j++) { const double d = (double)P; if (d > PSK_TWO_PI) P = (float)(d - PSK_TWO_PI); }
#pragma unroll
  for (int j = 0; j < 2; j++) { const double d = (double)P; if (d < -PSK_TWO_PI) P = (float)(d + PSK_TWO_PI); }
  return P;
}

// the defined sincos of the header (deviation 1)
__device__ __forceinline__ void psk_sincos(float P, float &s, float &c) {
  const double x = (double)P;
  const double k = rint(psk_dmul(x, PSK_TWO_OVER_PI));
  const double r = x - psk_dmul(k, PSK_PIO2);
  const double z = psk_dmul(r, r);
  double ps = 1.0 / 6227020800.0;
  ps = psk_dmul(ps, z) + -1.0 / 39916800.0;
  ps = psk_dmul(ps, z) + 1.0 / 362880.0;
  ps = psk_dmul(ps, z) + -1.0 / 5040.0;
  ps = psk_dmul(ps, z) + 1.0 / 120.0;
  ps = psk_dmul(ps, z) + -1.0 / 6.0;
  const double sr = r + psk_dmul(psk_dmul(r, z), ps);
  double pc = -1.0 / 87178291200.0;
  pc = psk_dmul(pc, z) + 1.0 / 479001600.0;
  pc = psk_dmul(pc, z) + -1.0 / 3628800.0;
  pc = psk_dmul(pc, z) + 1.0 / 40320.0;
  pc = psk_dmul(pc, z) + -1.0 / 720.0;
  pc = psk_dmul(pc, z) + 1.0 / 24.0;
  pc = psk_dmul(pc, z) + -1.0 / 2.0;
  const double cr = 1.0 + psk_dmul(z, pc);
  const int q = (k == k) ? ((int)k & 3) : 0;
  const double sv = (q & 1) ? cr : sr, cv = (q & 1) ? sr : cr;
  s = (float)((q & 2) ? -sv : sv);
  c = (float)(((q + 1) & 2) ? -cv : cv);
}

__device__ __forceinline__ float2 psk_sample(short2 v) { return make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ float2 psk_sample(float2 v) { return v; }

template <class S2>
__device__ __forceinline__ void psk_body(const PskArgs &a) {
  __shared__ S2 tile[PSK_G * PSK_T];
  __shared__ float tab[PSK_TABLE];
  __shared__ float hist_s[PSK_G * 64];
  __shared__ float2 dl_s[PSK_G * 16];
  __shared__ int idx_s[PSK_G];
  const int t = (int)threadIdx.x, c0 = (int)blockIdx.x * PSK_G;
  const int nch = min(PSK_G, a.C - c0);
  const int wave = t / PSK_WAVE, lane = t % PSK_WAVE;
  const bool active = wave < nch;
  const bool walk = active && lane == 0;
  float *st = a.st + (long)(c0 + (active ? wave : 0)) * PSK_STATE;
  float *hist = hist_s + wave * 64;
  float2 *dl = dl_s + wave * 16;

  for (int i = t; i < PSK_TABLE; i += PSK_THREADS) tab[i] = a.table[i];
  if (active) {
    hist[lane] = st[ST_HIST + lane];
    if (lane < 8) {
      const float2 v = make_float2(st[ST_LINE + 2 * lane], st[ST_LINE + 2 * lane + 1]);
      dl[lane] = v;
      dl[lane + 8] = v;
    }
  }
  float P = 0.f, F = 0.f, mu = 0.f, omega = 0.f, Fmin = 0.f, Fmax = 0.f;
  float c0T = 0.f, c1T = 0.f, c2T = 0.f, p0r = 0.f, p1r = 0.f, p2r = 0.f, p0i = 0.f, p1i = 0.f, p2i = 0.f;
  int hidx = 0, last = 1, dlx = 0, budget = a.budget;
  unsigned o = 0;
  if (walk) {
    P = st[ST_P]; F = st[ST_F]; mu = st[ST_MU]; omega = st[ST_OMEGA];
    hidx = __float_as_int(st[ST_HIDX]) & 63; last = __float_as_int(st[ST_LAST]);
    c0T = st[ST_C]; c1T = st[ST_C + 1]; c2T = st[ST_C + 2];
    p0r = st[ST_PP]; p0i = st[ST_PP + 1]; p1r = st[ST_PP + 2]; p1i = st[ST_PP + 3]; p2r = st[ST_PP + 4]; p2i = st[ST_PP + 5];
    const float2 f = a.par[c0 + wave];
    Fmin = f.x; Fmax = f.y;
  }
  const S2 *in = static_cast<const S2 *>(a.in);
  uint8_t *out = a.out + (long)(c0 + (active ? wave : 0)) * a.out_stride;
  __syncthreads();

  for (int n0 = 0; n0 < a.N; n0 += PSK_T) {
    const int cnt = min(PSK_T, a.N - n0);
    // phase 1
#pragma unroll
    for (int k = 0; k < PSK_G; k++)
      if (k < nch && t < cnt) tile[k * PSK_T + t] = in[(long)(c0 + k) * a.in_stride + n0 + t];
    __syncthreads();
    // phase 2
    if (walk) {
      const S2 *row = tile + wave * PSK_T;
      int i = 0;
      while (i < cnt) {
        if (!(mu <= 1.0f)) {   // fill (a NaN mu comes here too and consumes the call)
          mu = mu - 1.0f;
          P = psk_wrap(P + F);
          float s, c;
          psk_sincos(P, s, c);
          const float2 x = psk_sample(row[i]);
          const float2 v = make_float2(psk_mul(c, x.x) - psk_mul(s, x.y), psk_mul(c, x.y) + psk_mul(s, x.x));
          dl[dlx] = v;
          dl[dlx + 8] = v;
          dlx = (dlx + 1) & 7;
          i++;
        } else {               // sub-sample
          if (--budget < 0) break;
          int r = (int)roundf(mu * 128.0f);
          r = min(max(r, 0), PSK_ROWS - 1);
          const float *h = tab + r * PSK_TAPS;
          float re = 0.f, im = 0.f;
#pragma unroll
          for (int k = 0; k < PSK_TAPS; k++) {
            const float2 v = dl[dlx + k];
            re = re + psk_mul(v.x, h[k]);
            im = im + psk_mul(v.y, h[k]);
          }
          // timing loop
          p2r = p1r; p2i = p1i; p1r = p0r; p1i = p0i; p0r = re; p0i = im;
          c2T = c1T; c1T = c0T; c0T = re > 0.f ? -1.0f : 1.0f;
          float err = psk_mul(p0r - p2r, c1T) - psk_mul(c0T - c2T, p1r);
          if (err > 1.0f) err = 1.0f;
          if (err < -1.0f) err = -1.0f;
          omega = omega + psk_mul(0.001f, err);
          omega = omega < a.max_omega ? omega : a.max_omega;   // std::min(max_omega, omega)
          omega = a.min_omega < omega ? omega : a.min_omega;   // std::max(min_omega, .)
          mu = mu + (omega + psk_mul(0.01f, err));
          // carrier loop
          const float nrm2 = psk_mul(re, re) + psk_mul(im, im);
          const float phi = nrm2 == 0.f ? 0.f : psk_mul(-re, im) / nrm2;
          F = F + psk_mul(a.beta, phi);
          P = psk_wrap(P + (F + psk_mul(a.alpha, phi)));
          F = Fmin < F ? F : Fmin;   // std::max(Fmin, F)
          F = F < Fmax ? F : Fmax;   // std::min(Fmax, .)
          // symbol logic
          hist[hidx] = re;
          bool emit = false;
          if (hidx > 1) {
            const float prev = hist[hidx - 1];
            if ((prev >= 0.f && re <= 0.f) || (prev <= 0.f && re >= 0.f)) {
              emit = hidx >= 32;
              if (!emit) hidx = 0;
            } else if (hidx == 63) emit = true;
            else hidx++;
          } else hidx++;
          if (emit) {
            float sum = 0.f;
            for (int k = 0; k <= hidx; k++) sum = sum + hist[k];
            const int cc = sum > 0.f ? 1 : -1;
            if (o < a.cap) out[o] = (uint8_t)(last == cc);
            o++;
            last = cc;
            hidx = 0;
          }
        }
      }
    }
    __syncthreads();   // the next tile's phase 1 writes where this phase read
  }
  if (walk) {
    if (a.N > 0) {
      st[ST_P] = P; st[ST_F] = F; st[ST_MU] = mu; st[ST_OMEGA] = omega;
      st[ST_HIDX] = __int_as_float(hidx); st[ST_LAST] = __int_as_float(last);
      st[ST_C] = c0T; st[ST_C + 1] = c1T; st[ST_C + 2] = c2T;
      st[ST_PP] = p0r; st[ST_PP + 1] = p0i; st[ST_PP + 2] = p1r; st[ST_PP + 3] = p1i; st[ST_PP + 4] = p2r; st[ST_PP + 5] = p2i;
    }
    a.counts[c0 + wave] = min(o, a.cap);
    idx_s[wave] = dlx;
  }
  __syncthreads();
  if (active && a.N > 0) {
    st[ST_HIST + lane] = hist[lane];
    if (lane < 8) {
      const float2 v = dl[idx_s[wave] + lane];   // oldest first
      st[ST_LINE + 2 * lane] = v.x;
      st[ST_LINE + 2 * lane + 1] = v.y;
    }
  }
}

__global__ __launch_bounds__(PSK_THREADS) void psk31_cs16_kernel(const PskArgs a) { psk_body<short2>(a); }
__global__ __launch_bounds__(PSK_THREADS) void psk31_cf32_kernel(const PskArgs a) { psk_body<float2>(a); }

bool df_ok(double dF) { return dF > 0.0 && dF <= M_PI; }

}  // namespace

struct sdrhip_psk31 {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_PSK31_CS16, C = 1;
  size_t max_in = 0;
  float alpha = 0.f, beta = 0.f, omega0 = 1.f, min_omega = 1.f, max_omega = 1.f;
  std::vector<float2> par;   // the host's copy of the rows' Fmin, Fmax
  DevBuf<float2> par_dev;
  DevBuf<float> table, st;
  DevBuf<uint32_t> counts;   // of the host-pointer calls
  Staging stage;
  size_t elem() const { return dtype == SDRHIP_PSK31_CS16 ? 4 : 8; }

  // the sub-samples a call of n samples can take, and the bits (the header's bound)
  size_t sub_samples(size_t n) const {
    const double d = (double)min_omega - 0.0100001;
    return (size_t)std::floor(((double)n + 3.0 + (double)max_omega) / d) + 1;
  }
  size_t capacity(size_t n) const { return n ? 1 + sub_samples(n) / 33 : 0; }

  void fresh_row(float *s) const {
    memset(s, 0, PSK_STATE * sizeof(float));
    s[ST_MU] = 0.25f; s[ST_OMEGA] = omega0;
    const int one = 1;
    memcpy(&s[ST_LAST], &one, sizeof one);
  }
  void fresh_state() {
    std::vector<float> s((size_t)C * PSK_STATE);
    for (int c = 0; c < C; c++) fresh_row(&s[(size_t)c * PSK_STATE]);
    put_sync(ctx, st.p, s.data(), s.size() * sizeof(float));
  }
  void launch(const void *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride, uint32_t *counts_dev) {
    ctx->use();
    if (N == 0) return;
    PskArgs a;
    a.in = in_dev; a.out = out_dev; a.counts = counts_dev; a.in_stride = (long)in_stride; a.out_stride = (long)out_stride;
    a.N = (int)N; a.C = C; a.cap = (unsigned)std::min(capacity(N), out_stride); a.budget = (int)std::min(sub_samples(N), (size_t)0x7fffffff);
    a.table = table.p; a.par = par_dev.p; a.st = st.p;
    a.alpha = alpha; a.beta = beta; a.min_omega = min_omega; a.max_omega = max_omega;
    const dim3 grid((unsigned)ceil_div((size_t)C, (size_t)PSK_G));
    (void)hipGetLastError();
    if (dtype == SDRHIP_PSK31_CS16) hipLaunchKernelGGL(psk31_cs16_kernel, grid, dim3(PSK_THREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL(psk31_cf32_kernel, grid, dim3(PSK_THREADS), 0, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

static void require_df(double dF, int c) { SDRHIP_REQUIRE(df_ok(dF), SDRHIP_E_INVALID, "dF %g of channel %d outside (0,pi]", dF, c); }

// dF: `channels` floats, or (one) one double for all rows
static void psk_create(sdrhip_ctx *ctx, int dtype, double Fs, const float *dF, const double *dF_one, const float *table, int channels,
                       size_t max_in, sdrhip_psk31 **out) {
  if (out) *out = nullptr;
  SDRHIP_REQUIRE(out && table && (dF || dF_one), SDRHIP_E_INVALID, "NULL argument");
  SDRHIP_REQUIRE(dtype == SDRHIP_PSK31_CS16 || dtype == SDRHIP_PSK31_CF32, SDRHIP_E_INVALID, "bad dtype %d", dtype);
  require_channels(channels, PSK_CHANNELS_MAX);
  require_max_in(max_in);
  SDRHIP_REQUIRE(std::isfinite(Fs) && Fs >= 2000.0, SDRHIP_E_INVALID, "sample_rate %g is not a finite number of at least 2000", Fs);
  if (dF_one) require_df(*dF_one, 0);
  else for (int c = 0; c < channels; c++) require_df((double)dF[c], c);
  for (int i = 0; i < PSK_TABLE; i++) SDRHIP_REQUIRE(std::isfinite(table[i]), SDRHIP_E_INVALID, "table entry %d is not finite", i);
  require_device_for_null_ctx(ctx);
  make_handle(ctx, out, true, [&](sdrhip_psk31 *h) {
    h->dtype = dtype; h->C = channels; h->max_in = max_in;
    const double damping = std::sqrt(2.0) / 2, bw = M_PI / 100;
    const double tmp = 1. + 2 * damping * bw + bw * bw;
    h->alpha = (float)(4 * damping * bw / tmp);
    h->beta = (float)(4 * bw * bw / tmp);
    h->omega0 = (float)(Fs / 2000.0);
    h->min_omega = (float)((double)h->omega0 * (1.0 - (double)0.001f));
    h->max_omega = (float)((double)h->omega0 * (1.0 + (double)0.001f));
    h->par.resize((size_t)channels);
    for (int c = 0; c < channels; c++)
      h->par[c] = dF_one ? make_float2((float)(-*dF_one), (float)*dF_one) : make_float2(-dF[c], dF[c]);
    h->par_dev.alloc((size_t)channels);
    h->par_dev.upload(h->par.data(), h->par.size(), ctx->stream);
    h->table.alloc(PSK_TABLE);
    h->table.upload(table, PSK_TABLE, ctx->stream);
    h->st.alloc((size_t)channels * PSK_STATE);
    h->counts.alloc((size_t)channels);
    h->fresh_state();
  });
}

// A x = b for n = 8 in double, Gaussian elimination with partial pivoting
static void solve8(double A[8][8], double b[8], double x[8]) {
  for (int c = 0; c < 8; c++) {
    int p = c;
    for (int r = c + 1; r < 8; r++) if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
    if (p != c) { for (int k = 0; k < 8; k++) std::swap(A[p][k], A[c][k]); std::swap(b[p], b[c]); }
    for (int r = c + 1; r < 8; r++) {
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 8; k++) A[r][k] -= f * A[c][k];
      b[r] -= f * b[c];
    }
  }
  for (int r = 7; r >= 0; r--) {
    double s = b[r];
    for (int k = r + 1; k < 8; k++) s -= A[r][k] * x[k];
    x[r] = s / A[r][r];
  }
}
static double band_sinc(double t) { return t == 0.0 ? 0.5 : std::sin(M_PI * t / 2) / (M_PI * t); }

extern "C" {

int sdrhip_design_inpol_taps(float *out) {
  return guarded([&] {
    SDRHIP_REQUIRE(out, SDRHIP_E_INVALID, "NULL argument");
    for (int r = 0; r <= 64; r++) {
      double A[8][8], b[8], h[8];
      const double mu = (double)r / 128.0;
      for (int k = 0; k < 8; k++) {
        for (int l = 0; l < 8; l++) A[k][l] = band_sinc((double)(k - l));
        b[k] = band_sinc((double)(k - 4) + mu);
      }
      solve8(A, b, h);
      if (r == 0) for (int k = 0; k < 8; k++) h[k] = k == 4 ? 1.0 : 0.0;
      if (r == 64) for (int k = 0; k < 4; k++) h[k] = h[7 - k] = 0.5 * (h[k] + h[7 - k]);
      for (int k = 0; k < 8; k++) out[r * 8 + k] = (float)h[k];
    }
    for (int r = 65; r < PSK_ROWS; r++)
      for (int k = 0; k < 8; k++) out[r * 8 + k] = out[(128 - r) * 8 + (7 - k)];
  });
}

int sdrhip_psk31_create(sdrhip_ctx *ctx, int dtype, double sample_rate, double dF, const float *table, int channels, size_t max_in,
                        sdrhip_psk31 **out) {
  return guarded([&] { psk_create(ctx, dtype, sample_rate, nullptr, &dF, table, channels, max_in, out); });
}

int sdrhip_psk31bank_create(sdrhip_ctx *ctx, int dtype, double sample_rate, const float *dF, const float *table, int channels,
                            size_t max_in, sdrhip_psk31 **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(dF, SDRHIP_E_INVALID, "NULL argument");
    psk_create(ctx, dtype, sample_rate, dF, nullptr, table, channels, max_in, out);
  });
}

int sdrhip_psk31_out_capacity(sdrhip_psk31 *h, size_t n, size_t *bits) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && bits, SDRHIP_E_INVALID, "NULL argument");
    *bits = h->capacity(n);
  });
}

int sdrhip_psk31_process_dev(sdrhip_psk31 *h, const void *in_dev, size_t n, size_t in_stride, uint8_t *bits_dev, size_t out_stride,
                             uint32_t *counts_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_psk31_process_dev");
    if (!call_begin(h, "n", n, in_dev, bits_dev)) return;
    SDRHIP_REQUIRE(counts_dev, SDRHIP_E_INVALID, "NULL buffer");
    const size_t cap = h->capacity(n);
    const Strides s = call_strides("n", n, in_stride, cap, out_stride, STRIDE_IN | STRIDE_OUT, "capacity");
    require_disjoint(in_dev, s.in, n, h->elem(), bits_dev, s.out, cap, 1, (size_t)h->C);
    h->launch(in_dev, n, s.in, bits_dev, s.out, counts_dev);
  });
}

int sdrhip_psk31_process(sdrhip_psk31 *h, const void *in_host, size_t n, size_t in_stride, uint8_t *bits_host, size_t out_stride,
                         uint32_t *counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_psk31_process");
    process_counted(h, in_host, n, in_stride, h ? h->elem() : 0, bits_host, out_stride, counts_host,
                    [&](void *in, uint8_t *out, size_t cap) { h->launch(in, n, n, out, cap, h->counts.p); });
  });
}

int sdrhip_psk31_set_channel(sdrhip_psk31 *h, int channel, double dF) {
  return guarded([&] {
    require_channel(h, channel);
    require_df(dF, channel);
    h->ctx->use();
    const float2 p = make_float2((float)(-dF), (float)dF);
    float s[PSK_STATE];
    h->fresh_row(s);
    replace_row(h->ctx, h->par_dev.p + channel, h->par[channel], p, h->st.p + (size_t)channel * PSK_STATE, s, sizeof s);
  });
}

int sdrhip_psk31_reset(sdrhip_psk31 *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}

int sdrhip_psk31_get_state(sdrhip_psk31 *h, float *P, float *F, float *mu, float *omega, int *hist_idx, int *last, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    h->ctx->use();
    // the head of every row's state (the 8 floats before c0): a 2-D copy, 32 bytes of each row
    std::vector<float> s((size_t)h->C * 8);
    const hipError_t e = hipMemcpy2DAsync(s.data(), 8 * sizeof(float), h->st.p, PSK_STATE * sizeof(float), 8 * sizeof(float), (size_t)h->C,
                                          hipMemcpyDeviceToHost, h->ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(h->ctx->stream);
    SDRHIP_CHECK_HIP(e);
    SDRHIP_CHECK_HIP(e2);
    for (int c = 0; c < h->C; c++) {
      const float *r = &s[(size_t)c * 8];
      if (P) P[c] = r[ST_P];
      if (F) F[c] = r[ST_F];
      if (mu) mu[c] = r[ST_MU];
      if (omega) omega[c] = r[ST_OMEGA];
      if (hist_idx) memcpy(&hist_idx[c], &r[ST_HIDX], sizeof(int));
      if (last) memcpy(&last[c], &r[ST_LAST], sizeof(int));
    }
  });
}

int sdrhip_psk31_plan_info(sdrhip_psk31 *h, size_t n, int *tile_samples, int *channels_per_group) {
  return guarded([&] {
    (void)n;   // one geometry for every call length
    write_tile_plan(h, tile_samples, channels_per_group, PSK_T, PSK_G);
  });
}

int sdrhip_psk31_kernel_names(sdrhip_psk31 *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->dtype == SDRHIP_PSK31_CS16 ? "psk31_cs16_kernel" : "psk31_cf32_kernel"; });
  });
}

int sdrhip_psk31_destroy(sdrhip_psk31 *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
