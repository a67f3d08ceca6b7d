// agc.hip — the AGC bank (sdrhip_agc.h): `channels` reference AGC<int16_t> / AGC<float> nodes (src/utils.hh:658-793), one launch
// per call. The node is a per-sample recursion, but only two of its operations are a chain: sd <- fl(fl(lambda * sd) + c) with
// c = fl((1 - lambda) * |x|). c, the x4, the division, the product and the conversion are independent per sample. A lone wave's
// chain is bound by its SIMD's issue port (4 cycles per instruction), so the division (scale / rcp / fma sequence) must not sit
// in it. A workgroup of AGC_THREADS lanes takes AGC_G rows, AGC_T samples at a time, in three phases:
//   1  all lanes: load x (coalesced along the rows, kept in registers for phase 3), write c into the LDS tile;
//   2  one lane per row walks its row of c in LDS and replaces it with sd, the reads of the next eight running ahead;
//   3  all lanes: sd and x -> gain, product, conversion, store (coalesced).
// AGC_G is small on purpose: the chain costs the same for 1 or 64 lanes, phases 1 and 3 scale with the rows of the group, and a
// 1024-row bank is spread over 256 CUs instead of 16 (measured at 1024 x 8192 int16: 0.282 ms with 16 rows per group).
// The tile's leading dimension is odd (AGC_LD): the chain lanes (row = lane, same sample) fall on AGC_G different banks, the
// row-wise lanes (same row, sample = lane) on consecutive ones.
//
// Numerics: every product, the sum and the division must be rounded on their own. In this toolchain __fmul_rn / __fadd_rn /
// __fdiv_rn are plain x * y, x + y and x / y, and neither they nor a contraction pragma stop the backend from fusing under
// -ffp-contract=fast. What the code relies on is agc_mul below: its product passes through an empty asm statement, so no
// multiply-add can be formed from it, whatever the build's contraction mode (checked: the device code has the same multiplies,
// adds and fmas with -ffp-contract=off, which the library's Makefile passes, and with fast). The division relies on hipcc's
// default, the correctly rounded fp32 division (the Makefile sets no flag that relaxes it). f32 denormals are kept (hipcc's
// default kernel mode; no flush flag): after a long silence sd is denormal, 4 * sd exact and the gain +inf, as on the host.
#include "sdrhip_internal.hpp"
#include "sdrhip_agc.h"
#include "entry.hpp"

#include <cmath>

using namespace sdrhip;

namespace {

constexpr int AGC_G = 4, AGC_T = 256, AGC_LD = AGC_T + 1, AGC_THREADS = 256;
constexpr int AGC_CHANNELS_MAX = 65535;
static_assert(AGC_T == AGC_THREADS, "phases 1 and 3: lane t takes sample t of every row of the tile");

struct AgcArgs {
  const void *in; void *out;
  long in_stride, out_stride;
  int N, C;
  const float4 *par;   // lambda, 1 - lambda, target, enabled (1 / 0)
  float2 *st;          // sd, gain
};

// (the empty asm makes the product a value of its own: it costs no instruction and keeps it out of any fused multiply-add)
__device__ __forceinline__ float agc_mul(float a, float b) { float p = a * b; asm("" : "+v"(p)); return p; }
__device__ __forceinline__ float agc_add(float a, float b) { return a + b; }
__device__ __forceinline__ float agc_div(float a, float b) { return a / b; }
__device__ __forceinline__ float agc_abs(short x) { const int v = (int)x; return (float)(v < 0 ? -v : v); }
__device__ __forceinline__ float agc_abs(float x) { return fabsf(x); }
// The reference narrows on x86 with cvttss2si and keeps the low half: out of range, inf and NaN give 0x80000000, low half 0.
// v_cvt_i32_f32 saturates, so the range test is written out.
__device__ __forceinline__ short agc_out(float y, short) { return fabsf(y) < 2147483648.0f ? (short)(unsigned short)(unsigned)(int)y : (short)0; }
__device__ __forceinline__ float agc_out(float y, float) { return y; }

template <class S>
__device__ __forceinline__ void agc_body(const AgcArgs &a) {
  __shared__ float tile[AGC_G * AGC_LD + 8];   // (+ 8: the chain's read-ahead behind the last row's last sample)
  __shared__ float4 spar[AGC_G];
  __shared__ float2 sst[AGC_G];
  const int t = (int)threadIdx.x, c0 = (int)blockIdx.x * AGC_G;
  const int nch = min(AGC_G, a.C - c0);
  if (t < AGC_G) {
    // (a row behind the bank's last: disabled with gain 0, which no phase looks at)
    spar[t] = t < nch ? a.par[c0 + t] : make_float4(0.f, 0.f, 1.f, 0.f);
    sst[t] = t < nch ? a.st[c0 + t] : make_float2(1.f, 0.f);
  }
  __syncthreads();
  // the chain lane's row; a pass-through row (disabled, gain 0) is copied and its state left alone
  const int me = t < AGC_G ? t : 0;
  const float lam = spar[me].x;
  float sd = sst[me].x;
  const bool walk = t < nch && !(spar[me].w == 0.f && sst[me].y == 0.f);
  float *row = tile + me * AGC_LD;
  const S *in = static_cast<const S *>(a.in);
  S *out = static_cast<S *>(a.out);

  for (int n0 = 0; n0 < a.N; n0 += AGC_T) {
    const int cnt = min(AGC_T, a.N - n0);
    S x[AGC_G];
    // phase 1
#pragma unroll
    for (int k = 0; k < AGC_G; k++) {
      x[k] = S(0);
      if (k < nch && t < cnt) {
        x[k] = in[(long)(c0 + k) * a.in_stride + n0 + t];
        tile[k * AGC_LD + t] = agc_mul(spar[k].y, agc_abs(x[k]));
      }
    }
    __syncthreads();
    // phase 2
    if (walk) {
      float c[8], d[8];
#pragma unroll
      for (int j = 0; j < 8; j++) c[j] = row[j];
      int i = 0;
      for (; i + 8 <= cnt; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) d[j] = row[i + 8 + j];   // (at most 8 floats behind the row: inside the tile or its pad)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          sd = agc_add(agc_mul(lam, sd), c[j]);
          row[i + j] = sd;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) c[j] = d[j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (i + j < cnt) {
          sd = agc_add(agc_mul(lam, sd), c[j]);
          row[i + j] = sd;
        }
    }
    __syncthreads();
    // phase 3
#pragma unroll
    for (int k = 0; k < AGC_G; k++)
      if (k < nch && t < cnt) {
        const float4 p = spar[k];
        const float held = sst[k].y;
        S y = x[k];
        if (!(p.w == 0.f && held == 0.f)) {
          const float g = p.w != 0.f ? agc_div(p.z, agc_mul(4.0f, tile[k * AGC_LD + t])) : held;
          y = agc_out(agc_mul(g, (float)x[k]), S());
        }
        out[(long)(c0 + k) * a.out_stride + n0 + t] = y;
      }
    __syncthreads();   // the next tile's phase 1 writes where this phase read
  }
  if (walk && a.N > 0) {
    const float4 p = spar[me];
    a.st[c0 + t] = make_float2(sd, p.w != 0.f ? agc_div(p.z, agc_mul(4.0f, sd)) : sst[me].y);
  }
}

__global__ __launch_bounds__(AGC_THREADS) void agc_i16_kernel(const AgcArgs a) { agc_body<short>(a); }
__global__ __launch_bounds__(AGC_THREADS) void agc_f32_kernel(const AgcArgs a) { agc_body<float>(a); }

bool lambda_ok(float l) { return l >= 0.f && l < 1.f; }
bool target_ok(float t) { return std::isfinite(t) && t > 0.f; }

}  // namespace

struct sdrhip_agc {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_AGC_I16, C = 1;
  size_t max_in = 0;
  std::vector<float4> par;   // the host's copy of the rows' parameters (reset, get_state, the setters' whole-row copies)
  DevBuf<float4> par_dev;
  DevBuf<float2> st;
  Staging stage;
  size_t elem() const { return dtype == SDRHIP_AGC_I16 ? 2 : 4; }

  void fresh_state() {
    std::vector<float2> s((size_t)C);
    for (int c = 0; c < C; c++) s[c] = make_float2(par[c].z, 1.0f);
    put_sync(ctx, st.p, s.data(), s.size() * sizeof(float2));
  }
  void launch(const void *in_dev, size_t N, size_t in_stride, void *out_dev, size_t out_stride) {
    ctx->use();
    if (N == 0) return;
    AgcArgs a;
    a.in = in_dev; a.out = out_dev; a.in_stride = (long)in_stride; a.out_stride = (long)out_stride;
    a.N = (int)N; a.C = C; a.par = par_dev.p; a.st = st.p;
    const dim3 grid((unsigned)ceil_div((size_t)C, (size_t)AGC_G));
    (void)hipGetLastError();
    if (dtype == SDRHIP_AGC_I16) hipLaunchKernelGGL(agc_i16_kernel, grid, dim3(AGC_THREADS), 0, ctx->stream, a);
    else hipLaunchKernelGGL(agc_f32_kernel, grid, dim3(AGC_THREADS), 0, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

static void require_lambda(float l, int c) { SDRHIP_REQUIRE(lambda_ok(l), SDRHIP_E_INVALID, "lambda %g of channel %d outside [0,1)", (double)l, c); }
static void require_target(float t, int c) {
  SDRHIP_REQUIRE(target_ok(t), SDRHIP_E_INVALID, "target %g of channel %d is not a finite number above 0", (double)t, c);
}

// lambda, target, enabled: `channels` entries each, or (one = true) one entry for all rows
static void agc_create(sdrhip_ctx *ctx, int dtype, const float *lambda, const float *target, const int *enabled, bool one, int channels,
                       size_t max_in, sdrhip_agc **out) {
  if (out) *out = nullptr;
  SDRHIP_REQUIRE(out && lambda && target && enabled, SDRHIP_E_INVALID, "NULL argument");
  SDRHIP_REQUIRE(dtype == SDRHIP_AGC_I16 || dtype == SDRHIP_AGC_F32, SDRHIP_E_INVALID, "bad dtype %d", dtype);
  require_channels(channels, AGC_CHANNELS_MAX);
  require_max_in(max_in);
  for (int c = 0; c < (one ? 1 : channels); c++) require_lambda(lambda[c], c);
  for (int c = 0; c < (one ? 1 : channels); c++) require_target(target[c], c);
  require_device_for_null_ctx(ctx);
  make_handle(ctx, out, true, [&](sdrhip_agc *h) {
    h->dtype = dtype; h->C = channels; h->max_in = max_in;
    h->par.resize((size_t)channels);
    for (int c = 0; c < channels; c++) {
      const int k = one ? 0 : c;
      h->par[c] = make_float4(lambda[k], 1.0f - lambda[k], target[k], enabled[k] ? 1.f : 0.f);
    }
    h->par_dev.alloc((size_t)channels);
    h->par_dev.upload(h->par.data(), h->par.size(), ctx->stream);
    h->st.alloc((size_t)channels);
    h->fresh_state();
  });
}

extern "C" {

int sdrhip_design_agc_lambda(double tau, double sample_rate, float *lambda) {
  return guarded([&] {
    SDRHIP_REQUIRE(lambda, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(tau > 0 && sample_rate > 0, SDRHIP_E_INVALID, "tau %g and sample_rate %g must be above 0", tau, sample_rate);
    const float tau_f = (float)tau;   // the reference's member is a float
    *lambda = (float)std::exp(-1.0 / ((double)tau_f * sample_rate));
  });
}

int sdrhip_design_agc_target(int dtype, float *target) {
  return guarded([&] {
    SDRHIP_REQUIRE(target, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(dtype == SDRHIP_AGC_I16 || dtype == SDRHIP_AGC_F32, SDRHIP_E_INVALID, "bad dtype %d", dtype);
    *target = dtype == SDRHIP_AGC_I16 ? 16000.f : 0.5f;
  });
}

int sdrhip_agc_create(sdrhip_ctx *ctx, int dtype, float lambda, float target, int channels, size_t max_in, sdrhip_agc **out) {
  return guarded([&] {
    const int on = 1;
    agc_create(ctx, dtype, &lambda, &target, &on, true, channels, max_in, out);
  });
}

int sdrhip_agcbank_create(sdrhip_ctx *ctx, int dtype, const float *lambda, const float *target, const int *enabled, int channels,
                          size_t max_in, sdrhip_agc **out) {
  return guarded([&] { agc_create(ctx, dtype, lambda, target, enabled, false, channels, max_in, out); });
}

int sdrhip_agc_process_dev(sdrhip_agc *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_agc_process_dev");
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    const Strides s = call_strides("n", n, in_stride, n, out_stride, STRIDES_TOGETHER);
    // in place: every lane reads its samples of a tile before it writes the same ones
    if (!(in_dev == out_dev && s.in == s.out)) require_disjoint(in_dev, s.in, n, h->elem(), out_dev, s.out, n, h->elem(), (size_t)h->C);
    h->launch(in_dev, n, s.in, out_dev, s.out);
  });
}

int sdrhip_agc_process(sdrhip_agc *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_agc_process");
    if (!call_begin(h, "n", n, in_host, out_host)) return;
    const Strides s = call_strides("n", n, in_stride, n, out_stride, STRIDES_TOGETHER);
    const size_t eb = h->elem(), C = (size_t)h->C;
    run_staged(h->ctx, h->stage, C * h->max_in * eb, C * h->max_in * eb, {in_host, s.in * eb, n * eb, C}, {out_host, s.out * eb, n * eb, C},
               [&](void *in, void *out) {
                 h->launch(in, n, n, out, n);
                 return n * eb;
               });
  });
}

int sdrhip_agc_set_channel(sdrhip_agc *h, int channel, float lambda, float target) {
  return guarded([&] {
    require_channel(h, channel);
    require_lambda(lambda, channel);
    require_target(target, channel);
    h->ctx->use();
    const float4 p = make_float4(lambda, 1.0f - lambda, target, 1.f);
    const float2 s = make_float2(target, 1.0f);
    replace_row(h->ctx, h->par_dev.p + channel, h->par[channel], p, h->st.p + channel, &s, sizeof s);
  });
}

int sdrhip_agc_set_lambda(sdrhip_agc *h, int channel, float lambda) {
  return guarded([&] {
    require_channel(h, channel);
    require_lambda(lambda, channel);
    h->ctx->use();
    float4 p = h->par[channel];
    p.x = lambda; p.y = 1.0f - lambda;
    put_sync(h->ctx, h->par_dev.p + channel, &p, sizeof p);
    h->par[channel] = p;
  });
}

int sdrhip_agc_set_enabled(sdrhip_agc *h, int channel, int enabled) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    float4 p = h->par[channel];
    p.w = enabled ? 1.f : 0.f;
    put_sync(h->ctx, h->par_dev.p + channel, &p, sizeof p);
    h->par[channel] = p;
  });
}

int sdrhip_agc_set_gain(sdrhip_agc *h, int channel, float gain) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    put_sync(h->ctx, &h->st.p[channel].y, &gain, sizeof gain);
  });
}

int sdrhip_agc_get_state(sdrhip_agc *h, float *gain, float *sd, int *enabled, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    h->ctx->use();
    std::vector<float2> s((size_t)h->C);
    get_sync(h->ctx, s.data(), h->st.p, s.size() * sizeof(float2));
    for (int c = 0; c < h->C; c++) {
      if (sd) sd[c] = s[c].x;
      if (gain) gain[c] = s[c].y;
      if (enabled) enabled[c] = h->par[c].w != 0.f;
    }
  });
}

int sdrhip_agc_plan_info(sdrhip_agc *h, size_t n, int *tile_samples, int *channels_per_group) {
  return guarded([&] {
    (void)n;   // one geometry for every call length
    write_tile_plan(h, tile_samples, channels_per_group, AGC_T, AGC_G);
  });
}

int sdrhip_agc_kernel_names(sdrhip_agc *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->dtype == SDRHIP_AGC_I16 ? "agc_i16_kernel" : "agc_f32_kernel"; });
  });
}

int sdrhip_agc_reset(sdrhip_agc *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}

int sdrhip_agc_destroy(sdrhip_agc *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
