// resample.hip — the interpolating resampler bank (sdrhip_resample.h): `channels` reference InpolSubSampler<iScalar, oScalar>
// nodes (src/subsample.hh:194-288), one launch per call. The node looks sequential — a float phase mu decides per trip whether a
// sample is consumed or an output taken — but the phase chain does not depend on the samples: which window of the input and which
// table row every output takes is a function of frac, the carried mu and n alone. So the chain is walked as bookkeeping, and every
// output is then an independent 8-tap dot product. A workgroup of RS_THREADS lanes takes RS_G rows, RS_T input samples at a time:
//   1  all lanes: load the tile (coalesced along the rows) into LDS behind each row's carried line of 8, in the output type;
//   2  one lane per row (all in wave 0) walks the row's mu chain over the tile's inputs and writes, for every output, the position
//      of its window in the tile and its table row into the row's LDS list. It touches no sample, so it needs no barrier behind
//      phase 1 and runs beside it;
//   3  all lanes: the listed outputs, each 8 LDS reads of the window and 8 of the table row (the table is resident in LDS), the
//      type's accumulation, a store at the row's running output offset. Then the last 8 samples become the next tile's line.
// The list holds a tile's worst case (frac = 0.125: 8 outputs per input, RS_LIST entries); at frac > RS_T whole tiles list nothing.
// A row with frac == 1 is the reference's short cut: phase 3 copies its samples, its state is not touched.
//
// Numerics (the contract in sdrhip_resample.h): every product is rounded on its own — rs_mul passes it through an empty asm
// statement, so no multiply-add can be formed from it whatever the build's contraction mode (agc.hip). mu * 128 is exact; the
// chain's own operations are one subtraction or one addition per trip. Denormals are kept (no flush flag).
#include "sdrhip_internal.hpp"
#include "sdrhip_resample.h"
#include "entry.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace sdrhip;

namespace {

constexpr int RS_G = 4, RS_T = 256, RS_THREADS = 256, RS_LD = RS_T + 8;
constexpr int RS_LIST = 8 * RS_T + 16;   // floor((T + 1) / 0.125) + 2 = 8 T + 10 outputs of one tile at most
constexpr int RS_SPARE = RS_LIST - 1;    // the entry no output uses
constexpr int RS_CHANNELS_MAX = 65535, RS_ROWS = 129, RS_TAPS = 8, RS_TABLE = RS_ROWS * RS_TAPS;
constexpr float RS_FRAC_MIN = 0.125f, RS_FRAC_MAX = 4096.f;
// a row's state in device memory, in floats: mu - - - | line[8][2] (a real type uses the first 8; int16 values are kept as floats)
constexpr int ST_MU = 0, ST_LINE = 4, RS_STATE = 20;
static_assert(RS_T == RS_THREADS, "phase 1: lane t takes sample t of every row of the tile");
static_assert(RS_G * RS_TAPS <= 64, "the lanes that carry the lines forward sit in one wave: they all read before any writes");
static_assert(RS_T < (1 << 23), "a list entry is (position << 8) | table row");

struct RsArgs {
  const void *in; void *out; uint32_t *counts;
  long in_stride, out_stride;
  int N, C;
  unsigned cap;        // the outputs a row may write
  const float *table;  // [129][8]
  const float *frac;   // [C]
  float *st;           // [C][RS_STATE]
};

// (the empty asm makes the product a value of its own: it costs no instruction and keeps it out of any fused multiply-add)
__device__ __forceinline__ float rs_mul(float a, float b) { float p = a * b; asm("" : "+v"(p)); return p; }
// The reference narrows on x86 with cvttss2si and keeps the low half: out of range, inf and NaN give 0x80000000, low half 0.
// v_cvt_i32_f32 saturates, so the range test is written out (agc.hip).
__device__ __forceinline__ short rs_i16(float y) { return fabsf(y) < 2147483648.0f ? (short)(unsigned short)(unsigned)(int)y : (short)0; }

// a sample entering the line, in the line's (= the output's) type
__device__ __forceinline__ float rs_enter(float v, float) { return v; }
__device__ __forceinline__ float2 rs_enter(float2 v, float2) { return v; }
__device__ __forceinline__ short rs_enter(short v, short) { return v; }
__device__ __forceinline__ float2 rs_enter(short2 v, float2) { return make_float2((float)v.x, (float)v.y); }

// the 8 taps over the window w[0 ... 8) with the table row h
__device__ __forceinline__ float rs_interp(const float *w, const float *h) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < RS_TAPS; k++) acc = acc + rs_mul(w[k], h[k]);
  return acc;
}
__device__ __forceinline__ float2 rs_interp(const float2 *w, const float *h) {
  float re = 0.f, im = 0.f;
#pragma unroll
  for (int k = 0; k < RS_TAPS; k++) {
    const float2 v = w[k];
    re = re + rs_mul(v.x, h[k]);
    im = im + rs_mul(v.y, h[k]);
  }
  return make_float2(re, im);
}
__device__ __forceinline__ short rs_interp(const short *w, const float *h) {
  short acc = 0;
#pragma unroll
  for (int k = 0; k < RS_TAPS; k++) acc = rs_i16((float)acc + rs_mul((float)w[k], h[k]));
  return acc;
}

__device__ __forceinline__ void rs_line_load(float &v, const float *s, int j) { v = s[j]; }
__device__ __forceinline__ void rs_line_load(float2 &v, const float *s, int j) { v = make_float2(s[2 * j], s[2 * j + 1]); }
__device__ __forceinline__ void rs_line_load(short &v, const float *s, int j) { v = (short)s[j]; }
__device__ __forceinline__ void rs_line_store(float v, float *s, int j) { s[j] = v; }
__device__ __forceinline__ void rs_line_store(float2 v, float *s, int j) { s[2 * j] = v.x; s[2 * j + 1] = v.y; }
__device__ __forceinline__ void rs_line_store(short v, float *s, int j) { s[j] = (float)v; }

template <class I, class L>
__device__ __forceinline__ void rs_body(const RsArgs &a) {
  __shared__ L buf[RS_G * RS_LD];            // per row: the line (8), then the tile
  __shared__ float tab[RS_TABLE];
  __shared__ unsigned list[RS_G * RS_LIST];   // per row: (window position << 8) | table row of the tile's outputs
  __shared__ float frac_s[RS_G];
  __shared__ unsigned nout_s[RS_G], obase_s[RS_G];
  const int t = (int)threadIdx.x, c0 = (int)blockIdx.x * RS_G;
  const int nch = min(RS_G, a.C - c0);

  for (int i = t; i < RS_TABLE; i += RS_THREADS) tab[i] = a.table[i];
  if (t < RS_G) {
    frac_s[t] = t < nch ? a.frac[c0 + t] : 1.0f;   // (a row behind the bank's last: a pass-through nobody copies)
    nout_s[t] = 0;
    obase_s[t] = 0;
  }
  // the lanes that keep the lines: lane t has sample t % 8 of row t / 8
  const int lrow = t / RS_TAPS, lj = t % RS_TAPS;
  const bool liner = t < RS_G * RS_TAPS && lrow < nch;
  L carry = L();
  if (liner) {
    rs_line_load(carry, a.st + (long)(c0 + lrow) * RS_STATE + ST_LINE, lj);
    buf[lrow * RS_LD + lj] = carry;
  }
  // the chain lanes: lane t walks row t
  const bool chain = t < nch;
  const float frac = chain ? a.frac[c0 + t] : 1.0f;
  const bool walk = chain && frac != 1.0f;
  float mu = walk ? a.st[(long)(c0 + t) * RS_STATE + ST_MU] : 0.f;
  bool fill = true;       // the reference's loop a call is in: the first (fill the line) or the second (take outputs)
  unsigned o = 0;
  const I *in = static_cast<const I *>(a.in);
  L *out = static_cast<L *>(a.out);
  __syncthreads();

  for (int n0 = 0; n0 < a.N; n0 += RS_T) {
    const int cnt = min(RS_T, a.N - n0);
    const bool last = n0 + RS_T >= a.N;
    // phase 1
#pragma unroll
    for (int k = 0; k < RS_G; k++)
      if (k < nch && t < cnt) buf[k * RS_LD + RS_TAPS + t] = rs_enter(in[(long)(c0 + k) * a.in_stride + n0 + t], L());
    // phase 2
    if (walk) {
      unsigned *mine = list + t * RS_LIST;
      int i = 0;
      unsigned nl = 0;
      // Every trip but a turn from the second loop to the first consumes a sample or lists an output. Written as selects, not
      // branches: the trip is the kernel's critical path, and the rows of a group take different ones. A trip that lists
      // nothing stores into the list's spare last entry.
      bool done = false;
      for (int trip = 0; trip < 2 * RS_T + RS_LIST + 4 && !done; trip++) {
        const bool ge1 = mu >= 1.0f, le1 = mu <= 1.0f, have = i < cnt;
        const bool push = fill && ge1 && have;
        const bool pause = fill && ge1 && !have && !last;   // the first loop goes on in the next tile
        const bool emit = !push && !pause && le1;
        const bool turn = !push && !pause && !le1;          // mu > 1: back to the first loop while input is left
        int r = (int)roundf(rs_mul(mu, 128.0f));
        r = min(max(r, 0), RS_ROWS - 1);
        mine[emit && nl < (unsigned)RS_SPARE ? nl : (unsigned)RS_SPARE] = ((unsigned)i << 8) | (unsigned)r;
        // the first loop's pushes in one trip: mu - 1 is exact for 1 <= mu < 2^24, so k of them are mu - k, k = floor(mu) at most
        const int k = min((int)mu, cnt - i);
        mu = push ? mu - (float)k : emit ? mu + frac : mu;
        i += push ? k : 0;
        nl += emit ? 1u : 0u;
        fill = !emit && (push || turn || fill);
        done = pause || (turn && !have);                    // (a turn without input, in the last tile: the call ends)
      }
      nout_s[t] = min(nl, (unsigned)RS_SPARE);
      obase_s[t] = o;
      o += nl;
    }
    __syncthreads();
    // phase 3
#pragma unroll
    for (int k = 0; k < RS_G; k++) {
      if (k >= nch) continue;
      L *orow = out + (long)(c0 + k) * a.out_stride;
      const L *brow = buf + k * RS_LD;
      if (frac_s[k] == 1.0f) {
        if (t < cnt && (unsigned)(n0 + t) < a.cap) orow[n0 + t] = brow[RS_TAPS + t];
        continue;
      }
      const unsigned nk = nout_s[k], base = obase_s[k];
      for (unsigned j = (unsigned)t; j < nk; j += RS_THREADS) {
        const unsigned e = list[k * RS_LIST + j];
        const L y = rs_interp(brow + (e >> 8), tab + (e & 255u) * RS_TAPS);
        if (base + j < a.cap) orow[base + j] = y;
      }
    }
    if (liner) carry = buf[lrow * RS_LD + cnt + lj];   // the 8 last samples, read before the barrier, written behind it
    __syncthreads();
    if (liner) buf[lrow * RS_LD + lj] = carry;
  }
  if (a.N > 0) {
    if (chain) a.counts[c0 + t] = walk ? min(o, a.cap) : min((unsigned)a.N, a.cap);
    if (walk) a.st[(long)(c0 + t) * RS_STATE + ST_MU] = mu;
    if (liner && frac_s[lrow] != 1.0f) rs_line_store(carry, a.st + (long)(c0 + lrow) * RS_STATE + ST_LINE, lj);
  }
}

__global__ __launch_bounds__(RS_THREADS) void resample_f32_kernel(const RsArgs a) { rs_body<float, float>(a); }
__global__ __launch_bounds__(RS_THREADS) void resample_cf32_kernel(const RsArgs a) { rs_body<float2, float2>(a); }
__global__ __launch_bounds__(RS_THREADS) void resample_i16_kernel(const RsArgs a) { rs_body<short, short>(a); }
__global__ __launch_bounds__(RS_THREADS) void resample_cs16_cf32_kernel(const RsArgs a) { rs_body<short2, float2>(a); }

bool frac_ok(float f) { return std::isfinite(f) && f >= RS_FRAC_MIN && f <= RS_FRAC_MAX; }
bool dtype_ok(int d) { return d >= SDRHIP_RESAMPLE_F32 && d <= SDRHIP_RESAMPLE_CS16_CF32; }

}  // namespace

struct sdrhip_resample {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_RESAMPLE_F32, C = 1;
  size_t max_in = 0;
  std::vector<float> frac;   // the host's copy of the rows' frac
  float frac_least = 1.f;    // the smallest frac of a row that resamples (1 where none does), and whether a row passes through
  bool any_pass = false;
  DevBuf<float> frac_dev, table, st;
  DevBuf<uint32_t> counts;   // of the host-pointer calls
  Staging stage;
  size_t in_elem() const { return dtype == SDRHIP_RESAMPLE_F32 ? 4 : dtype == SDRHIP_RESAMPLE_CF32 ? 8 : dtype == SDRHIP_RESAMPLE_I16 ? 2 : 4; }
  size_t out_elem() const { return dtype == SDRHIP_RESAMPLE_F32 ? 4 : dtype == SDRHIP_RESAMPLE_I16 ? 2 : 8; }
  int components() const { return dtype == SDRHIP_RESAMPLE_CF32 || dtype == SDRHIP_RESAMPLE_CS16_CF32 ? 2 : 1; }

  void survey() {
    frac_least = RS_FRAC_MAX; any_pass = false;
    bool any = false;
    for (float f : frac) {
      if (f == 1.0f) any_pass = true;
      else { frac_least = std::min(frac_least, f); any = true; }
    }
    if (!any) frac_least = 1.f;
  }
  // the header's bound, the largest over the rows (floor((n + 1) / frac) + 2 falls as frac grows)
  size_t capacity(size_t n) const {
    if (n == 0) return 0;
    size_t cap = any_pass ? n : 0;
    if (frac_least != 1.f) cap = std::max(cap, (size_t)std::floor(((double)n + 1.0) / (double)frac_least) + 2);
    return cap;
  }
  void fresh_state() {
    std::vector<float> s((size_t)C * RS_STATE, 0.f);
    put_sync(ctx, st.p, s.data(), s.size() * sizeof(float));
  }
  void launch(const void *in_dev, size_t N, size_t in_stride, void *out_dev, size_t out_stride, uint32_t *counts_dev) {
    ctx->use();
    if (N == 0) return;
    RsArgs a;
    a.in = in_dev; a.out = out_dev; a.counts = counts_dev; a.in_stride = (long)in_stride; a.out_stride = (long)out_stride;
    a.N = (int)N; a.C = C; a.cap = (unsigned)std::min(std::min(capacity(N), out_stride), (size_t)0xffffffffu);
    a.table = table.p; a.frac = frac_dev.p; a.st = st.p;
    const dim3 grid((unsigned)ceil_div((size_t)C, (size_t)RS_G)), block(RS_THREADS);
    (void)hipGetLastError();
    switch (dtype) {
      case SDRHIP_RESAMPLE_F32: hipLaunchKernelGGL(resample_f32_kernel, grid, block, 0, ctx->stream, a); break;
      case SDRHIP_RESAMPLE_CF32: hipLaunchKernelGGL(resample_cf32_kernel, grid, block, 0, ctx->stream, a); break;
      case SDRHIP_RESAMPLE_I16: hipLaunchKernelGGL(resample_i16_kernel, grid, block, 0, ctx->stream, a); break;
      default: hipLaunchKernelGGL(resample_cs16_cf32_kernel, grid, block, 0, ctx->stream, a); break;
    }
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

static void require_frac(float f, int c) {
  SDRHIP_REQUIRE(frac_ok(f), SDRHIP_E_INVALID, "frac %g of channel %d is not a finite number in [0.125,4096]", (double)f, c);
}

// frac: `channels` entries, or (one = true) one entry for all rows
static void rs_create(sdrhip_ctx *ctx, int dtype, const float *frac, bool one, const float *table, int channels, size_t max_in,
                      sdrhip_resample **out) {
  if (out) *out = nullptr;
  SDRHIP_REQUIRE(out && table && frac, SDRHIP_E_INVALID, "NULL argument");
  SDRHIP_REQUIRE(dtype_ok(dtype), SDRHIP_E_INVALID, "bad dtype %d", dtype);
  require_channels(channels, RS_CHANNELS_MAX);
  require_max_in(max_in);
  for (int c = 0; c < (one ? 1 : channels); c++) require_frac(frac[c], c);
  for (int i = 0; i < RS_TABLE; i++) SDRHIP_REQUIRE(std::isfinite(table[i]), SDRHIP_E_INVALID, "table entry %d is not finite", i);
  require_device_for_null_ctx(ctx);
  make_handle(ctx, out, true, [&](sdrhip_resample *h) {
    h->dtype = dtype; h->C = channels; h->max_in = max_in;
    h->frac.resize((size_t)channels);
    for (int c = 0; c < channels; c++) h->frac[c] = frac[one ? 0 : c];
    h->survey();
    h->frac_dev.alloc((size_t)channels);
    h->frac_dev.upload(h->frac.data(), h->frac.size(), ctx->stream);
    h->table.alloc(RS_TABLE);
    h->table.upload(table, RS_TABLE, ctx->stream);
    h->st.alloc((size_t)channels * RS_STATE);
    h->counts.alloc((size_t)channels);
    h->fresh_state();
  });
}

extern "C" {

int sdrhip_resample_create(sdrhip_ctx *ctx, int dtype, float frac, const float *table, int channels, size_t max_in, sdrhip_resample **out) {
  return guarded([&] { rs_create(ctx, dtype, &frac, true, table, channels, max_in, out); });
}

int sdrhip_resamplebank_create(sdrhip_ctx *ctx, int dtype, const float *frac, const float *table, int channels, size_t max_in,
                               sdrhip_resample **out) {
  return guarded([&] { rs_create(ctx, dtype, frac, false, table, channels, max_in, out); });
}

int sdrhip_resample_out_capacity(sdrhip_resample *h, size_t n, size_t *outputs) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && outputs, SDRHIP_E_INVALID, "NULL argument");
    *outputs = h->capacity(n);
  });
}

int sdrhip_resample_process_dev(sdrhip_resample *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t out_stride,
                                uint32_t *counts_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_resample_process_dev");
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    SDRHIP_REQUIRE(counts_dev, SDRHIP_E_INVALID, "NULL buffer");
    const size_t cap = h->capacity(n);
    const Strides s = call_strides("n", n, in_stride, cap, out_stride, STRIDE_IN | STRIDE_OUT, "capacity");
    require_disjoint(in_dev, s.in, n, h->in_elem(), out_dev, s.out, cap, h->out_elem(), (size_t)h->C);
    h->launch(in_dev, n, s.in, out_dev, s.out, counts_dev);
  });
}

int sdrhip_resample_process(sdrhip_resample *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t out_stride,
                            uint32_t *counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_resample_process");
    process_counted(h, in_host, n, in_stride, h ? h->in_elem() : 0, static_cast<uint8_t *>(out_host), out_stride, counts_host,
                    [&](void *in, uint8_t *out, size_t cap) { h->launch(in, n, n, out, cap, h->counts.p); }, h ? h->out_elem() : 1);
  });
}

int sdrhip_resample_set_channel(sdrhip_resample *h, int channel, float frac) {
  return guarded([&] {
    require_channel(h, channel);
    require_frac(frac, channel);
    h->ctx->use();
    const float s[RS_STATE] = {0.f};
    replace_row(h->ctx, h->frac_dev.p + channel, h->frac[channel], frac, h->st.p + (size_t)channel * RS_STATE, s, sizeof s);
    h->survey();
  });
}

int sdrhip_resample_reset(sdrhip_resample *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}

int sdrhip_resample_get_state(sdrhip_resample *h, float *frac, float *mu, float *line_f32, int16_t *line_i16, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    h->ctx->use();
    std::vector<float> s((size_t)h->C * RS_STATE);
    get_sync(h->ctx, s.data(), h->st.p, s.size() * sizeof(float));
    const int w = RS_TAPS * h->components();
    const bool i16 = h->dtype == SDRHIP_RESAMPLE_I16;
    for (int c = 0; c < h->C; c++) {
      const float *r = &s[(size_t)c * RS_STATE];
      if (frac) frac[c] = h->frac[c];
      if (mu) mu[c] = r[ST_MU];
      for (int j = 0; j < w; j++) {
        if (i16 && line_i16) line_i16[(size_t)c * w + j] = (int16_t)r[ST_LINE + j];
        if (!i16 && line_f32) line_f32[(size_t)c * w + j] = r[ST_LINE + j];
      }
    }
  });
}

int sdrhip_resample_plan_info(sdrhip_resample *h, size_t n, int *tile_samples, int *channels_per_group) {
  return guarded([&] {
    (void)n;   // one geometry for every call length
    write_tile_plan(h, tile_samples, channels_per_group, RS_T, RS_G);
  });
}

int sdrhip_resample_kernel_names(sdrhip_resample *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] {
      return h->dtype == SDRHIP_RESAMPLE_F32 ? "resample_f32_kernel" : h->dtype == SDRHIP_RESAMPLE_CF32 ? "resample_cf32_kernel"
             : h->dtype == SDRHIP_RESAMPLE_I16 ? "resample_i16_kernel" : "resample_cs16_cf32_kernel";
    });
  });
}

int sdrhip_resample_destroy(sdrhip_resample *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
